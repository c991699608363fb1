#!/usr/bin/env python3
"""Device time of pfq_prep_reads' adapter step, between HIP events (pfq_debug_last_adapters), on the block of tools/prep_bench.py:
--reads (8 388 608) synthetic reads of 150 bases from the benchmark's tree with that tool's qualities and parameters.  Every
second read carries read-through: behind an insert of 20 .. 149 bases the 33-base adapter and a random tail.

Three runs, each the median of --steps calls after --warmup:
    no adapters set        trim + mark (pfq_debug_last_prep ms[0]): the yardstick, the code path without this step;
    1 adapter, 8 adapters  the adapter kernels, and trim + mark, the scans, offsets + gather of the same calls;
    the bytes the adapter kernels must move (the bases and the offsets in, cut and which out) over their time against the
    6.3 TB/s a streaming kernel reaches on this chip.
Writes --text afresh.
Usage: tools/adapter_bench.py [--reads 8388608] [--steps 3] [--warmup 1] [--leaves 1024] [--text profiles/adapter_bench.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from prep_bench import GENOME_LEN, HBM_TBS, K, NBITS, NUM_HASHES, PARAMS, READ_LEN, make_block  # noqa: E402
from sim_bench import build  # noqa: E402

ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
O, E = 5, 10


def plant(seq_t, n_reads):
    """Read-through into every second read of the page-locked block, in place; returns the number of reads that carry it."""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(777)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    ad = torch.tensor(list(ADAPTER), dtype=torch.uint8, device="cuda")
    pos = torch.arange(READ_LEN, device="cuda", dtype=torch.int64)[None, :]
    step = 1 << 20
    for r0 in range(0, n_reads, step):
        r1 = min(n_reads, r0 + step)
        rows = (r1 - r0 + 1) // 2
        block = seq_t[r0 * READ_LEN:r1 * READ_LEN].cuda().reshape(r1 - r0, READ_LEN)
        insert = torch.randint(20, READ_LEN, (rows, 1), device="cuda", generator=gen, dtype=torch.int64)
        tail = letters[torch.randint(0, 4, (rows, READ_LEN), device="cuda", generator=gen)]
        behind = pos - insert                                         # < 0: the insert; < 33: the adapter; else the tail
        planted = torch.where(behind < 0, block[0::2], torch.where(behind < len(ADAPTER), ad[behind.clamp(0, len(ADAPTER) - 1)], tail))
        block[0::2] = planted
        seq_t[r0 * READ_LEN:r1 * READ_LEN].copy_(block.reshape(-1))
    torch.cuda.synchronize()
    return (n_reads + 1) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8 * 1024 * 1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--leaves", type=int, default=1024)
    ap.add_argument("--text", default=os.path.join(ROOT, "profiles", "adapter_bench.txt"))
    args = ap.parse_args()
    tree = build(args.leaves, GENOME_LEN, K, NBITS, NUM_HASHES)
    seq_t, qual_t, off = make_block(args.leaves, args.reads)
    n_planted = plant(seq_t, args.reads)
    seq, qual = seq_t.numpy(), qual_t.numpy()
    rng = np.random.default_rng(5)
    others = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), len(ADAPTER)).astype(np.uint8)) for _ in range(7)]
    lines = [f"adapter_bench: {args.reads} reads of {READ_LEN} bases, {n_planted} with read-through into a {len(ADAPTER)}-base adapter; O={O} E={E}; " +
             " ".join(f"{k}={v}" for k, v in PARAMS.items()) + f"; median of {args.steps} after {args.warmup}"]
    yardstick = None
    for name, adapters in (("no adapters", []), ("1 adapter", [ADAPTER]), ("8 adapters", [ADAPTER, *others])):
        tree.set_adapters(adapters, min_overlap=O, max_error_percent=E)
        rows, res, found = [], None, None
        for it in range(args.warmup + args.steps):
            res = tree.prep_reads(seq, off, qual, **PARAMS)
            ms = tree.last_prep_ms()
            if adapters:
                found = tree.last_adapters()
            if it >= args.warmup:
                rows.append((tree.last_adapters_ms() if adapters else 0.0, *ms))
        med = [statistics.median(r[i] for r in rows) for i in range(4)]
        if not adapters:
            yardstick = med[1]
            lines.append(f"  {name}: trim + mark {med[1]:.3f} ms (the yardstick), scans {med[2]:.3f} ms, offsets + gather {med[3]:.3f} ms; kept {res['n_kept']} reads, "
                         f"{res['bases_kept']} of {res['bases_in']} bases")
            continue
        moved = res["bases_in"] + 8 * (args.reads + 1) + 5 * args.reads
        rate = moved / (med[0] * 1e-3) / 1e12
        lines.append(f"  {name}: adapter kernels {med[0]:.3f} ms = {med[0] / yardstick:.2f} x the yardstick; trim + mark {med[1]:.3f} ms, scans {med[2]:.3f} ms, "
                     f"offsets + gather {med[3]:.3f} ms")
        lines.append(f"    cut {found['n_found']} reads ({found['bases_cut']} bases; per adapter {found['found'][:len(adapters)]}); kept {res['n_kept']} reads, "
                     f"{res['bases_kept']} of {res['bases_in']} bases")
        lines.append(f"    the adapter kernels move {moved / 1e9:.3f} GB (bases and offsets in, cut and which out): {rate:.2f} TB/s = {100 * rate / HBM_TBS:.0f} % of the "
                     f"{HBM_TBS} TB/s streaming rate")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.text)), exist_ok=True)
    with open(args.text, "w") as f:
        f.write(text)
    tree.close()


if __name__ == "__main__":
    main()
