#!/usr/bin/env python3
"""Device time of pfq_prep_reads' mate overlap step, between HIP events (pfq_debug_last_overlap), on the block of
tools/prep_bench.py taken as fragments: --reads (8 388 608) synthetic reads of 150 bases from the benchmark's tree, reads 2f and
2f + 1 the mates of fragment f, with that tool's qualities and parameters.  Every second fragment has an insert of 30 .. 149
bases: mate 1 is the insert, the 33-base adapter and a random tail, mate 2 the insert's reverse complement and a random tail.  The
other fragments keep their two unrelated reads and do not overlap.

Four runs in one session, each the median of --steps calls after --warmup, all with paired=True:
    nothing set            trim + mark (pfq_debug_last_prep ms[0]): the yardstick, the code path without this step;
    1 adapter              the adapter kernels;
    the overlap            the overlap kernel, and trim + mark, the scans, offsets + gather of the same calls;
    1 adapter + overlap    every piece of the prep, and the threshold-1 classification of the prepared block (pfq_prep_query with
                           fragments, between HIP events): the prep of a block runs while the block before it is classified, so it
                           is hidden as long as adapter + overlap + trim + scans + gather stay below the classification.
Writes --text afresh.
Usage: tools/overlap_bench.py [--reads 8388608] [--steps 3] [--warmup 1] [--leaves 1024] [--text profiles/overlap_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from prep_bench import GENOME_LEN, K, NBITS, NUM_HASHES, PARAMS, READ_LEN, make_block  # noqa: E402
from sim_bench import build  # noqa: E402

ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
O, E = 30, 10
ADAPTER_O, ADAPTER_E = 5, 10


def plant(seq_t, n_reads):
    """Read-through into every second fragment of the page-locked block, in place; returns the number of fragments that carry it."""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(778)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    comp = torch.arange(256, dtype=torch.uint8, device="cuda")
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    ad = torch.tensor(list(ADAPTER), dtype=torch.uint8, device="cuda")
    pos = torch.arange(READ_LEN, device="cuda", dtype=torch.int64)[None, :]
    step = 1 << 20                                                    # reads a slice: a multiple of 4, so slices begin at a planted fragment
    planted = 0
    for r0 in range(0, n_reads - n_reads % 2, step):
        r1 = min(n_reads - n_reads % 2, r0 + step)
        block = seq_t[r0 * READ_LEN:r1 * READ_LEN].cuda().reshape(r1 - r0, READ_LEN)
        rows = (r1 - r0 + 3) // 4
        insert = torch.randint(30, READ_LEN, (rows, 1), device="cuda", generator=gen, dtype=torch.int64)
        tails = letters[torch.randint(0, 4, (2, rows, READ_LEN), device="cuda", generator=gen)]
        first = block[0::4]
        behind = pos - insert                                         # < 0: the insert; < 33: the adapter; else the tail
        block[0::4] = torch.where(behind < 0, first, torch.where(behind < len(ADAPTER), ad[behind.clamp(0, len(ADAPTER) - 1)], tails[0]))
        mirrored = comp[torch.gather(first, 1, (insert - 1 - pos).clamp(min=0)).long()]
        block[1::4] = torch.where(behind < 0, mirrored, tails[1])
        seq_t[r0 * READ_LEN:r1 * READ_LEN].copy_(block.reshape(-1))
        planted += rows
    torch.cuda.synchronize()
    return planted


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8 * 1024 * 1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--leaves", type=int, default=1024)
    ap.add_argument("--text", default=os.path.join(ROOT, "profiles", "overlap_bench.txt"))
    args = ap.parse_args()
    if args.reads % 4:
        ap.error("--reads must be a multiple of 4: every second fragment is planted")
    tree = build(args.leaves, GENOME_LEN, K, NBITS, NUM_HASHES)
    seq_t, qual_t, off = make_block(args.leaves, args.reads)
    n_planted = plant(seq_t, args.reads)
    seq, qual = seq_t.numpy(), qual_t.numpy()
    lines = [f"overlap_bench: {args.reads} reads of {READ_LEN} bases as {args.reads // 2} fragments, {n_planted} with an insert of 30 .. {READ_LEN - 1} bases, a "
             f"{len(ADAPTER)}-base adapter behind it in mate 1; O={O} E={E}; adapter O={ADAPTER_O} E={ADAPTER_E}; " + " ".join(f"{k}={v}" for k, v in PARAMS.items()) +
             f"; median of {args.steps} after {args.warmup}"]
    yardstick = None
    for name, adapters, overlap in (("nothing set", [], 0), ("1 adapter", [ADAPTER], 0), ("the overlap", [], O), ("1 adapter + the overlap", [ADAPTER], O)):
        tree.set_adapters(adapters, min_overlap=ADAPTER_O, max_error_percent=ADAPTER_E)
        tree.set_mate_overlap(overlap, E)
        rows, res, found = [], None, None
        for it in range(args.warmup + args.steps):
            res = tree.prep_reads(seq, off, qual, paired=True, **PARAMS)
            ms = tree.last_prep_ms()
            if overlap:
                found = tree.last_overlap()
            classify = 0.0
            if adapters and overlap:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tree.query_prep(1.0, paired=True)
                e1.record()
                e1.synchronize()
                classify = e0.elapsed_time(e1)
                tree.reset_counts()
            if it >= args.warmup:
                rows.append((tree.last_adapters_ms() if adapters else 0.0, tree.last_overlap_ms() if overlap else 0.0, *ms, classify))
        ad, ov, trim, scans, gather, classify = (statistics.median(r[i] for r in rows) for i in range(6))
        kept = f"kept {res['n_kept']} reads, {res['bases_kept']} of {res['bases_in']} bases"
        if not adapters and not overlap:
            yardstick = trim
            lines.append(f"  {name}: trim + mark {trim:.3f} ms (the yardstick), scans {scans:.3f} ms, offsets + gather {gather:.3f} ms; {kept}")
            continue
        parts = ([f"adapter kernels {ad:.3f} ms = {ad / yardstick:.2f} x the yardstick"] if adapters else []) + \
                ([f"overlap kernel {ov:.3f} ms = {ov / yardstick:.2f} x the yardstick"] if overlap else [])
        lines.append(f"  {name}: " + "; ".join(parts) + f"; trim + mark {trim:.3f} ms, scans {scans:.3f} ms, offsets + gather {gather:.3f} ms; {kept}")
        if overlap:
            lines.append(f"    {found['n_overlapped']} of {found['n_analysed']} fragments overlap, {found['n_readthrough']} with read-through: {found['reads_cut']} reads cut "
                         f"({found['bases_cut']} bases); {int(found['hist'][30:READ_LEN].sum())} inserts of 30 .. {READ_LEN - 1} bases")
        if adapters and overlap:
            prep = ad + ov + trim + scans + gather
            lines.append(f"    the whole prep {prep:.3f} ms against the threshold-1 classification of the prepared fragments {classify:.3f} ms: "
                         f"{prep / classify:.2f} of it, {'hidden behind it' if prep < classify else 'NOT hidden behind it'}")
    text = "# tools/overlap_bench.py on one MI355X; the committed kernels\n" + "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.text)), exist_ok=True)
    with open(args.text, "w") as f:
        f.write(text)
    tree.close()


if __name__ == "__main__":
    main()
