#!/usr/bin/env python3
"""Device times of pfq_prep_reads' stages, between HIP events (pfq_debug_last_prep), on the benchmark's block: --reads (8 388 608)
synthetic reads of 150 bases drawn from the benchmark's tree (1024 leaves, k 21, nbits 71 887 936, 10 hashes), resident in
page-locked host memory, with synthetic qualities: good up to a per-read point 10 .. 30 bases before the end, then decaying by
3 a base, so that trimming does real work.  Parameters: --trim-quality 20 --trim-window 4 --trim-poly-x 10 --min-length 21.

Per run, the median of --steps calls after --warmup:
    trim + mark, the two scans, offsets + gather (device ms), and the whole pfq_prep_reads call by the host clock (it includes
    the copies of bases, qualities and offsets to the device);
    the bytes the kernels must move (bases + qualities in, kept bases out) over trim + gather against the 6.3 TB/s a streaming
    kernel reaches on this chip;
    pfq_prep_query at threshold 1 (the kept, trimmed block, already on the device) and pfq_query_batch at threshold 1 on the same
    reads untrimmed (from host memory), each by the host clock round the call and the read-out of the counters.
Appends to --text.
Usage: tools/prep_bench.py [--reads 8388608] [--steps 3] [--warmup 1] [--leaves 1024] [--text profiles/prep_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from phagefilter_amd import _ffi  # noqa: E402
from sim_bench import build  # noqa: E402

K, NBITS, NUM_HASHES, GENOME_LEN, READ_LEN = 21, 71887936, 10, 50000, 150
GENOME_SEED, READ_SEED = 0x5EED0000, 0x5EED1234
HBM_TBS = 6.3
PARAMS = dict(trim_quality=20, trim_window=4, poly_x=10, min_length=21)


def make_block(n_leaves, n_reads):
    """The benchmark's reads (pfq_synth_reads_device over the benchmark's genomes) and their qualities, in page-locked memory."""
    import torch
    L = _ffi.lib()
    genomes = torch.empty(n_leaves * GENOME_LEN, dtype=torch.uint8, device="cuda")
    _ffi.check(L.pfq_synth_genomes_device(genomes.data_ptr(), n_leaves, GENOME_LEN, GENOME_SEED, None))
    reads = torch.empty(n_reads * READ_LEN + 64, dtype=torch.uint8, device="cuda")
    _ffi.check(L.pfq_synth_reads_device(reads.data_ptr(), 0, n_reads, READ_LEN, genomes.data_ptr(), GENOME_LEN, n_leaves, READ_SEED, None))
    torch.cuda.synchronize()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4242)
    cut = torch.randint(READ_LEN - 30, READ_LEN - 9, (n_reads, 1), device="cuda", generator=gen, dtype=torch.int16)
    pos = torch.arange(READ_LEN, device="cuda", dtype=torch.int16)[None, :]
    qual = torch.empty(n_reads * READ_LEN + 64, dtype=torch.uint8, device="cuda")
    step = 1 << 20
    for r0 in range(0, n_reads, step):                                # (a slice at a time: the int16 matrix of all reads is 2.5 GB)
        r1 = min(n_reads, r0 + step)
        q = (73 - 3 * (pos - cut[r0:r1]).clamp(min=0)).clamp(min=35).to(torch.uint8)       # 'I' = 40, down to '#' = 2
        qual[r0 * READ_LEN:r1 * READ_LEN] = q.reshape(-1)
    qual[n_reads * READ_LEN:] = 0
    seq_h = torch.empty(reads.numel(), dtype=torch.uint8).pin_memory()
    qual_h = torch.empty(qual.numel(), dtype=torch.uint8).pin_memory()
    seq_h.copy_(reads)
    qual_h.copy_(qual)
    torch.cuda.synchronize()
    del genomes, reads, qual
    torch.cuda.empty_cache()
    off = np.arange(n_reads + 1, dtype=np.uint64) * READ_LEN
    return seq_h, qual_h, off                                          # (the tensors own the page-locked memory)


def counts_sum(tree):
    return sum(c for _, c in tree.get_leaf_counts())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8 * 1024 * 1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--leaves", type=int, default=1024)
    ap.add_argument("--text", default=os.path.join(ROOT, "profiles", "prep_bench.txt"))
    args = ap.parse_args()
    tree = build(args.leaves, GENOME_LEN, K, NBITS, NUM_HASHES)
    seq_t, qual_t, off = make_block(args.leaves, args.reads)
    seq, qual = seq_t.numpy(), qual_t.numpy()
    rows, res = [], None
    for it in range(args.warmup + args.steps):
        t0 = time.time()
        res = tree.prep_reads(seq, off, qual, **PARAMS)
        wall = (time.time() - t0) * 1e3
        trim, scan, gather = tree.last_prep_ms()
        tree.reset_counts()
        t0 = time.time()
        tree.query_prep(1.0)
        hits_prep = counts_sum(tree)
        q_prep = (time.time() - t0) * 1e3
        tree.reset_counts()
        t0 = time.time()
        tree.query_packed(seq, off, 1.0)
        hits_raw = counts_sum(tree)
        q_raw = (time.time() - t0) * 1e3
        if it >= args.warmup:
            rows.append((trim, scan, gather, wall, q_prep, q_raw))
    med = [statistics.median(r[i] for r in rows) for i in range(6)]
    moved = 2 * res["bases_in"] + res["bases_kept"]
    rate = moved / ((med[0] + med[2]) * 1e-3) / 1e12
    lines = [
        f"prep_bench: {args.reads} reads of {READ_LEN} bases, {args.leaves} leaves, k {K}; " + " ".join(f"{k}={v}" for k, v in PARAMS.items()) +
        f"; median of {args.steps} after {args.warmup}",
        f"  kept {res['n_kept']} of {res['n_reads']} reads ({res['n_trimmed']} trimmed), {res['bases_kept']} of {res['bases_in']} bases; dropped " +
        ", ".join(f"{k} {v}" for k, v in res["n_reason"].items() if k != "kept"),
        f"  device: trim + mark {med[0]:.3f} ms, scans {med[1]:.3f} ms, offsets + gather {med[2]:.3f} ms",
        f"  trim + gather move {moved / 1e9:.3f} GB (bases + qualities in, kept bases out): {rate:.2f} TB/s = {100 * rate / HBM_TBS:.0f} % of the "
        f"{HBM_TBS} TB/s streaming rate",
        f"  pfq_prep_reads, host clock (with the copies to the device): {med[3]:.1f} ms",
        f"  threshold 1: pfq_prep_query {med[4]:.1f} ms ({hits_prep} leaf counts); pfq_query_batch of the untrimmed reads from host memory "
        f"{med[5]:.1f} ms ({hits_raw} leaf counts); trim + gather = {100 * (med[0] + med[2]) / med[5]:.1f} % of that call",
    ]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.text)), exist_ok=True)
    with open(args.text, "a") as f:
        f.write(text)
    tree.close()


if __name__ == "__main__":
    main()
