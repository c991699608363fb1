#!/usr/bin/env python3
"""Rate of the headline query on TRIMMED reads — lengths drawn uniformly from --min-len .. --max-len (100 .. 150 bp), which
bench.py's arguments cannot express: balanced 1024-leaf SBT of 50 kbp genomes, nbits 71 887 936, 10 hashes, k 21, threshold 1;
8 388 608 reads per call, resident in HBM, half of them from the genomes (the generator's 150 bp reads cut to their length).
Every last-window shape of k_tail_records is in play at once here (tails of 16 .. 64 and 1 .. 2 k-mers at k = 21), so this is
the guard against trading trimmed reads for the benchmark's uniform ones.  pfq_query_batch_device timed with HIP events around
the calls (warm-up calls excluded).  Prints one JSON line.
Usage: tools/trimmed_bench.py [--steps S] [--warmup W] [--min-len 100] [--max-len 150]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_G, GLEN, B = 1024, 50000, 8388608
K, NBITS, H = 21, 71887936, 10
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
GENOME_SEED, READ_SEED, LENGTH_SEED = 0x5EED0000, 0x5EED1234, 4242


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-len", type=int, default=100)
    ap.add_argument("--max-len", type=int, default=150)
    args = ap.parse_args()
    import torch
    from phagefilter_amd import BloomTree, _ffi
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    genomes = torch.empty(N_G * GLEN, dtype=torch.uint8, device=dev)
    _ffi.check(L.pfq_synth_genomes_device(genomes.data_ptr(), N_G, GLEN, GENOME_SEED, None))
    torch.cuda.synchronize()
    ids = [f"G{i:05d}" for i in range(N_G)]
    tree = BloomTree.build_balanced_device(genomes.data_ptr(), GLEN, N_G, ids, K, NBITS, H, SEEDS[0], SEEDS[1], 0.001, 5000000)
    rl = args.max_len
    full = torch.empty(B * rl + 64, dtype=torch.uint8, device=dev)
    _ffi.check(L.pfq_synth_reads_device(full.data_ptr(), 0, B, rl, genomes.data_ptr(), GLEN, N_G, READ_SEED, None))
    torch.cuda.synchronize()
    del genomes
    gen = torch.Generator(device=dev)
    gen.manual_seed(LENGTH_SEED)
    lens = torch.randint(args.min_len, args.max_len + 1, (B,), device=dev, generator=gen, dtype=torch.int64)
    off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    keep = torch.arange(rl, device=dev)[None, :] < lens[:, None]  # row-major selection = the reads' prefixes, packed
    reads = torch.cat([full[:B * rl].view(B, rl)[keep], torch.zeros(64, dtype=torch.uint8, device=dev)])
    assert reads.numel() == total + 64
    del full, keep
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: tree.query_device(reads.data_ptr(), off.data_ptr(), B, total, 1.0, stream)
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    tree.reset_counts()
    ms = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    st = tree.last_stats()
    counted = sum(c for _, c in tree.get_leaf_counts())
    out = {"workload": f"{B} reads of {args.min_len} .. {args.max_len} bp (uniform) per call, balanced {N_G}-leaf SBT, k={K}, "
                       f"nbits={NBITS}, {H} hashes, threshold 1", "steps": args.steps, "warmup": args.warmup,
           "reads_per_s": round(B * args.steps / (sum(ms) * 1e-3)), "ms_per_step": round(sum(ms) / args.steps, 3),
           "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "path": st.path, "tile_mode": st.tile_mode,
           "pair_stage": getattr(st, "pair_stage", None), "reads_counted": counted}
    tree.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
