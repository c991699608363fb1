#!/usr/bin/env python3
"""Rate of the paired-end query (PFQ_PAIRED) against the same mates unpaired, on the config-3 geometry: balanced 1024-leaf SBT
of 50 kbp genomes, nbits 71 887 936, 10 hashes, k 21; 8 388 608 reads of 150 bp per call (4 194 304 fragments: reads 2i and
2i + 1 are mates), resident in HBM, half of them from the genomes, all with 1 % substitutions.  For every threshold: reads/s
of pfq_query_batch_device with PFQ_WANT_HITS, then with PFQ_WANT_HITS | PFQ_PAIRED in mode `either` and in mode `both`, timed
with HIP events around the calls (warm-up calls excluded).  Prints one JSON line.
Usage: tools/pair_bench.py [--steps S] [--warmup W] [--thresholds 1.0,0.7,0.3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_G, GLEN, RL, B = 1024, 50000, 150, 8388608
K, NBITS, H = 21, 71887936, 10
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
GENOME_SEED, READ_SEED = 0x5EED0000, 0x5EED1234


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--thresholds", default="1.0,0.7,0.3")
    ap.add_argument("--errors", type=float, default=0.01)
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
    reads = torch.empty(B * RL + 64, dtype=torch.uint8, device=dev)
    _ffi.check(L.pfq_synth_reads_device(reads.data_ptr(), 0, B, RL, genomes.data_ptr(), GLEN, N_G, READ_SEED, None))
    torch.cuda.synchronize()
    if args.errors > 0:
        gen = torch.Generator(device=dev)
        gen.manual_seed(777)
        view = reads[:B * RL]
        mut = torch.rand(view.numel(), device=dev, generator=gen) < args.errors
        alt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (view.numel(),), device=dev, generator=gen)]
        view.copy_(torch.where(mut, alt, view))
        del mut, alt
    del genomes
    off = torch.arange(B + 1, dtype=torch.int64, device=dev) * RL
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    def rate(thr: float, paired: bool, mode: str = "either"):
        call = lambda: tree.query_device_hits(reads.data_ptr(), off.data_ptr(), B, B * RL, thr, stream, paired=paired, pair_mode=mode)
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        ms, hits = 0.0, 0
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = call()
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
            hits = int(res[0][-1])
        return B * args.steps / (ms * 1e-3), ms / args.steps, hits

    out = {"workload": f"{B} reads x {RL} bp per call = {B // 2} fragments ({args.errors:.0%} substitutions), balanced {N_G}-leaf "
                       f"SBT, k={K}, nbits={NBITS}, {H} hashes", "steps": args.steps, "warmup": args.warmup, "thresholds": {}}
    for thr in (float(x) for x in args.thresholds.split(",")):
        r0, ms0, h0 = rate(thr, False)
        r1, ms1, h1 = rate(thr, True, "either")
        r2, ms2, h2 = rate(thr, True, "both")
        assert h2 <= h1 <= h0
        out["thresholds"][str(thr)] = {"hits_unpaired": h0, "reads_per_s_unpaired": round(r0), "ms_unpaired": round(ms0, 3),
                                       "hits_either": h1, "reads_per_s_either": round(r1), "ms_either": round(ms1, 3),
                                       "hits_both": h2, "reads_per_s_both": round(r2), "ms_both": round(ms2, 3),
                                       "overhead_either": round(ms1 / ms0 - 1, 4), "overhead_both": round(ms2 / ms0 - 1, 4)}
    tree.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
