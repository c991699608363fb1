#!/usr/bin/env python3
"""Device time of pfq_tree_similarity's intersection kernel, all leaves x all leaves, on synthetic trees built on the device
(pfq_synth_genomes_device + pfq_tree_build_balanced_device):
    config-3 geometry:  1024 leaves, k 21, nbits 71 887 936, 10 hashes — the tiled kernel at its built-in slices and the
                        one-block-per-pair kernel (PFQ_SIM_NAIVE=1), the yardstick, on the same tree in the same run;
    harness geometry:  10 010 leaves, k 20, nbits 11 981 322, 17 hashes (the reference's own benchmark size) — tiled only.
The matrix is asked for in panels as `phage_filter compare` asks: at most 1024 leaves of a by as many of b as stay under 2^26
pairs, only the panels on or above the diagonal.  A repeat's time is the sum over its panels of the kernel's device time between
two HIP events round the launch (option PFQ_SIM_TIME, pfq_debug_last_similarity); the median of --steps repeats after --warmup is reported, with
    word pairs  = sum over panels of n_a * n_b * ceil(nbits / 64),
    VALU share  = word pairs * 4 operations (and, bit count with accumulate, on both 32-bit halves) / (1024 SIMDs * 16 lanes * clock * time),
    bytes asked = tiled: what the tiles must read: per panel, tiles of 128 x 128 leaves, each reading its 256 rows once
                  (ragged tiles: the rows they have), against the filters' own size; naive: both rows of every pair.
--slices tries other slice counts on the config-3 tree as well.  Appends to --text.
Usage: tools/sim_bench.py [--steps 5] [--warmup 1] [--clock-ghz 2.4] [--skip-naive] [--skip-harness] [--slices 8,32] [--text profiles/sim_bench.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phagefilter_amd import BloomTree, _ffi  # noqa: E402

SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
PANEL_A, MAX_PAIRS, TILE = 1024, 1 << 26, 128


def panels(n):
    """(a0, a1, b0, b1) of `phage_filter compare` without --against."""
    out = []
    for a0 in range(0, n, PANEL_A):
        a1 = min(n, a0 + PANEL_A)
        pb = MAX_PAIRS // (a1 - a0)
        for b0 in range(a0, n, pb):
            out.append((a0, a1, b0, min(n, b0 + pb)))
    return out


def build(n_leaves, genome_len, k, nbits, h):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), n_leaves * genome_len) == 0
    _ffi.check(_ffi.lib().pfq_synth_genomes_device(d, n_leaves, genome_len, 0x5EED0000, None))
    assert hip.hipDeviceSynchronize() == 0
    t = BloomTree.build_balanced_device(d.value, genome_len, n_leaves, [f"G{i:05d}" for i in range(n_leaves)], k, nbits, h, *SEEDS,
                                        largest_expected_genome=5000000)
    assert hip.hipFree(d) == 0
    return t


def run(tree, n, steps, warmup):
    """Median over `steps` repeats of the summed kernel time of all panels (ms); the slices of the first panel; a checksum."""
    times, slices, check = [], 0, 0
    for it in range(warmup + steps):
        total = 0.0
        for (a0, a1, b0, b1) in panels(n):
            s = tree.similarity(leaves_a=np.arange(a0, a1, dtype=np.uint32), leaves_b=np.arange(b0, b1, dtype=np.uint32))
            ms, sl = tree.last_similarity()
            total += ms
            slices = slices or sl
            if it == 0:
                check += int(s["shared_bits"].sum(dtype=np.uint64))
        if it >= warmup:
            times.append(total)
    return statistics.median(times), min(times), max(times), slices, check


def arithmetic(n, nbits):
    words = (nbits + 63) // 64
    pairs = sum((a1 - a0) * (b1 - b0) for a0, a1, b0, b1 in panels(n))
    tile_rows = 0
    for a0, a1, b0, b1 in panels(n):
        for ta in range(a0, a1, TILE):
            for tb in range(b0, b1, TILE):
                tile_rows += min(TILE, a1 - ta) + min(TILE, b1 - tb)
    return pairs, pairs * words, tile_rows * words * 8, n * words * 8, pairs * 2 * words * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--skip-naive", action="store_true")
    ap.add_argument("--skip-harness", action="store_true")
    ap.add_argument("--slices", default="")
    ap.add_argument("--text", default=os.path.join(ROOT, "profiles", "sim_bench.txt"))
    a = ap.parse_args()
    lines = []

    def report(tag, n, nbits, h, med, lo, hi, slices, check, naive=False):
        pairs, word_pairs, hbm, filters, per_pair = arithmetic(n, nbits)
        asked = (f"pairs read {per_pair / 1e12:.2f} TB (two rows per pair, {per_pair / filters:.0f} x the filters' {filters / 1e9:.2f} GB) = "
                 f"{per_pair / 1e12 / (med * 1e-3):.1f} TB/s asked of the memory system" if naive else
                 f"tiles read {hbm / 1e9:.1f} GB ({hbm / filters:.1f} x the filters' {filters / 1e9:.2f} GB) = {hbm / 1e9 / (med * 1e-3):.0f} GB/s if none of it hit a cache")
        valu = word_pairs * 4 / (1024 * 16 * a.clock_ghz * 1e9 * med * 1e-3)
        line = (f"{tag}: {n} leaves, nbits {nbits}, {h} hashes, {len(panels(n))} panel(s), {pairs} pairs, {word_pairs:.4g} word pairs, slices {slices}: "
                f"median {med:.2f} ms (min {lo:.2f}, max {hi:.2f}, {a.steps} repeats after {a.warmup}); VALU share {100 * valu:.1f} % of "
                f"1024 SIMDs x 16 lanes x {a.clock_ghz} GHz; {asked}; checksum {check}")
        print(line, flush=True)
        lines.append(line)

    n, nbits, h = 1024, 71887936, 10
    t0 = time.time()
    tree = build(n, 50000, 21, nbits, h)
    tree.set_option("PFQ_SIM_TIME", "1")
    print(f"config-3 tree built in {time.time() - t0:.1f} s", flush=True)
    tiled = run(tree, n, a.steps, a.warmup)
    report("config 3, tiled", n, nbits, h, *tiled)
    for s in [x for x in a.slices.split(",") if x]:
        tree.set_option("PFQ_SIM_SLICES", s)
        r = run(tree, n, a.steps, a.warmup)
        assert r[4] == tiled[4], "checksums differ"
        report(f"config 3, tiled, PFQ_SIM_SLICES={s}", n, nbits, h, *r)
    tree.set_option("PFQ_SIM_SLICES", None)
    if not a.skip_naive:
        tree.set_option("PFQ_SIM_NAIVE", "1")
        naive = run(tree, n, a.steps, a.warmup)
        assert naive[4] == tiled[4], "checksums differ"
        report("config 3, naive (one block per pair)", n, nbits, h, *naive, naive=True)
        line = f"config 3: naive / tiled = {naive[0] / tiled[0]:.1f} x"
        print(line, flush=True)
        lines.append(line)
    tree.close()
    if not a.skip_harness:
        n, nbits, h = 10010, 11981322, 17
        tree = build(n, 5000, 20, nbits, h)
        tree.set_option("PFQ_SIM_TIME", "1")
        report("harness geometry, tiled", n, nbits, h, *run(tree, n, a.steps, a.warmup))
        tree.close()
    os.makedirs(os.path.dirname(a.text), exist_ok=True)
    with open(a.text, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
