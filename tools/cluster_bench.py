#!/usr/bin/env python3
"""Device times of pfq_tree_recluster's stages, between HIP events (option PFQ_CLUSTER_TIME, pfq_debug_last_recluster), on
synthetic trees built on the device (pfq_synth_genomes_device + pfq_tree_build_balanced_device):
    config-3 geometry:  1024 leaves, k 21, nbits 71 887 936, 10 hashes;
    harness geometry:  10 010 leaves, k 20, nbits 11 981 322, 17 hashes (the reference's own benchmark size).
Per geometry: the scores stage (shared bits of all leaf pairs on or above the diagonal, in panels, and their scores), all rounds
(kernels, the read-back of every round's merges and the unions of the new filters), the nearest-neighbour kernel alone summed
over the rounds, the rounds, and that kernel's score-matrix bytes (live rows x row pitch x 8, summed over the rounds) over its
time against the 6.3 TB/s a streaming kernel reaches on this chip.  The median of --steps calls after --warmup.

Then what the new shape buys a query (--skip-families leaves it out): a database of --families strain families of --strains
genomes (--genome-len bases, --rate substitutions per base) and unrelated genomes up to --leaves, inserted by the greedy
pfq_tree_insert in shuffled order, against its re-clustered form: tree height, and for --reads reads of 150 bases with 1 %
errors at threshold 0.3, pfq_stats.group_reads (the (read, leaf group) screens of the two-level frontier) and reads/s by the
host clock round the call and the read-out of the counters.  Appends to --text.
Usage: tools/cluster_bench.py [--steps 3] [--warmup 1] [--skip-config3] [--skip-harness] [--skip-families] [--text profiles/cluster_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from phagefilter_amd import BloomTree, pack_reads  # noqa: E402
from sim_bench import SEEDS, build  # noqa: E402

HBM_TBS = 6.3
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def stages(tree, steps, warmup):
    rows = []
    for it in range(warmup + steps):
        t0 = time.time()
        new = tree.recluster()
        wall = time.time() - t0
        r = tree.last_recluster()
        height = max(c[1] for c in new.clades()) if it == 0 else 0
        new.close()
        if it >= warmup:
            rows.append((r["scores_ms"], r["rounds_ms"], r["nearest_ms"], wall * 1e3, r["nearest_bytes"], r["rounds"]))
        if it == 0:
            first_height = height
    med = [statistics.median(x[i] for x in rows) for i in range(4)]
    return med, rows[0][4], rows[0][5], first_height


def families_db(n_leaves, n_fam, strains, length, rate, rng):
    genomes = []
    for _ in range(n_fam):
        base = ACGT[rng.integers(0, 4, length)]
        for _ in range(strains):
            g = base.copy()
            pos = rng.choice(length, size=rng.binomial(length, rate), replace=False)
            g[pos] = ACGT[(np.searchsorted(ACGT, g[pos]) + rng.integers(1, 4, len(pos))) % 4]
            genomes.append(g.tobytes())
    genomes += [ACGT[rng.integers(0, 4, length)].tobytes() for _ in range(n_leaves - len(genomes))]
    order = rng.permutation(len(genomes))
    return [genomes[i] for i in order]


def query_rate(tree, seq, off, n_reads, steps, warmup):
    times, group_reads, groups = [], 0, 0
    for it in range(warmup + steps):
        tree.reset_counts()
        t0 = time.time()
        tree.query_packed(seq, off, 0.3)
        total = sum(c for _, c in tree.get_leaf_counts())                     # (waits for the call)
        dt = time.time() - t0
        st = tree.last_stats()
        group_reads, groups = int(st.group_reads), int(st.leaf_groups)
        if it >= warmup:
            times.append(dt)
    return n_reads / statistics.median(times), group_reads, groups, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-config3", action="store_true")
    ap.add_argument("--skip-harness", action="store_true")
    ap.add_argument("--skip-families", action="store_true")
    ap.add_argument("--leaves", type=int, default=10010)
    ap.add_argument("--families", type=int, default=1500)
    ap.add_argument("--strains", type=int, default=4)
    ap.add_argument("--genome-len", type=int, default=5000)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--reads", type=int, default=400000)
    ap.add_argument("--text", default=os.path.join(ROOT, "profiles", "cluster_bench.txt"))
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for tag, skip, n, glen, k, nbits, h in (("config 3", a.skip_config3, 1024, 50000, 21, 71887936, 10),
                                             ("harness geometry", a.skip_harness, 10010, 5000, 20, 11981322, 17)):
        if skip:
            continue
        tree = build(n, glen, k, nbits, h)
        tree.set_option("PFQ_CLUSTER_TIME", "1")
        (scores, rounds_ms, nn, wall), nn_bytes, rounds, height = stages(tree, a.steps, a.warmup)
        tree.close()
        rate = nn_bytes / 1e12 / (nn * 1e-3) if nn > 0 else 0.0
        say(f"{tag}: {n} leaves, nbits {nbits}, {h} hashes: scores {scores:.1f} ms, rounds {rounds_ms:.2f} ms ({rounds} rounds, height {height}), of which "
            f"nearest-neighbour kernel {nn:.3f} ms reading {nn_bytes / 1e6:.1f} MB of scores = {rate:.3f} TB/s, {100 * rate / HBM_TBS:.1f} % of the "
            f"{HBM_TBS} TB/s a streaming kernel reaches; whole call {wall:.1f} ms by the host clock (median of {a.steps} after {a.warmup})")
    if not a.skip_families:
        rng = np.random.default_rng(1009)
        genomes = families_db(a.leaves, a.families, a.strains, a.genome_len, a.rate, rng)
        t0 = time.time()
        greedy = BloomTree.new(21, 0.001, a.genome_len, *SEEDS, expected_genomes=len(genomes))
        for i, g in enumerate(genomes):
            greedy.insert(g, f"G{i:05d}")
        h_greedy = max(c[1] for c in greedy.clades())
        t1 = time.time()
        new = greedy.recluster()
        t2 = time.time()
        h_new = max(c[1] for c in new.clades())
        reads = []
        for _ in range(a.reads):
            g = genomes[int(rng.integers(0, len(genomes)))]
            o = int(rng.integers(0, len(g) - 150))
            r = bytearray(g[o:o + 150])
            r[int(rng.integers(0, 150))] = ord("ACGT"[int(rng.integers(0, 4))])
            reads.append(bytes(r))
        seq, off = pack_reads(reads)
        say(f"families: {a.leaves} leaves = {a.families} families of {a.strains} strains ({a.genome_len} bases, {a.rate} substitutions per base) and "
            f"unrelated genomes, shuffled; greedy build {t1 - t0:.1f} s, recluster {t2 - t1:.2f} s ({new.merge_rounds()} rounds); {a.reads} reads of 150 bases, "
            f"threshold 0.3")
        results = []
        for tag, tree, height in (("greedy", greedy, h_greedy), ("reclustered", new, h_new)):
            rate, group_reads, groups, total = query_rate(tree, seq, off, a.reads, a.steps, a.warmup)
            results.append(total)
            say(f"  {tag}: height {height}, {groups} leaf groups, group_reads {group_reads} ({group_reads / a.reads:.2f} per read), "
                f"{rate / 1e6:.2f} M reads/s, {total} hits counted")
        assert results[0] == results[1], "the two trees count different hits"
        new.close()
        greedy.close()
    os.makedirs(os.path.dirname(a.text), exist_ok=True)
    with open(a.text, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
