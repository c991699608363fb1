#!/usr/bin/env python3
"""Device time of the mate overlap kernel with the mate correction (pfq_tree_set_mate_correct) against the same kernel without it,
between HIP events (pfq_debug_last_overlap), on the block of tools/overlap_bench.py: --reads (8 388 608) reads of 150 bases as
fragments, every second one with an insert of 30 .. 149 bases.

Two blocks.  In the first no overlap carries a mismatch; in the second --percent (10) of the overlapping fragments carry one
substitution in mate 2 with quality '#' against quality 'I' in mate 1.  On each block the settings alternate call by call in one
process — correction off (the baseline), on, and on the second block also on with want_reads (the patch list: the overlap kernel
counts, then the scan and the patch kernel of pfq_debug_last_corrections) — and the medians of --steps calls after --warmup are
reported as ratios to the baseline of the same block, with the spread (min .. max) of the baseline's own calls.  Writes --text afresh.
Usage: tools/correct_bench.py [--reads 8388608] [--steps 5] [--warmup 1] [--percent 10] [--text profiles/correct_bench.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from overlap_bench import E, O, plant  # noqa: E402
from prep_bench import GENOME_LEN, K, NBITS, NUM_HASHES, PARAMS, READ_LEN, make_block  # noqa: E402
from sim_bench import build  # noqa: E402

HIGH, LOW = 30, 14


def spoil(seq, qual, insert, percent, rng):
    """One low-quality substitution at base 5 of mate 2 in `percent` of the fragments with read-through, in place."""
    through = np.flatnonzero(insert < READ_LEN)
    chosen = through[rng.random(through.size) < percent / 100.0].astype(np.int64)
    at2 = (2 * chosen + 1) * READ_LEN + 5
    at1 = 2 * chosen * READ_LEN + insert[chosen].astype(np.int64) - 6
    swap = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"CGTA"):
        swap[a] = b
    seq[at2] = swap[seq[at2]]
    qual[at2] = ord("#")
    qual[at1] = ord("I")
    return chosen.size, through.size


def measure(tree, seq, off, qual, settings, steps, warmup):
    """Alternating calls; per setting the overlap kernel's ms of every measured call, the patch kernels' ms and the last totals."""
    times = {name: [] for name, _, _ in settings}
    extra = {name: [] for name, _, _ in settings}
    last = {}
    for it in range(warmup + steps):
        for name, high, want_reads in settings:
            tree.set_mate_correct(high, LOW if high else 0)
            tree.prep_reads(seq, off, qual, paired=True, want_reads=want_reads, **PARAMS)
            if it >= warmup:
                times[name].append(tree.last_overlap_ms())
                if high and want_reads:
                    extra[name].append(tree.last_corrections_ms())
            if high:
                last[name] = tree.last_corrections()
    return times, extra, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8 * 1024 * 1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--leaves", type=int, default=1024)
    ap.add_argument("--percent", type=float, default=10.0)
    ap.add_argument("--text", default=os.path.join(ROOT, "profiles", "correct_bench.txt"))
    args = ap.parse_args()
    if args.reads % 4:
        ap.error("--reads must be a multiple of 4: every second fragment is planted")
    tree = build(args.leaves, GENOME_LEN, K, NBITS, NUM_HASHES)
    seq_t, qual_t, off = make_block(args.leaves, args.reads)
    n_planted = plant(seq_t, args.reads)
    seq, qual = seq_t.numpy(), qual_t.numpy()
    tree.set_mate_overlap(O, E)
    lines = [f"correct_bench: {args.reads} reads of {READ_LEN} bases as {args.reads // 2} fragments, {n_planted} with an insert of 30 .. {READ_LEN - 1} bases; O={O} E={E}; "
             f"high={HIGH} low={LOW}; " + " ".join(f"{k}={v}" for k, v in PARAMS.items()) + f"; alternating, median of {args.steps} after {args.warmup}"]
    off_on = (("off", 0, False), ("on", HIGH, False))

    def report(title, times, extra, last, names):
        base = statistics.median(times["off"])
        lines.append(f"  {title}: correction off {base:.3f} ms (the baseline; its calls {min(times['off']):.3f} .. {max(times['off']):.3f} ms, "
                     f"spread {100 * (max(times['off']) - min(times['off'])) / base:.1f} %)")
        for name in names:
            t = statistics.median(times[name])
            c = last[name]
            more = f"; scan + patch kernel {statistics.median(extra[name]):.3f} ms more = {statistics.median(extra[name]) / base:.3f} x" if extra[name] else ""
            lines.append(f"    {name}: overlap kernel {t:.3f} ms = {t / base:.3f} x the baseline ({min(times[name]):.3f} .. {max(times[name]):.3f} ms){more}; "
                         f"{sum(c['n_bases'])} bases corrected in {c['n_fragments_corrected']} fragments, {c['n_unresolved']} unresolved")

    times, extra, last = measure(tree, seq, off, qual, off_on, args.steps, args.warmup)
    report("0 % of the overlapping fragments carry a mismatch", times, extra, last, ["on"])
    tree.set_mate_correct(0)
    tree.prep_reads(seq, off, qual, paired=True, want_reads=True, **PARAMS)
    insert = tree.last_overlap()["insert"]
    n_spoiled, n_through = spoil(seq, qual, insert, args.percent, np.random.default_rng(779))
    settings = (*off_on, ("on, want_reads", HIGH, True))
    times, extra, last = measure(tree, seq, off, qual, settings, args.steps, args.warmup)
    report(f"{n_spoiled} of the {n_through} fragments with read-through ({100 * n_spoiled / max(n_through, 1):.1f} %) carry one low-quality mismatch", times, extra, last,
           ["on", "on, want_reads"])
    text = "# tools/correct_bench.py on one MI355X; the committed kernels\n" + "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.text)), exist_ok=True)
    with open(args.text, "w") as f:
        f.write(text)
    tree.close()


if __name__ == "__main__":
    main()
