#!/usr/bin/env python3
"""Device time of pfq_prep_deplete on one MI355X, written to profiles/deplete_bench.txt (HIP events throughout).

The block is the benchmark's: 8 Mi reads of 150 bases, half of them drawn by the synthetic read generator from a 16-genome
screen and half from the 1024-genome database; the generator makes every second read random, so a quarter of the block is
the screen's.  The block is prepared (quality trimming off, --min-length = k: every read is kept, so the prep's scans and
gather move the whole block), then depleted, three times after one warm-up; reported are pfq_debug_last_prep ms[1] + ms[2]
(scans, offsets and gather of the whole block) against pfq_debug_last_deplete ms[1] (mark, scans, offsets and gather of what
is left) of the same block in the same process, and ms[0], the screen's classification.

The wall-clock comparison with the two-run pipeline of the parent commit (query --neg-filter against the screen, then a run on
NEG_FILTERING) needs a build of that commit next to this one: pass --parent-cli PATH and --reads FILE --db DIR --screen DIR; it
runs both three times, alternating.  Without them the section says "not measured"."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, NBITS, H, SEEDS = 21, 2875517, 10, (0x0123456789ABCDEF, 0xFEDCBA9876543210)


def device_time(lines, n_reads, rl, thr):
    import numpy as np
    import torch
    from phagefilter_amd import BloomTree, _ffi
    L = _ffi.lib()
    dev = torch.device("cuda:0")
    glen = 50000

    def tree(n_g, seed, prefix):
        g = torch.empty(n_g * glen, dtype=torch.uint8, device=dev)
        _ffi.check(L.pfq_synth_genomes_device(g.data_ptr(), n_g, glen, seed, None))
        torch.cuda.synchronize()
        t = BloomTree.build_balanced_device(g.data_ptr(), glen, n_g, [f"{prefix}{i:05d}" for i in range(n_g)], K, NBITS, H, *SEEDS, 0.001, 5000000)
        return g, t

    main_g, main = tree(1024, 0x5EED0000, "G")
    screen_g, screen = tree(16, 0x5C4EE000, "S")
    half = n_reads // 2
    reads = torch.empty(n_reads * rl + 64, dtype=torch.uint8, device=dev)
    _ffi.check(L.pfq_synth_reads_device(reads.data_ptr(), 0, half, rl, screen_g.data_ptr(), glen, 16, 0x5EED1234, None))
    _ffi.check(L.pfq_synth_reads_device(reads.data_ptr() + half * rl, half, n_reads - half, rl, main_g.data_ptr(), glen, 1024, 0x5EED1234, None))
    torch.cuda.synchronize()
    seq = reads.cpu().numpy()
    off = np.arange(n_reads + 1, dtype=np.uint64) * rl
    lines.append(f"block: {n_reads} reads of {rl} bases; screen: 16 leaves, main: 1024 leaves, k {K}, {NBITS} bits, {H} hashes; threshold {thr}")
    lines.append("run  prep ms[1]+ms[2]  deplete ms[1]  ratio  deplete ms[0] (screen)  units removed  call wall ms")
    for run in range(4):
        prep = main.prep_reads(seq, off, min_length=K)
        p = main.last_prep_ms()
        t0 = time.perf_counter()
        got = main.prep_deplete(screen, thr)
        wall = (time.perf_counter() - t0) * 1e3
        d = main.last_deplete_ms()
        assert prep["n_kept"] == n_reads and got["n_units"] == n_reads
        tag = "warm-up" if run == 0 else str(run)
        lines.append(f"{tag:>7}  {p[1] + p[2]:9.3f}  {d[1]:9.3f}  {d[1] / (p[1] + p[2]):5.2f}  {d[0]:9.3f}  {got['units_removed']}  {wall:9.1f}")
    for t in (main, screen):
        t.close()


def wall_clock(lines, a):
    if not (a.parent_cli and a.reads and a.db and a.screen):
        lines.append("wall-clock, fused run against the parent commit's two-run pipeline: not measured")
        return
    cli = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
    out = a.out_dir

    def timed(cmd):
        t0 = time.perf_counter()
        subprocess.run(cmd, check=True, capture_output=True, timeout=1200)
        return time.perf_counter() - t0

    common = ["--threads", "16", "-f", str(a.threshold)]
    for run in range(3):
        fused = timed([cli, "query", "-r", a.reads, "-d", a.db, "-o", out + "/fused", "--deplete", a.screen, *common])
        two = {}
        for tag, extra in (("host writers", []), ("--device-output", ["--device-output"])):
            first = timed([a.parent_cli, "query", "-r", a.reads, "-d", a.screen, "-o", out + "/neg", "--neg-filter", *extra, *common])
            neg = [f for f in os.listdir(out + "/neg") if f.startswith("NEG_FILTERING")][0]
            second = timed([a.parent_cli, "query", "-r", os.path.join(out, "neg", neg), "-d", a.db, "-o", out + "/second", *common])
            two[tag] = (first, second)
        lines.append(f"wall-clock run {run + 1}: fused {fused:.2f} s; two runs " +
                     "; ".join(f"{tag}: {x:.2f} + {y:.2f} = {x + y:.2f} s" for tag, (x, y) in two.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads-per-block", type=int, default=8 * 1024 * 1024)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--threshold", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deplete_bench.txt"))
    ap.add_argument("--parent-cli")
    ap.add_argument("--reads")
    ap.add_argument("--db")
    ap.add_argument("--screen")
    ap.add_argument("--out-dir", default="/tmp/deplete_bench")
    a = ap.parse_args()
    lines = ["pfq_prep_deplete on one MI355X (tools/deplete_bench.py); device milliseconds from HIP events"]
    device_time(lines, a.reads_per_block, a.read_len, a.threshold)
    wall_clock(lines, a)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
