#!/usr/bin/env python3
"""Alternated plain bench.py runs of two builds of libpfq on one box: base (another libpfq.so, through PFQ_LIBPFQ) and new (this
tree's).  Prints one line per run and, per scenario, min / max / mean of both builds, the gain of the means and its ratio to
the base's spread (max - min) — the project's bar is every new run above every base run and a gain of at least three spreads.

usage: tools/lib_ab.py <base libpfq.so> <rounds> <name> [VAR=value ...] [-- bench.py arguments]
Stops at the first run that fails or exceeds its time limit (nothing else is started on the device after that)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(lib, env_extra, bench_args, limit):
    env = dict(os.environ, **env_extra)
    if lib:
        env["PFQ_LIBPFQ"] = lib
    else:
        env.pop("PFQ_LIBPFQ", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + bench_args, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stdout.write(p.stderr[-2000:])
        raise SystemExit(f"bench.py exited with {p.returncode}")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def main():
    argv = sys.argv[1:]
    bench_args = ["--steps", "10", "--warmup", "2"]
    if "--" in argv:
        bench_args = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    base, rounds, name = os.path.abspath(argv[0]), int(argv[1]), argv[2]
    env_extra = dict(a.split("=", 1) for a in argv[3:])
    vals = {"B": [], "N": []}
    for i in range(1, rounds + 1):
        for tag, lib in (("B", base), ("N", None)):
            d = run(lib, env_extra, bench_args, 280)
            vals[tag].append(d["value"] / 1e6)
            print("%-12s %7.2f M reads/s  %.3f ms/step  setup %.1f s " % (f"{name}{i}{tag}", d["value"] / 1e6, d["ms_per_step"], d["setup_seconds"]),
                  {k: round(v, 3) for k, v in d["kernel_ms_per_step"].items()}, flush=True)
    b, n = vals["B"], vals["N"]
    mb, mn, spread = sum(b) / len(b), sum(n) / len(n), max(b) - min(b)
    print(f"{name}: base min {min(b):.2f} max {max(b):.2f} mean {mb:.2f} (spread {spread:.2f})   new min {min(n):.2f} max {max(n):.2f} mean {mn:.2f}   "
          f"gain of the means {mn - mb:+.2f} M reads/s = {100 * (mn - mb) / mb:+.2f} % = {(mn - mb) / spread if spread > 0 else float('inf'):.2f} x the base's spread; "
          f"every new run above every base run: {min(n) > max(b)}", flush=True)


if __name__ == "__main__":
    main()
