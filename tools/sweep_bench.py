#!/usr/bin/env python3
"""Cost of PFQ_WANT_SWEEP, and one scored pass against one plain run per threshold, on the geometry of tools/cover_bench.py:
balanced 1024-leaf SBT of 50 kbp genomes in families of 8 (so that rows are long), nbits 71 887 936, 10 hashes, k 21; 8 388 608
reads of 150 bp per call, resident in HBM, half of them from the genomes; pfq_query_batch_device on a stream, every call between
two HIP events.  Base threshold 0.3, list 0.3, 0.5, 0.7, 0.9, 1.0.

The workers run in processes of their own, alternated (parent, child, parent again), each timing its variants `--steps` times
after `--warmup` calls:
    parent:  S  PFQ_WANT_HITS | PFQ_WANT_SCORES at the base threshold (what the sweep rides on)
             F  five calls with flags 0, one per threshold of the list: what choosing a threshold costs without the sweep
    child:   the same two; W the scored call with PFQ_WANT_SWEEP, `pass` counted in LDS; G the same with PFQ_SWEEP_LDS=0
The unflagged legs are taken from a libpfq.so built from the parent commit (--parent-lib) as well, so that the baseline is not
the code under test.  Reported: W and G minus the parent's S (the sweep's own cost over a scored call), and W over the
parent's F (one scored pass against five plain runs).  No gate.  Prints one JSON line (writes --json, appends to --text).
Usage: tools/sweep_bench.py --parent-lib /path/to/parent/libpfq.so [--rounds 1] [--steps 3] [--commits "parent child"]
The workers bind the handful of calls they need with ctypes themselves, so that the parent's library needs none of this
commit's symbols."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_G, GLEN, RL, B = 1024, 50000, 150, 8388608
K, NBITS, H = 21, 71887936, 10
FAMILY, DIVERGENCE = 8, 0.001
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
GENOME_SEED, READ_SEED = 0x5EED0000, 0x5EED1234
WANT_HITS, WANT_SCORES, WANT_SWEEP = 1, 2, 1024
LIST = (0.3, 0.5, 0.7, 0.9, 1.0)


class Hits(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("offsets", C.POINTER(C.c_uint64)), ("leaves", C.POINTER(C.c_uint32))]


class Sweep(C.Structure):
    _fields_ = [("n_thresholds", C.c_uint32), ("thresholds", C.POINTER(C.c_float)), ("n_leaves", C.c_uint64), ("n_units", C.c_uint64),
                ("leaf_units", C.POINTER(C.c_uint64)), ("leaf_unique", C.POINTER(C.c_uint64)), ("units_hit", C.POINTER(C.c_uint64)),
                ("units_unique", C.POINTER(C.c_uint64)), ("entries", C.POINTER(C.c_uint64)), ("genomes_hit", C.POINTER(C.c_uint64))]


def worker(lib_path: str, who: str, steps: int, warmup: int) -> dict:
    vp = C.c_void_p
    L, hip = C.CDLL(lib_path), C.CDLL("libamdhip64.so")
    L.pfq_last_error.restype = C.c_char_p
    L.pfq_synth_genomes_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    L.pfq_synth_reads_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    L.pfq_tree_build_balanced_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64, C.c_uint64, C.c_uint32,
                                                 C.c_uint64, C.c_uint64, C.c_float, C.c_uint32, C.c_int, C.POINTER(vp)]
    L.pfq_query_batch_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_float, C.c_uint32, vp, C.POINTER(Hits)]
    L.pfq_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.pfq_tree_close.argtypes = [vp]
    L.pfq_tree_close.restype = None
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    hip.hipFree.argtypes = [vp]
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc} {L.pfq_last_error().decode(errors='replace') if what.startswith('pfq') else ''}")

    def malloc(n):
        p = vp()
        ok(hip.hipMalloc(C.byref(p), n), "hipMalloc")
        return p

    genomes = malloc(N_G * GLEN)
    ok(L.pfq_synth_genomes_device(genomes, N_G, GLEN, GENOME_SEED, None), "pfq_synth_genomes_device")
    ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
    # every genome = its family's first genome with substitutions of its own (a fixed seed: every worker alike)
    host = np.empty((N_G, GLEN), dtype=np.uint8)
    ok(hip.hipMemcpy(host.ctypes.data, genomes, host.nbytes, 2), "hipMemcpy")
    rng = np.random.default_rng(12345)
    base = host[(np.arange(N_G) // FAMILY) * FAMILY]
    mut = rng.random((N_G, GLEN), dtype=np.float32) < DIVERGENCE
    alt = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (N_G, GLEN), dtype=np.uint8)]
    host = np.ascontiguousarray(np.where(mut, alt, base))
    ok(hip.hipMemcpy(genomes, host.ctypes.data, host.nbytes, 1), "hipMemcpy")
    del host, base, mut, alt
    ids = (C.c_char_p * N_G)(*[f"G{i:05d}".encode() for i in range(N_G)])
    tree = vp()
    ok(L.pfq_tree_build_balanced_device(genomes, GLEN, N_G, ids, K, NBITS, H, SEEDS[0], SEEDS[1], 0.001, 5000000, 0, C.byref(tree)),
       "pfq_tree_build_balanced_device")
    reads = malloc(B * RL + 64)
    ok(L.pfq_synth_reads_device(reads, 0, B, RL, genomes, GLEN, N_G, READ_SEED, None), "pfq_synth_reads_device")
    ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
    ok(hip.hipFree(genomes), "hipFree")
    off_h = np.arange(B + 1, dtype=np.uint64) * RL
    off = malloc(off_h.nbytes)
    ok(hip.hipMemcpy(off, off_h.ctypes.data, off_h.nbytes, 1), "hipMemcpy")
    stream, e0, e1 = vp(), vp(), vp()
    ok(hip.hipStreamCreateWithFlags(C.byref(stream), 1), "hipStreamCreateWithFlags")
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    child = who == "child"
    if child:
        L.pfq_tree_set_sweep.argtypes = [vp, C.POINTER(C.c_float), C.c_uint32]
        L.pfq_sweep_get.argtypes = [vp, C.POINTER(Sweep)]
        L.pfq_sweep_reset.argtypes = [vp]
        ok(L.pfq_tree_set_sweep(tree, (C.c_float * len(LIST))(*LIST), len(LIST)), "pfq_tree_set_sweep")
    hits = Hits()
    scored = WANT_HITS | WANT_SCORES
    variants = {"S": [(LIST[0], scored)], "F": [(t, 0) for t in LIST]}
    if child:
        variants.update(W=[(LIST[0], scored | WANT_SWEEP)], G=[(LIST[0], scored | WANT_SWEEP)])
    out = {}
    for name, calls in variants.items():
        if child:
            ok(L.pfq_set_option(tree, b"PFQ_SWEEP_LDS", b"0" if name == "G" else None), "pfq_set_option")
        ms = []
        for i in range(warmup + steps):
            ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
            for thr, flags in calls:
                ok(L.pfq_query_batch_device(tree, reads, off, B, B * RL, thr, flags, stream, C.byref(hits) if flags else None), "pfq_query_batch_device")
            ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            t = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(t), e0, e1), "hipEventElapsedTime")
            if i >= warmup:
                ms.append(round(t.value, 4))
        out[name] = ms
    if child:  # what the last flagged call counted
        ok(L.pfq_sweep_reset(tree), "pfq_sweep_reset")
        ok(L.pfq_query_batch_device(tree, reads, off, B, B * RL, LIST[0], scored | WANT_SWEEP, stream, C.byref(hits)), "pfq_query_batch_device")
        sw = Sweep()
        ok(L.pfq_sweep_get(tree, C.byref(sw)), "pfq_sweep_get")
        n = int(sw.n_thresholds)
        out["sweep"] = {"n_units": int(sw.n_units), **{k: [int(getattr(sw, k)[t]) for t in range(n)] for k in ("units_hit", "units_unique", "entries")}}
    L.pfq_tree_close(tree)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--commits", default="")
    ap.add_argument("--json")
    ap.add_argument("--text")
    ap.add_argument("--worker", choices=["parent", "child"])
    ap.add_argument("--lib")
    ap.add_argument("--worker-timeout", type=int, default=240)
    args = ap.parse_args()
    child_lib = os.path.join(ROOT, "phagefilter_amd", "libpfq.so")
    if args.worker:
        print(json.dumps(worker(args.lib or (child_lib if args.worker == "child" else args.parent_lib), args.worker, args.steps, args.warmup)))
        return
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("--parent-lib: a libpfq.so built from the parent commit is needed (the baseline is never this commit's own build)")
    runs = {"parent": {}, "child": {}, "again": {}}
    counted = {}
    for rnd in range(args.rounds):  # a worker that fails ends the run: nothing more is started on the device
        for role, who, lib in (("parent", "parent", args.parent_lib), ("child", "child", child_lib), ("again", "parent", args.parent_lib)):
            cmd = ["timeout", "-k", "10", str(args.worker_timeout), sys.executable, os.path.abspath(__file__), "--worker", who, "--lib", lib,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit(f"{role} worker of round {rnd} ended with status {p.returncode}:\n{p.stderr[-2000:]}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            counted = res.pop("sweep", counted)
            for key, ms in res.items():
                runs[role].setdefault(key, []).extend(ms)
            print(f"round {rnd} {role} done", file=sys.stderr, flush=True)

    def summary(ms):
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "repeats": ms}

    out = {"workload": f"{B} reads x {RL} bp per call, base theta {LIST[0]}, list {list(LIST)}, balanced {N_G}-leaf SBT (families of {FAMILY}, "
                       f"{DIVERGENCE} substitutions per base apart), k={K}, nbits={NBITS}, {H} hashes; device-resident calls, HIP events",
           "commits": args.commits, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup}
    tables = {role: {k: summary(v) for k, v in runs[role].items()} for role in runs}
    par, chi = tables["parent"], tables["child"]
    reported = {"W minus parent S, ms (the sweep's own cost, pass in LDS)": round(chi["W"]["median_ms"] - par["S"]["median_ms"], 3),
                "G minus parent S, ms (pass with global atomics)": round(chi["G"]["median_ms"] - par["S"]["median_ms"], 3),
                "W minus child S, ms": round(chi["W"]["median_ms"] - chi["S"]["median_ms"], 3),
                "W over parent S": round(chi["W"]["median_ms"] / par["S"]["median_ms"], 4),
                "W over parent F (one scored pass with the sweep against five plain runs)": round(chi["W"]["median_ms"] / par["F"]["median_ms"], 4),
                "counted by one call": counted}
    out.update(tables, reported=reported)
    lines = [f"# tools/sweep_bench.py: {out['workload']}", f"# commits (parent child): {args.commits}",
             f"# parent, child and parent-again processes alternated, {args.rounds} rounds x {args.steps} timed repeats per variant; ms: median [min .. max]"]
    for who, table in tables.items():
        for k, v in table.items():
            lines.append(f"  {who:6s} {k:2s} {v['median_ms']:9.3f} [{v['min_ms']:9.3f} .. {v['max_ms']:9.3f}]")
    lines += [f"  reported {k}: {v}" for k, v in reported.items()]
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if args.text:
        with open(args.text, "a") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
