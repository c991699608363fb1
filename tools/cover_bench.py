#!/usr/bin/env python3
"""Cost of PFQ_WANT_COVERAGE against the PARENT commit's library, on the config-3 geometry of tools/lca_bench.py: balanced
1024-leaf SBT of 50 kbp genomes, nbits 71 887 936, 10 hashes, k 21; 8 388 608 reads of 150 bp per call, resident in HBM, half
of them from the genomes; pfq_query_batch_device on a stream, every call between two HIP events.  --family N (the workload
of PFQ_BENCH_FAMILY in bench.py): the genomes come in families of N, --divergence substitutions per base apart, so a positive
read lists up to N leaves; without it every positive read lists one.  --threshold 1.0 takes the kernel that probes nothing,
0.7 the probing one.

The yardstick is a libpfq.so built from the parent commit (--parent-lib), never this commit's own variants.  The workers run
in processes of their own, alternated (parent, child, parent again, ...), each timing its variants `--steps` times after
`--warmup` calls:
    parent:  P0 flags 0, P1 PFQ_WANT_HITS          (the second parent process of a round is the A/A role "again")
    child:   the same two; (c) PFQ_WANT_HITS | PFQ_WANT_COVERAGE into a sketch that earlier calls have filled (the steady
             state of a run); (c0) the same into an empty one (pfq_coverage_reset before every call, outside the timed span:
             the span includes the allocation and every register's first rise)
Gates, on the flag-off paths only: the child's P0 and P1 medians within the parent's own spread (max - min of its repeats)
plus the A/A difference (|median of parent - median of again|) measured in the same run.  Reported only: (c) and (c0) over
the parent's P1, the cost of the sketch.  Prints one JSON line (writes --json, appends to --text) and ends with status 1 when
a gate fails.
Usage: tools/cover_bench.py --parent-lib /path/to/parent/libpfq.so [--family 8] [--threshold 0.7] [--rounds 2] [--steps 3]
--only child --flags 129 runs one child worker alone with the given flags (for a profiler: rocprofv3 ... -- python
tools/cover_bench.py --only child --flags 129 ...).
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
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
GENOME_SEED, READ_SEED = 0x5EED0000, 0x5EED1234
WANT_HITS, WANT_COVERAGE = 1, 128
PARENT_VARIANTS = {"P0": 0, "P1": WANT_HITS}
CHILD_VARIANTS = dict(PARENT_VARIANTS, c=WANT_HITS | WANT_COVERAGE, c0=WANT_HITS | WANT_COVERAGE)


class Hits(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("offsets", C.POINTER(C.c_uint64)), ("leaves", C.POINTER(C.c_uint32))]


class Coverage(C.Structure):
    _fields_ = [("n_leaves", C.c_uint64), ("n_units", C.c_uint64), ("precision", C.c_uint32), ("registers", C.POINTER(C.c_uint8)),
                ("units", C.POINTER(C.c_uint64)), ("matched", C.POINTER(C.c_uint64)), ("filter_bits", C.POINTER(C.c_uint64)),
                ("distinct", C.POINTER(C.c_double)), ("genome_kmers", C.POINTER(C.c_double))]


def worker(lib_path: str, who: str, thr: float, steps: int, warmup: int, family: int, divergence: float, only_flags: int) -> dict:
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
    if family > 1:  # every genome = its family's first genome with substitutions of its own (a fixed seed: every worker alike)
        host = np.empty((N_G, GLEN), dtype=np.uint8)
        ok(hip.hipMemcpy(host.ctypes.data, genomes, host.nbytes, 2), "hipMemcpy")
        rng = np.random.default_rng(12345)
        base = host[(np.arange(N_G) // family) * family]
        mut = rng.random((N_G, GLEN), dtype=np.float32) < divergence
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
        L.pfq_coverage_reset.argtypes = [vp]
        L.pfq_coverage_get.argtypes = [vp, C.POINTER(Coverage)]
    hits = Hits()
    out = {}
    variants = CHILD_VARIANTS if child else PARENT_VARIANTS
    if only_flags >= 0:
        variants = {"only": only_flags}
    for name, flags in variants.items():
        ms = []
        for i in range(warmup + steps):
            if name == "c0":
                ok(L.pfq_coverage_reset(tree), "pfq_coverage_reset")
            ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
            ok(L.pfq_query_batch_device(tree, reads, off, B, B * RL, thr, flags, stream, C.byref(hits) if flags else None), "pfq_query_batch_device")
            ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            t = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(t), e0, e1), "hipEventElapsedTime")
            if i >= warmup:
                ms.append(round(t.value, 4))
        out[name] = ms
    if child and only_flags < 0:  # what one call sketched (the last c0 call)
        cv = Coverage()
        ok(L.pfq_coverage_get(tree, C.byref(cv)), "pfq_coverage_get")
        n = int(cv.n_leaves)
        units, matched = np.ctypeslib.as_array(cv.units, shape=(n,)), np.ctypeslib.as_array(cv.matched, shape=(n,))
        distinct = np.ctypeslib.as_array(cv.distinct, shape=(n,))
        out["sketch"] = {"n_units": int(cv.n_units), "precision": int(cv.precision), "listed (unit, leaf) pairs": int(units.sum()),
                         "matched k-mers": int(matched.sum()), "distinct k-mers, sum of the estimates": round(float(distinct.sum()), 1),
                         "bytes": (n << int(cv.precision)) + 16 * n}
    L.pfq_tree_close(tree)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--family", type=int, default=0)
    ap.add_argument("--divergence", type=float, default=0.001)
    ap.add_argument("--threshold", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json")
    ap.add_argument("--text")
    ap.add_argument("--worker", choices=["parent", "child"])
    ap.add_argument("--only", choices=["parent", "child"])
    ap.add_argument("--flags", type=int, default=-1)
    ap.add_argument("--lib")
    ap.add_argument("--worker-timeout", type=int, default=240)
    args = ap.parse_args()
    child_lib = os.path.join(ROOT, "phagefilter_amd", "libpfq.so")
    if args.worker or args.only:
        who = args.worker or args.only
        lib = args.lib or (child_lib if who == "child" else args.parent_lib)
        print(json.dumps(worker(lib, who, args.threshold, args.steps, args.warmup, args.family, args.divergence, args.flags)))
        return
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("--parent-lib: a libpfq.so built from the parent commit is needed (the yardstick is never this commit's own build)")
    runs = {"parent": {}, "child": {}, "again": {}}
    sketch = {}
    for rnd in range(args.rounds):  # a worker that fails ends the run: nothing more is started on the device
        for role, who, lib in (("parent", "parent", args.parent_lib), ("child", "child", child_lib), ("again", "parent", args.parent_lib)):
            cmd = ["timeout", "-k", "10", str(args.worker_timeout), sys.executable, os.path.abspath(__file__), "--worker", who, "--lib", lib,
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--threshold", str(args.threshold), "--family", str(args.family),
                   "--divergence", str(args.divergence)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit(f"{role} worker of round {rnd} ended with status {p.returncode}:\n{p.stderr[-2000:]}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            sketch = res.pop("sketch", sketch)
            for key, ms in res.items():
                runs[role].setdefault(key, []).extend(ms)
            print(f"round {rnd} {role} done", file=sys.stderr, flush=True)

    def summary(ms):
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "repeats": ms}

    fam = f"families of {args.family}, {args.divergence} substitutions per base apart" if args.family > 1 else "unrelated genomes"
    out = {"workload": f"{B} reads x {RL} bp per call, theta {args.threshold}, balanced {N_G}-leaf SBT ({fam}), k={K}, nbits={NBITS}, {H} hashes; "
                       f"device-resident calls, HIP events", "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup}
    par = {k: summary(runs["parent"][k]) for k in PARENT_VARIANTS}
    aga = {k: summary(runs["again"][k]) for k in PARENT_VARIANTS}
    chi = {k: summary(runs["child"][k]) for k in CHILD_VARIANTS}
    spread = {k: round(v["max_ms"] - v["min_ms"], 3) for k, v in par.items()}
    aa = {k: round(abs(par[k]["median_ms"] - aga[k]["median_ms"]), 3) for k in PARENT_VARIANTS}
    margin = {k: round(spread[k] + aa[k], 3) for k in PARENT_VARIANTS}
    gates = {f"child {k} within parent {k} + spread + A/A": chi[k]["median_ms"] <= par[k]["median_ms"] + margin[k] for k in PARENT_VARIANTS}
    reported = {"(c) over parent P1": round(chi["c"]["median_ms"] / par["P1"]["median_ms"], 4),
                "(c) minus parent P1, ms": round(chi["c"]["median_ms"] - par["P1"]["median_ms"], 3),
                "(c0) over parent P1": round(chi["c0"]["median_ms"] / par["P1"]["median_ms"], 4),
                "(c0) minus parent P1, ms": round(chi["c0"]["median_ms"] - par["P1"]["median_ms"], 3),
                "sketch of one call": sketch}
    out.update(parent=par, again=aga, child=chi, spread_ms=spread, aa_ms=aa, margin_ms=margin, gates=gates, reported=reported,
               gates_ok=all(gates.values()))
    lines = [f"# tools/cover_bench.py: {out['workload']}", f"# parent, child and parent-again processes alternated, {args.rounds} rounds x {args.steps} "
             f"timed repeats per variant; ms: median [min .. max]; margin = spread of the parent variant's repeats + A/A difference"]
    for who, table in (("parent", par), ("again", aga), ("child", chi)):
        for k, v in table.items():
            lines.append(f"  {who:6s} {k:4s} {v['median_ms']:9.3f} [{v['min_ms']:9.3f} .. {v['max_ms']:9.3f}]" +
                         (f"  spread {spread[k]:.3f} A/A {aa[k]:.3f} margin {margin[k]:.3f}" if who == "parent" else ""))
    lines += [f"  gate {'ok  ' if v else 'FAIL'} {k}" for k, v in gates.items()] + [f"  reported {k}: {v}" for k, v in reported.items()]
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if args.text:
        with open(args.text, "a") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))
    if not out["gates_ok"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
