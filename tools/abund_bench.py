#!/usr/bin/env python3
"""Cost of PFQ_WANT_ABUNDANCE against the PARENT commit's library, on the config-3 geometry of tools/lca_bench.py: balanced
1024-leaf SBT of 50 kbp genomes, nbits 71 887 936, 10 hashes, k 21; 8 388 608 reads of 150 bp per call, resident in HBM, half
of them from the genomes; pfq_query_batch_device on a stream, every call between two HIP events.  --family N (the workload
of PFQ_BENCH_FAMILY in bench.py): the genomes come in families of N, --divergence substitutions per base apart, so a positive
read passes up to N leaves and its row is ambiguous; without it every positive read hits one leaf and the log stays empty.

The yardstick is a libpfq.so built from the parent commit (--parent-lib), never this commit's own variants.  Parent and child
run in processes of their own, alternated (parent, child, parent, child, ...), each timing its variants `--steps` times after
`--warmup` calls:
    parent:  P0 flags 0, P1 PFQ_WANT_HITS
    child:   the same two, (a) PFQ_WANT_HITS | PFQ_WANT_ABUNDANCE into an empty log (pfq_abundance_reset before every call,
             outside the timed span: the span includes the log's first allocation)
The margin of a comparison is the spread (max - min) of the parent variant's own repeats.  Gates: the child's P0 and P1 within
the margin of the parent's (the feature costs nothing when it is off).  Reported only: (a) over the parent's P1 — the cost of
the append; one EM iteration over the log of one call (wall time of pfq_abundance_estimate with tol 0 over its iterations, one
host wait each), the log's bytes over that time next to the streaming rate HBM reads reach on this part, and the same with
PFQ_ABUND_LDS=0, and the default path at PFQ_ABUND_BLOCKS = 256 / 1024 / 2048 / 4096.  Prints one JSON line (writes --json,
appends to --text) and ends with status 1 when a gate fails.
Usage: tools/abund_bench.py --parent-lib /path/to/parent/libpfq.so [--family 8] [--rounds 2] [--steps 3] [--warmup 1]
The workers bind the handful of calls they need with ctypes themselves, so that the parent's library needs none of this
commit's symbols."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_G, GLEN, RL, B = 1024, 50000, 150, 8388608
K, NBITS, H = 21, 71887936, 10
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
GENOME_SEED, READ_SEED = 0x5EED0000, 0x5EED1234
WANT_HITS, WANT_ABUNDANCE = 1, 64
PARENT_VARIANTS = {"P0": 0, "P1": WANT_HITS}
CHILD_VARIANTS = dict(PARENT_VARIANTS, a=WANT_HITS | WANT_ABUNDANCE)
EM_BLOCKS = (256, 1024, 2048, 4096)
HBM_READ_TBS = 6.3  # what streaming reads reach on an MI355X (8 TB/s on paper)


class Hits(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("offsets", C.POINTER(C.c_uint64)), ("leaves", C.POINTER(C.c_uint32))]


class Abundance(C.Structure):
    _fields_ = [("n_leaves", C.c_uint64), ("mass", C.POINTER(C.c_uint64)), ("unique", C.POINTER(C.c_uint64)),
                ("n_units", C.c_uint64), ("n_unhit", C.c_uint64), ("n_unique", C.c_uint64), ("n_ambiguous", C.c_uint64),
                ("n_all_leaves", C.c_uint64), ("n_entries", C.c_uint64), ("last_delta", C.c_uint64),
                ("iterations", C.c_uint32), ("converged", C.c_uint32)]


def worker(lib_path: str, who: str, thr: float, steps: int, warmup: int, family: int, divergence: float, em_iters: int) -> dict:
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
        L.pfq_abundance_reset.argtypes = [vp]
        L.pfq_abundance_estimate.argtypes = [vp, C.c_uint32, C.c_uint64, C.POINTER(Abundance)]
    hits = Hits()
    out = {}
    for name, flags in (CHILD_VARIANTS if child else PARENT_VARIANTS).items():
        ms = []
        for i in range(warmup + steps):
            if flags & WANT_ABUNDANCE:
                ok(L.pfq_abundance_reset(tree), "pfq_abundance_reset")
            ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
            ok(L.pfq_query_batch_device(tree, reads, off, B, B * RL, thr, flags, stream, C.byref(hits) if flags else None), "pfq_query_batch_device")
            ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            t = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(t), e0, e1), "hipEventElapsedTime")
            if i >= warmup:
                ms.append(round(t.value, 4))
        out[name] = ms
    if child:  # the log holds the last call's rows: the EM over it, with and without the LDS histogram
        ab = Abundance()
        for key, lds in (("em_lds", None), ("em_global", b"0")):
            ok(L.pfq_set_option(tree, b"PFQ_ABUND_LDS", lds), "pfq_set_option")
            per_iter = []
            for i in range(1 + steps):
                t0 = time.perf_counter()
                ok(L.pfq_abundance_estimate(tree, em_iters, 0, C.byref(ab)), "pfq_abundance_estimate")
                if i >= 1:
                    per_iter.append(round((time.perf_counter() - t0) * 1e3 / max(1, ab.iterations), 4))
            out[key] = per_iter
        ok(L.pfq_set_option(tree, b"PFQ_ABUND_LDS", None), "pfq_set_option")
        for blocks in EM_BLOCKS:  # the default path at other grids (reported only)
            ok(L.pfq_set_option(tree, b"PFQ_ABUND_BLOCKS", str(blocks).encode()), "pfq_set_option")
            per_iter = []
            for i in range(1 + steps):
                t0 = time.perf_counter()
                ok(L.pfq_abundance_estimate(tree, em_iters, 0, C.byref(ab)), "pfq_abundance_estimate")
                if i >= 1:
                    per_iter.append(round((time.perf_counter() - t0) * 1e3 / max(1, ab.iterations), 4))
            out[f"em_blocks_{blocks}"] = per_iter
        ok(L.pfq_set_option(tree, b"PFQ_ABUND_BLOCKS", None), "pfq_set_option")
        out["log"] = {"n_units": ab.n_units, "n_unhit": ab.n_unhit, "n_unique": ab.n_unique, "n_ambiguous": ab.n_ambiguous,
                      "n_all_leaves": ab.n_all_leaves, "n_entries": ab.n_entries, "iterations": ab.iterations,
                      "bytes": int(ab.n_ambiguous) * 12 + int(ab.n_entries) * 4}
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
    ap.add_argument("--em-iters", type=int, default=20)
    ap.add_argument("--json")
    ap.add_argument("--text")
    ap.add_argument("--worker", choices=["parent", "child"])
    ap.add_argument("--lib")
    ap.add_argument("--worker-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(worker(args.lib, args.worker, args.threshold, args.steps, args.warmup, args.family, args.divergence, args.em_iters)))
        return
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("--parent-lib: a libpfq.so built from the parent commit is needed (the yardstick is never this commit's own build)")
    child_lib = os.path.join(ROOT, "phagefilter_amd", "libpfq.so")
    runs = {"parent": {}, "child": {}}
    log = {}
    for rnd in range(args.rounds):  # a worker that fails ends the run: nothing more is started on the device
        for who, lib in (("parent", args.parent_lib), ("child", child_lib)):
            cmd = ["timeout", "-k", "10", str(args.worker_timeout), sys.executable, os.path.abspath(__file__), "--worker", who, "--lib", lib,
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--threshold", str(args.threshold), "--family", str(args.family),
                   "--divergence", str(args.divergence), "--em-iters", str(args.em_iters)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit(f"{who} worker of round {rnd} ended with status {p.returncode}:\n{p.stderr[-2000:]}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            log = res.pop("log", log)
            for key, ms in res.items():
                runs[who].setdefault(key, []).extend(ms)
            print(f"round {rnd} {who} done", file=sys.stderr, flush=True)

    def summary(ms):
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "repeats": ms}

    fam = f"families of {args.family}, {args.divergence} substitutions per base apart" if args.family > 1 else "unrelated genomes"
    out = {"workload": f"{B} reads x {RL} bp per call, theta {args.threshold}, balanced {N_G}-leaf SBT ({fam}), k={K}, nbits={NBITS}, {H} hashes; "
                       f"device-resident calls, HIP events", "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup}
    par = {k: summary(runs["parent"][k]) for k in PARENT_VARIANTS}
    chi = {k: summary(runs["child"][k]) for k in list(CHILD_VARIANTS) + ["em_lds", "em_global"] + [f"em_blocks_{b}" for b in EM_BLOCKS]}
    margin = {k: round(v["max_ms"] - v["min_ms"], 3) for k, v in par.items()}
    gates = {f"child {k} within the margin of parent {k}": chi[k]["median_ms"] <= par[k]["median_ms"] + margin[k] for k in PARENT_VARIANTS}

    def rate(ms):
        return round(log["bytes"] / (ms * 1e-3) / 1e12, 3) if ms > 0 and log.get("bytes") else 0.0

    reported = {"(a) over parent P1": round(chi["a"]["median_ms"] / par["P1"]["median_ms"], 4),
                "(a) minus parent P1, ms": round(chi["a"]["median_ms"] - par["P1"]["median_ms"], 3),
                "log of one call": log,
                "EM iteration, LDS histogram (default), ms": chi["em_lds"]["median_ms"],
                "EM iteration, LDS histogram, log TB/s": rate(chi["em_lds"]["median_ms"]),
                "EM iteration, PFQ_ABUND_LDS=0, ms": chi["em_global"]["median_ms"],
                "EM iteration, PFQ_ABUND_LDS=0, log TB/s": rate(chi["em_global"]["median_ms"]),
                "EM iteration at PFQ_ABUND_BLOCKS = " + " / ".join(str(b) for b in EM_BLOCKS) + ", ms":
                    " / ".join(str(chi[f"em_blocks_{b}"]["median_ms"]) for b in EM_BLOCKS),
                "HBM streaming reads, TB/s": HBM_READ_TBS}
    out.update(parent=par, child=chi, margin_ms=margin, gates=gates, reported=reported, gates_ok=all(gates.values()))
    lines = [f"# tools/abund_bench.py: {out['workload']}", f"# parent and child processes alternated, {args.rounds} rounds x {args.steps} "
             f"timed repeats per variant; ms: median [min .. max]; margin = spread of the parent variant's repeats"]
    for who, table in (("parent", par), ("child", chi)):
        for k, v in table.items():
            lines.append(f"  {who:6s} {k:14s} {v['median_ms']:9.3f} [{v['min_ms']:9.3f} .. {v['max_ms']:9.3f}]" + (f"  margin {margin[k]:.3f}" if who == "parent" else ""))
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
