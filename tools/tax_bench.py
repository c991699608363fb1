#!/usr/bin/env python3
"""Cost of PFQ_WANT_TAXA against the PARENT commit's library, on the config-3 geometry of tools/lca_bench.py: balanced
1024-leaf SBT of 50 kbp genomes, nbits 71 887 936, 10 hashes, k 21; 8 388 608 reads of 150 bp per call, resident in HBM, half
of them from the genomes, about 1 % substitutions; pfq_query_batch_device on a stream, every call between two HIP events.

The yardstick is a libpfq.so built from the parent commit (--parent-lib), never this commit's own variants.  Parent and child
run in processes of their own, alternated (parent, child, parent, child, ...), each timing its variants `--steps` times after
`--warmup` calls at every threshold:
    parent:  P0 flags 0, P1 PFQ_WANT_HITS
    child:   the same two, (a) P1 | PFQ_WANT_TAXA on a six-level random taxonomy, (b) the same flags on the worst case for
             contention: one depth-1 taxon holding every genome under the root
The margin of every comparison is the spread (max - min) of the parent variant's own repeats.  Gates: the child's P0 and P1
within the margin of the parent's (the option must cost nothing when it is off).  Reported only: (a) and (b) minus the
parent's P1, ms per call.  The k_tax_* kernel times come from one `rocprofv3 --kernel-trace --stats` run of the child worker on
its own (`rocprofv3 --kernel-trace --stats -- python tools/tax_bench.py --worker child --lib phagefilter_amd/libpfq.so`).
Prints one JSON line (and writes --json / --text).
Usage: tools/tax_bench.py --parent-lib /path/to/parent/libpfq.so [--rounds 2] [--steps 5] [--warmup 2] [--thresholds 1.0,0.7]
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
WANT_HITS, WANT_TAXA = 1, 256
NO_CLADE = 0xFFFFFFFF
PARENT_VARIANTS = {"P0": 0, "P1": WANT_HITS}
CHILD_VARIANTS = dict(PARENT_VARIANTS, a=WANT_HITS | WANT_TAXA, b=WANT_HITS | WANT_TAXA)
TAXONOMY_OF = {"a": "random6", "b": "one_taxon"}


def taxonomy(kind: str):
    """(taxon_parent, leaf_taxon) over N_G leaves.  random6: 300 taxa, six levels, 40 % of the genomes in one taxon (phage
    taxonomies are top-heavy), the others anywhere; one_taxon: the root and one taxon that holds every genome."""
    if kind == "one_taxon":
        return np.array([NO_CLADE, 0], dtype=np.uint32), np.ones(N_G, dtype=np.uint32)
    rng = np.random.default_rng(6)
    parent, depth = [NO_CLADE], [0]
    while len(parent) < 300:
        p = int(rng.integers(0, len(parent)))
        if depth[p] < 6:
            parent.append(p)
            depth.append(depth[p] + 1)
    heavy = int(rng.integers(1, len(parent)))
    leaf = np.where(rng.random(N_G) < 0.4, heavy, rng.integers(0, len(parent), N_G))
    return np.array(parent, dtype=np.uint32), leaf.astype(np.uint32)


class Hits(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("offsets", C.POINTER(C.c_uint64)), ("leaves", C.POINTER(C.c_uint32))]


def worker(lib_path: str, variants: dict, thresholds, steps: int, warmup: int, errors: float) -> dict:
    vp = C.c_void_p
    L, hip = C.CDLL(lib_path), C.CDLL("libamdhip64.so")
    L.pfq_last_error.restype = C.c_char_p
    L.pfq_synth_genomes_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    L.pfq_synth_reads_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    L.pfq_tree_build_balanced_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64, C.c_uint64, C.c_uint32,
                                                 C.c_uint64, C.c_uint64, C.c_float, C.c_uint32, C.c_int, C.POINTER(vp)]
    L.pfq_query_batch_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_float, C.c_uint32, vp, C.POINTER(Hits)]
    L.pfq_tree_close.argtypes = [vp]
    L.pfq_tree_close.restype = None
    if any(v in TAXONOMY_OF for v in variants):
        L.pfq_tree_set_taxonomy.argtypes = [vp, C.c_uint64, vp, C.POINTER(C.c_char_p), vp]
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    hip.hipFree.argtypes = [vp]
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
    hip.hipStreamSynchronize.argtypes = [vp]
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
    ids = (C.c_char_p * N_G)(*[f"G{i:05d}".encode() for i in range(N_G)])
    tree = vp()
    ok(L.pfq_tree_build_balanced_device(genomes, GLEN, N_G, ids, K, NBITS, H, SEEDS[0], SEEDS[1], 0.001, 5000000, 0, C.byref(tree)),
       "pfq_tree_build_balanced_device")
    reads = malloc(B * RL + 64)
    ok(L.pfq_synth_reads_device(reads, 0, B, RL, genomes, GLEN, N_G, READ_SEED, None), "pfq_synth_reads_device")
    ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
    if errors > 0:  # substitutions at B * RL * errors random places (a fixed seed: every worker sees the same reads)
        host = np.empty(B * RL, dtype=np.uint8)
        ok(hip.hipMemcpy(host.ctypes.data, reads, host.nbytes, 2), "hipMemcpy")
        rng = np.random.default_rng(777)
        n_mut = int(B * RL * errors)
        host[rng.integers(0, host.size, n_mut)] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n_mut)]
        ok(hip.hipMemcpy(reads, host.ctypes.data, host.nbytes, 1), "hipMemcpy")
        del host
    ok(hip.hipFree(genomes), "hipFree")
    off_h = np.arange(B + 1, dtype=np.uint64) * RL
    off = malloc(off_h.nbytes)
    ok(hip.hipMemcpy(off, off_h.ctypes.data, off_h.nbytes, 1), "hipMemcpy")
    stream, e0, e1 = vp(), vp(), vp()
    ok(hip.hipStreamCreateWithFlags(C.byref(stream), 1), "hipStreamCreateWithFlags")
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    hits = Hits()
    out = {}
    for thr in thresholds:
        for name, flags in variants.items():
            if name in TAXONOMY_OF:
                par, leaf = taxonomy(TAXONOMY_OF[name])
                names = (C.c_char_p * len(par))(*[f"t{i}".encode() for i in range(len(par))])
                ok(L.pfq_tree_set_taxonomy(tree, len(par), par.ctypes.data, names, leaf.ctypes.data), "pfq_tree_set_taxonomy")
            ms = []
            for i in range(warmup + steps):
                ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
                ok(L.pfq_query_batch_device(tree, reads, off, B, B * RL, thr, flags, stream, C.byref(hits)), "pfq_query_batch_device")
                ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
                ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
                t = C.c_float()
                ok(hip.hipEventElapsedTime(C.byref(t), e0, e1), "hipEventElapsedTime")
                if i >= warmup:
                    ms.append(round(t.value, 4))
            out[f"{thr}/{name}"] = ms
    L.pfq_tree_close(tree)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--thresholds", default="1.0,0.7")
    ap.add_argument("--errors", type=float, default=0.01)
    ap.add_argument("--json")
    ap.add_argument("--text")
    ap.add_argument("--worker", choices=["parent", "child"])
    ap.add_argument("--lib")
    ap.add_argument("--worker-timeout", type=int, default=240)
    args = ap.parse_args()
    thresholds = [float(x) for x in args.thresholds.split(",")]
    if args.worker:
        variants = PARENT_VARIANTS if args.worker == "parent" else CHILD_VARIANTS
        print(json.dumps(worker(args.lib, variants, thresholds, args.steps, args.warmup, args.errors)))
        return
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("--parent-lib: a libpfq.so built from the parent commit is needed (the yardstick is never this commit's own build)")
    child_lib = os.path.join(ROOT, "phagefilter_amd", "libpfq.so")
    runs = {"parent": {}, "child": {}}
    for rnd in range(args.rounds):  # a worker that fails ends the run: nothing more is started on the device
        for who, lib in (("parent", args.parent_lib), ("child", child_lib)):
            cmd = ["timeout", "-k", "10", str(args.worker_timeout), sys.executable, os.path.abspath(__file__), "--worker", who, "--lib", lib,
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--thresholds", args.thresholds, "--errors", str(args.errors)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit(f"{who} worker of round {rnd} ended with status {p.returncode}:\n{p.stderr[-2000:]}")
            for key, ms in json.loads(p.stdout.strip().splitlines()[-1]).items():
                runs[who].setdefault(key, []).extend(ms)
            print(f"round {rnd} {who} done", file=sys.stderr, flush=True)

    def summary(ms):
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "repeats": ms}

    out = {"workload": f"{B} reads x {RL} bp per call ({args.errors:.0%} substitutions), balanced {N_G}-leaf SBT, k={K}, nbits={NBITS}, "
                       f"{H} hashes; device-resident calls, HIP events", "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup,
           "thresholds": {}}
    lines = [f"# tools/tax_bench.py: {out['workload']}", f"# parent and child processes alternated, {args.rounds} rounds x {args.steps} "
             f"timed repeats per variant; ms per call: median [min .. max]; margin = spread of the parent variant's repeats"]
    all_ok = True
    for thr in thresholds:
        par = {k: summary(runs["parent"][f"{thr}/{k}"]) for k in PARENT_VARIANTS}
        chi = {k: summary(runs["child"][f"{thr}/{k}"]) for k in CHILD_VARIANTS}
        margin = {k: round(v["max_ms"] - v["min_ms"], 3) for k, v in par.items()}
        gates = {}
        for k in PARENT_VARIANTS:  # nothing existing moved
            gates[f"child {k} within the margin of parent {k}"] = chi[k]["median_ms"] <= par[k]["median_ms"] + margin[k]
        reported = {"(a) six-level random taxonomy minus parent P1, ms": round(chi["a"]["median_ms"] - par["P1"]["median_ms"], 3),
                    "(b) one taxon holding every genome minus parent P1, ms": round(chi["b"]["median_ms"] - par["P1"]["median_ms"], 3)}
        all_ok = all_ok and all(gates.values())
        out["thresholds"][str(thr)] = {"parent": par, "child": chi, "margin_ms": margin, "gates": gates, "reported": reported}
        lines.append(f"theta {thr}")
        for who, table in (("parent", par), ("child", chi)):
            for k, v in table.items():
                lines.append(f"  {who:6s} {k:3s} {v['median_ms']:9.3f} [{v['min_ms']:9.3f} .. {v['max_ms']:9.3f}]" +
                             (f"  margin {margin[k]:.3f}" if who == "parent" else ""))
        lines += [f"  gate {'ok  ' if v else 'FAIL'} {k}" for k, v in gates.items()] + [f"  reported {k}: {v}" for k, v in reported.items()]
    out["gates_ok"] = all_ok
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if args.text:
        with open(args.text, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
