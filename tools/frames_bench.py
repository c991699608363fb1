#!/usr/bin/env python3
"""Cost of pfq_query_frames on the bench's 1024-leaf geometry (balanced SBT of 50 kbp genomes, nbits 71 887 936, 10 hashes,
k 21): --seqs synthetic sequences of 20 kb, resident in HBM, every second one carrying a 5 kb insert from one of the genomes.
    (a)  pfq_query_frames_device at F = 1000, S = 500 and at S = F, in Mbases/s of input;
    (b)  what the library could do before: pfq_query_batch_device | PFQ_WANT_HITS on the same frames cut on the host into a
         CSR buffer at S = F, so the inner classification is the same work.
(a at S = F) - (b) is the cost of the cut, the segments, the sequence counts and the refinement.  --pieces: (a) at S = F for
every PFQ_FRAME_PIECE listed.  Every call lies between two HIP events on its stream; median of --steps after --warmup.
Prints one JSON line (writes --json, appends to --text).
--only frames|precut [--step S] [--piece P] runs that one variant alone, for a profiler:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/frames_bench.py --only frames --step 1000"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_G, GLEN, K, NBITS, H = 1024, 50000, 21, 71887936, 10
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
SEQ_LEN, INSERT, FRAME = 20000, 5000, 1000


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=4096)
    ap.add_argument("--threshold", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pieces", default="256,1024,4096,16384")
    ap.add_argument("--only", choices=["frames", "precut"])
    ap.add_argument("--step", type=int, default=FRAME)
    ap.add_argument("--piece", type=int, default=0)
    ap.add_argument("--json")
    ap.add_argument("--text")
    args = ap.parse_args()
    from phagefilter_amd import BloomTree, _ffi
    L, hip, vp = _ffi.lib(), C.CDLL("libamdhip64.so"), C.c_void_p
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    def to_device(a):
        p = vp()
        ok(hip.hipMalloc(C.byref(p), a.nbytes + 64), "hipMalloc")
        ok(hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1), "hipMemcpy")
        return p

    d_gen = vp()
    ok(hip.hipMalloc(C.byref(d_gen), N_G * GLEN), "hipMalloc")
    _ffi.check(L.pfq_synth_genomes_device(d_gen, N_G, GLEN, 0x5EED0000, None))
    ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
    tree = BloomTree.build_balanced_device(d_gen.value, GLEN, N_G, [f"G{i:05d}" for i in range(N_G)], K, NBITS, H, *SEEDS)
    genomes = np.empty((N_G, GLEN), dtype=np.uint8)
    ok(hip.hipMemcpy(genomes.ctypes.data, d_gen, genomes.nbytes, 2), "hipMemcpy")
    rng = np.random.default_rng(2024)
    n = args.seqs
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, SEQ_LEN), dtype=np.uint8)]
    for i in range(0, n, 2):
        g, o, at = int(rng.integers(0, N_G)), int(rng.integers(0, GLEN - INSERT)), int(rng.integers(0, SEQ_LEN - INSERT))
        seqs[i, at:at + INSERT] = genomes[g, o:o + INSERT]
    d_seq, d_off = to_device(seqs), to_device(np.arange(n + 1, dtype=np.uint64) * SEQ_LEN)
    # the same frames cut on the host at S = F: sequence-major, frame after frame — the input itself, under other offsets
    n_pre = n * (SEQ_LEN // FRAME)
    d_pre_off = to_device(np.arange(n_pre + 1, dtype=np.uint64) * FRAME)
    stream, e0, e1 = vp(), vp(), vp()
    ok(hip.hipStreamCreateWithFlags(C.byref(stream), 1), "hipStreamCreateWithFlags")
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    found = {}

    def frames(step):
        offs, segs = tree.query_frames_device(d_seq.value, d_off.value, n, n * SEQ_LEN, FRAME, step, args.threshold, stream.value)
        found[step] = {"segments": int(offs[-1]), "frames": tree.last_n_frames, "matched k-mers": int(segs["matched"].sum())}

    def precut():
        offs, _ = tree.query_device_hits(d_seq.value, d_pre_off.value, n_pre, n * SEQ_LEN, args.threshold, stream.value)
        found["precut"] = {"hits": int(offs[-1]), "frames": n_pre}

    def timed(fn):
        ms = []
        for i in range(args.warmup + args.steps):
            ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
            fn()
            ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            t = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(t), e0, e1), "hipEventElapsedTime")
            if i >= args.warmup:
                ms.append(round(t.value, 3))
        med = statistics.median(ms)
        return {"median_ms": round(med, 3), "min_ms": min(ms), "max_ms": max(ms), "Mbases_per_s": round(n * SEQ_LEN / med / 1e3, 1)}

    if args.only:
        if args.piece:
            tree.set_option("PFQ_FRAME_PIECE", str(args.piece))
        print(json.dumps({args.only: timed(precut if args.only == "precut" else lambda: frames(args.step)), "found": found}))
        tree.close()
        return
    out = {"workload": f"{n} sequences x {SEQ_LEN} bases, every second one with a {INSERT}-base insert; theta {args.threshold}; balanced {N_G}-leaf "
                       f"SBT, k={K}, nbits={NBITS}, {H} hashes; F = {FRAME}; device-resident calls, HIP events, median of {args.steps}"}
    out["(b) precut frames, pfq_query_batch_device | PFQ_WANT_HITS"] = timed(precut)
    out["(a) frames S = F"] = timed(lambda: frames(FRAME))
    out["(a) frames S = 500"] = timed(lambda: frames(500))
    for piece in [int(p) for p in args.pieces.split(",") if p]:
        tree.set_option("PFQ_FRAME_PIECE", str(piece))
        out[f"(a) frames S = F, PFQ_FRAME_PIECE = {piece}"] = timed(lambda: frames(FRAME))
        out[f"(a) frames S = 500, PFQ_FRAME_PIECE = {piece}"] = timed(lambda: frames(500))
    tree.set_option("PFQ_FRAME_PIECE", None)
    out["post-stage ms, (a at S = F) - (b)"] = round(out["(a) frames S = F"]["median_ms"] - out["(b) precut frames, pfq_query_batch_device | PFQ_WANT_HITS"]["median_ms"], 3)
    out["found"] = {str(k): v for k, v in found.items()}
    tree.close()
    text = [f"# tools/frames_bench.py: {out['workload']}"] + [f"  {k}: {v}" for k, v in out.items() if k != "workload"]
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if args.text:
        with open(args.text, "a") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
