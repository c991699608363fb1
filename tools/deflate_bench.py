#!/usr/bin/env python3
"""Device times of pfq_bgzf_deflate between HIP events (pfq_debug_last_deflate) on the POS + NEG bytes pfq_text_format makes of
tools/format_bench.py's block (--reads 1 048 576 reads of 150 bases as FASTQ, both streams, about 333 MB), against zlib level 1 on
the same members on one and on --threads host threads in the same session (Python's zlib releases the interpreter lock, so a
thread pool is that many cores of zlib).

Reports the medians of --steps calls after --warmup: copy in, deflate kernel, scan + gather + copy out (device ms), GB/s of text
through the kernel and through the whole call, the compressed sizes and the ratio of the rates.  Appends to --text.
Usage: tools/deflate_bench.py [--reads 1048576] [--block 1000] [--steps 5] [--warmup 1] [--threads 16] [--text profiles/deflate_bench.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from phagefilter_amd import _ffi  # noqa: E402
from format_bench import GENOME_LEN, K, NBITS, NUM_HASHES, make_text  # noqa: E402
from sim_bench import build  # noqa: E402

MEMBER = 65280


def zlib_member(part):
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
    return len(c.compress(part)) + len(c.flush()) + 26


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--block", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--leaves", type=int, default=1024)
    ap.add_argument("--text", default=os.path.join(ROOT, "profiles", "deflate_bench.txt"))
    args = ap.parse_args()
    tree = build(args.leaves, GENOME_LEN, K, NBITS, NUM_HASHES)
    text, n_bytes = make_text(args.leaves, args.reads)
    L = _ffi.lib()
    parsed, hits, out = _ffi.Text(), _ffi.Hits(), _ffi.TextRecords()
    _ffi.check(L.pfq_text_parse(tree._h, text.data_ptr(), n_bytes, (1 << 64) - 1, _ffi.TEXT_FASTQ, _ffi.TEXT_FINAL, C.byref(parsed)))
    _ffi.check(L.pfq_text_query(tree._h, 1.0, _ffi.WANT_HITS, C.byref(hits)))
    _ffi.check(L.pfq_text_format(tree._h, 0, args.block, _ffi.FMT_POS | _ffi.FMT_NEG, C.byref(out)))
    import torch
    data = torch.empty(int(out.pos_bytes) + int(out.neg_bytes), dtype=torch.uint8).pin_memory()
    C.memmove(data.data_ptr(), out.pos, int(out.pos_bytes))
    C.memmove(data.data_ptr() + int(out.pos_bytes), out.neg, int(out.neg_bytes))
    n = data.numel()
    rows, gz = [], _ffi.Bgzf()
    for it in range(args.warmup + args.steps):
        t0 = time.time()
        _ffi.check(L.pfq_bgzf_deflate(tree._h, data.data_ptr(), n, None, 0, C.byref(gz)))
        t1 = time.time()
        if it >= args.warmup:
            rows.append(tree.last_deflate_ms() + ((t1 - t0) * 1e3,))
    med = [statistics.median(r[i] for r in rows) for i in range(4)]
    ours = int(gz.gz_bytes)
    view = memoryview(data.numpy())
    parts = [view[at:at + MEMBER] for at in range(0, n, MEMBER)]
    t0 = time.time()
    z1 = sum(zlib_member(p) for p in parts)
    one = time.time() - t0
    with ThreadPoolExecutor(args.threads) as pool:
        t0 = time.time()
        zn = sum(pool.map(zlib_member, parts, chunksize=16))
        many = time.time() - t0
    assert z1 == zn
    kernel = n / (med[1] * 1e-3) / 1e9
    lines = [
        f"deflate_bench: {n} bytes of POS + NEG FASTQ ({args.reads} reads, block {args.block}) in {int(gz.n_members)} members; median of {args.steps} after {args.warmup}",
        f"  device: copy in {med[0]:.3f} ms, deflate kernel {med[1]:.3f} ms, scan + gather + copy out {med[2]:.3f} ms; the kernel takes {kernel:.2f} GB/s of text, "
        f"the call by the host clock {med[3]:.1f} ms = {n / (med[3] * 1e-3) / 1e9:.2f} GB/s",
        f"  size: device {ours} bytes ({ours / n:.4f} of the text), zlib level 1 {z1} bytes ({z1 / n:.4f}); device / zlib = {ours / z1:.3f}",
        f"  zlib level 1 on the same members: 1 thread {one:.2f} s = {n / one / 1e9:.3f} GB/s; {args.threads} threads {many:.2f} s = {n / many / 1e9:.3f} GB/s; "
        f"kernel / {args.threads} threads = {kernel / (n / many / 1e9):.2f}, whole call / {args.threads} threads = {(n / (med[3] * 1e-3)) / (n / many):.2f}",
    ]
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    os.makedirs(os.path.dirname(os.path.abspath(args.text)), exist_ok=True)
    with open(args.text, "a") as f:
        f.write(report)
    tree.close()


if __name__ == "__main__":
    main()
