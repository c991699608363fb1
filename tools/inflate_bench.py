#!/usr/bin/env python3
"""Device times of pfq_text_inflate between HIP events (pfq_debug_last_inflate) on the text block of tools/format_bench.py:
--reads (1 048 576) synthetic FASTQ records of 150 bases (343 MB of text), written as blocked gzip at --level (6) in members
of 65 280 text bytes, resident in page-locked host memory.

Per run, the median of --steps calls after --warmup:
    the copy of the compressed bytes and the kernel (device ms), the kernel's rate in GB/s of text out and as a share of --stream-gbs,
    the chip's streaming rate (reading the compressed bytes and writing the text: what a kernel that did nothing else would move);
    the whole call by the host clock;
    pfq_text_parse_inflated (the device-to-device assembly of the text and the parse) against pfq_text_parse of the same text from
    host memory, by the host clock;
    zlib inflating the same members on the host, given their boundaries, with 1 and with --threads (16) threads.
The inflated text is compared with the original once.  Appends to --text.

With --cli N: whole processes instead.  N (8 000 000) such reads as one blocked gzip file (page-cached: written just before the
runs), a 64-leaf database of the benchmark's shape, counts only, --threads threads, --repeats (3) alternations of
`query --device-parse` (the streaming host reader: the path without the option) and `query --device-parse --device-inflate`; the
two must leave the same CLASSIFICATION.csv.
Usage: tools/inflate_bench.py [--reads 1048576] [--level 6] [--steps 5] [--warmup 1] [--threads 16] [--text profiles/inflate_bench.txt]
       tools/inflate_bench.py --cli 8000000 [--repeats 3] [--threads 16] [--workdir /tmp/pfq_inflate_bench]"""
import argparse
import ctypes as C
import os
import shutil
import statistics
import subprocess
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from phagefilter_amd import _ffi  # noqa: E402
from format_bench import GENOME_LEN, K, make_text  # noqa: E402
from sim_bench import build  # noqa: E402

BLOCK = 65280


def bgzf_member(text, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    pay = c.compress(text) + c.flush()
    size = 18 + len(pay) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + pay + struct.pack("<II", zlib.crc32(text), len(text)))


def cli_runs(args):
    import torch
    from cli_bench import CLI, write_fastq
    from phagefilter_amd import BloomTree
    L = _ffi.lib()
    shutil.rmtree(args.workdir, ignore_errors=True)
    os.makedirs(args.workdir)
    n_g, glen, nbits, h = 64, GENOME_LEN, 71887936, 10
    dg = torch.empty(n_g * glen, dtype=torch.uint8, device="cuda")
    _ffi.check(L.pfq_synth_genomes_device(dg.data_ptr(), n_g, glen, 0x5EED0000, None))
    torch.cuda.synchronize()
    gt = BloomTree.build_balanced_device(dg.data_ptr(), glen, n_g, [f"G{i:05d}" for i in range(n_g)], K, nbits, h, 0x0123456789ABCDEF, 0xFEDCBA9876543210)
    db = os.path.join(args.workdir, "db")
    os.makedirs(db)
    gt.save(db)
    gt.close()
    fq, gz = os.path.join(args.workdir, "piece.fq"), os.path.join(args.workdir, "reads.fq.gz")
    t0, n_text, n_members = time.time(), 0, 0
    with open(gz, "wb") as out, ThreadPoolExecutor(args.threads) as pool:
        for first in range(0, args.cli, 2_000_000):
            n = min(2_000_000, args.cli - first)
            dr = torch.empty(n * 150, dtype=torch.uint8, device="cuda")
            _ffi.check(L.pfq_synth_reads_device(dr.data_ptr(), first, n, 150, dg.data_ptr(), glen, n_g, 0x5EED1234, None))
            torch.cuda.synchronize()
            write_fastq(fq, dr.cpu().numpy().reshape(n, 150), first)
            view = memoryview(open(fq, "rb").read())
            os.remove(fq)
            for m in pool.map(lambda a: bgzf_member(view[a:a + BLOCK], args.level), range(0, len(view), BLOCK)):
                out.write(m)
                n_members += 1
            n_text += len(view)
        out.write(bgzf_member(b"", args.level))
    del dg
    torch.cuda.empty_cache()
    lines = [f"inflate_bench --cli: {args.cli} reads of 150 bases, {n_text} bytes of FASTQ text as one blocked gzip file of {os.path.getsize(gz)} bytes "
             f"({n_members} members and the end marker, level {args.level}; written in {time.time() - t0:.1f} s, page-cached); 64 leaves, k {K}, threshold 1, "
             f"counts only, -t {args.threads}; the runs alternate"]
    csvs = set()
    for rep_i in range(args.repeats):
        for label, extra in (("query --device-parse", ("--device-parse",)), ("query --device-parse --device-inflate", ("--device-parse", "--device-inflate"))):
            o = os.path.join(args.workdir, "out")
            shutil.rmtree(o, ignore_errors=True)
            t0 = time.time()
            p = subprocess.run([CLI, "query", "-r", gz, "-o", o, "-d", db, "-t", str(args.threads), "-f", "1.0", *extra], capture_output=True, text=True,
                               env=dict(os.environ, PFQ_INGEST_TIMING="1"))
            wall = time.time() - t0
            assert p.returncode == 0, p.stderr
            csvs.add(open(os.path.join(o, "CLASSIFICATION.csv"), "rb").read())
            pick = lambda head: next((l for l in p.stderr.splitlines() if l.startswith(head)), "")
            lines.append(f"  {label:40s} whole process {wall:.3f} s = {args.cli / wall / 1e6:.2f} M reads/s; {pick('query loop')}")
            for head in ("device parse:", "device inflate:", "cpu:"):
                if pick(head):
                    lines.append(f"      {pick(head)}")
    assert len(csvs) == 1, "the runs left different CLASSIFICATION.csv"
    lines.append("  every run left the same CLASSIFICATION.csv")
    shutil.rmtree(args.workdir, ignore_errors=True)
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cli", type=int, default=0, help="whole processes on a blocked gzip file of this many reads instead of the kernel's rates")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/pfq_inflate_bench")
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--stream-gbs", type=float, default=6290.0, help="the chip's measured streaming rate (a 16-byte copy kernel) the kernel's is set against")
    ap.add_argument("--text", default=os.path.join(ROOT, "profiles", "inflate_bench.txt"))
    args = ap.parse_args()
    if args.cli:
        report = cli_runs(args)
        sys.stdout.write(report)
        os.makedirs(os.path.dirname(os.path.abspath(args.text)), exist_ok=True)
        with open(args.text, "a") as f:
            f.write(report)
        return
    import torch
    tree = build(16, GENOME_LEN, K, 1 << 20, 4)
    text_t, n_text = make_text(16, args.reads)
    text = text_t.numpy()
    view = memoryview(text)
    with ThreadPoolExecutor(args.threads) as pool:
        members = list(pool.map(lambda a: bgzf_member(view[a:a + BLOCK], args.level), range(0, n_text, BLOCK)))
    members.append(bgzf_member(b"", args.level))
    n_gz = sum(map(len, members))
    gz_t = torch.empty(n_gz, dtype=torch.uint8).pin_memory()
    gz_t.numpy()[:] = memoryview(b"".join(members))
    L = _ffi.lib()
    rows = []
    for it in range(args.warmup + args.steps):
        inf, parsed, parsed_host = _ffi.TextInflated(), _ffi.Text(), _ffi.Text()
        t0 = time.time()
        _ffi.check(L.pfq_text_inflate(tree._h, gz_t.data_ptr(), n_gz, 0, _ffi.TEXT_FINAL, C.byref(inf)))
        t1 = time.time()
        assert inf.n_good == len(members) and inf.good_text == n_text, (inf.n_good, inf.good_text)
        _ffi.check(L.pfq_text_parse_inflated(tree._h, None, 0, (1 << 64) - 1, _ffi.TEXT_FASTQ, _ffi.TEXT_FINAL, C.byref(parsed)))
        t2 = time.time()
        assert parsed.n_records == args.reads
        if it == 0:
            assert tree.read_text(0, n_text) == text.tobytes(), "the inflated text differs from the original"
        t3 = time.time()
        _ffi.check(L.pfq_text_parse(tree._h, text_t.data_ptr(), n_text, (1 << 64) - 1, _ffi.TEXT_FASTQ, _ffi.TEXT_FINAL, C.byref(parsed_host)))
        t4 = time.time()
        if it >= args.warmup:
            rows.append(tree.last_inflate_ms() + ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t4 - t3) * 1e3))
    med = [statistics.median(r[i] for r in rows) for i in range(5)]
    lo = [min(r[i] for r in rows) for i in range(5)]

    def host_inflate(m):
        return len(zlib.decompress(m[18:-8], -15))
    host = {}
    for threads in (1, args.threads):
        best = None
        for _ in range(2):
            t0 = time.time()
            with ThreadPoolExecutor(threads) as pool:
                assert sum(pool.map(host_inflate, members, chunksize=64)) == n_text
            dt = time.time() - t0
            best = dt if best is None else min(best, dt)
        host[threads] = best
    kernel_gbs = n_text / (med[1] * 1e-3) / 1e9
    moved = (n_text + n_gz) / (med[1] * 1e-3) / 1e9
    lines = [
        f"inflate_bench: {args.reads} reads of 150 bases as FASTQ text ({n_text} bytes) as blocked gzip at level {args.level}: {len(members)} members, "
        f"{n_gz} bytes ({n_text / n_gz:.2f} : 1); median (min) of {args.steps} after {args.warmup}",
        f"  device: copy {med[0]:.3f} ({lo[0]:.3f}) ms = {n_gz / (med[0] * 1e-3) / 1e9:.1f} GB/s of compressed bytes; k_gz_inflate {med[1]:.3f} ({lo[1]:.3f}) ms = "
        f"{kernel_gbs:.2f} GB/s of text out, {args.reads / (med[1] * 1e-3) / 1e6:.1f} M reads/s; bytes read and written {moved:.2f} GB/s = "
        f"{100 * moved / args.stream_gbs:.2f} % of a streaming rate of {args.stream_gbs:.0f} GB/s",
        f"  host clock: pfq_text_inflate {med[2]:.1f} ({lo[2]:.1f}) ms; pfq_text_parse_inflated {med[3]:.1f} ({lo[3]:.1f}) ms against pfq_text_parse of the same "
        f"text from page-locked host memory {med[4]:.1f} ({lo[4]:.1f}) ms",
        f"  zlib on the host, given the boundaries (python threads, zlib releases the lock): 1 thread {host[1] * 1e3:.0f} ms = {n_text / host[1] / 1e9:.2f} GB/s; "
        f"{args.threads} threads {host[args.threads] * 1e3:.0f} ms = {n_text / host[args.threads] / 1e9:.2f} GB/s (best of 2)",
    ]
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    os.makedirs(os.path.dirname(os.path.abspath(args.text)), exist_ok=True)
    with open(args.text, "a") as f:
        f.write(report)
    tree.close()


if __name__ == "__main__":
    main()
