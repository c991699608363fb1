#!/usr/bin/env python3
"""Device times of pfq_text_format's stages, between HIP events (pfq_debug_last_format, PFQ_FMT_TIME=1), on the benchmark's reads
as FASTQ text: --reads (1 048 576) synthetic reads of 150 bases drawn from the benchmark's tree (1024 leaves, k 21, nbits
71 887 936, 10 hashes), every other read replaced by random bases so that both streams fill, wrapped as four-line records with
unique ids and qualities of 150 bytes (339 bytes a record), resident in page-locked host memory.

Per run, the median of --steps rounds after --warmup; a round is pfq_text_parse, pfq_text_query(PFQ_WANT_HITS) at threshold 1
and pfq_text_format(first_index 0, --block, POS and NEG):
    ids + blocks, sizes + scans, emit (device ms) and the emit kernel's rate over the bytes it writes;
    the three calls by the host clock (pfq_text_format includes the copy of both streams to page-locked host memory).
Appends to --text.
Usage: tools/format_bench.py [--reads 1048576] [--block 1000] [--steps 3] [--warmup 1] [--leaves 1024] [--text profiles/format_bench.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from phagefilter_amd import _ffi  # noqa: E402
from sim_bench import build  # noqa: E402

K, NBITS, NUM_HASHES, GENOME_LEN, READ_LEN = 21, 71887936, 10, 50000, 150
GENOME_SEED, READ_SEED = 0x5EED0000, 0x5EED1234


def make_text(n_leaves, n_reads):
    """The benchmark's reads (pfq_synth_reads_device over the benchmark's genomes), every other one random, as FASTQ text in
    page-locked memory: (tensor that owns the memory, its bytes)."""
    import torch
    L = _ffi.lib()
    genomes = torch.empty(n_leaves * GENOME_LEN, dtype=torch.uint8, device="cuda")
    _ffi.check(L.pfq_synth_genomes_device(genomes.data_ptr(), n_leaves, GENOME_LEN, GENOME_SEED, None))
    reads = torch.empty(n_reads * READ_LEN + 64, dtype=torch.uint8, device="cuda")
    _ffi.check(L.pfq_synth_reads_device(reads.data_ptr(), 0, n_reads, READ_LEN, genomes.data_ptr(), GENOME_LEN, n_leaves, READ_SEED, None))
    torch.cuda.synchronize()
    bases = reads[:n_reads * READ_LEN].cpu().numpy().reshape(n_reads, READ_LEN).copy()
    del genomes, reads
    rng = np.random.default_rng(7)
    bases[0::2] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, bases[0::2].shape)]
    head = np.frombuffer(b"@r000000000 1:N:0:ACGT\n", dtype=np.uint8)
    rec = np.empty((n_reads, len(head) + READ_LEN + 3 + READ_LEN + 1), dtype=np.uint8)
    rec[:, :len(head)] = head
    idx = np.arange(n_reads, dtype=np.int64)
    for d in range(9):                                                 # the nine digits of the id
        rec[:, 10 - d] = 48 + (idx // 10 ** d) % 10
    o = len(head)
    rec[:, o:o + READ_LEN] = bases
    rec[:, o + READ_LEN:o + READ_LEN + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, o + READ_LEN + 3:-1] = ord("I")
    rec[:, -1] = 10
    text = torch.empty(rec.size, dtype=torch.uint8).pin_memory()
    text.numpy()[:] = rec.reshape(-1)
    return text, rec.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--block", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--leaves", type=int, default=1024)
    ap.add_argument("--text", default=os.path.join(ROOT, "profiles", "format_bench.txt"))
    args = ap.parse_args()
    tree = build(args.leaves, GENOME_LEN, K, NBITS, NUM_HASHES)
    text, n_bytes = make_text(args.leaves, args.reads)
    assert n_bytes < 1 << 31, "pfq_text_parse takes less than 2^31 bytes a call"
    L = _ffi.lib()
    tree.set_option("PFQ_FMT_TIME", "1")
    rows, out = [], None
    for it in range(args.warmup + args.steps):
        parsed, hits, out = _ffi.Text(), _ffi.Hits(), _ffi.TextRecords()
        t0 = time.time()
        _ffi.check(L.pfq_text_parse(tree._h, text.data_ptr(), n_bytes, (1 << 64) - 1, _ffi.TEXT_FASTQ, _ffi.TEXT_FINAL, C.byref(parsed)))
        t1 = time.time()
        _ffi.check(L.pfq_text_query(tree._h, 1.0, _ffi.WANT_HITS, C.byref(hits)))
        t2 = time.time()
        _ffi.check(L.pfq_text_format(tree._h, 0, args.block, _ffi.FMT_POS | _ffi.FMT_NEG, C.byref(out)))
        t3 = time.time()
        assert parsed.n_records == args.reads and out.n_left == (1 if args.reads % args.block else 0)
        if it >= args.warmup:
            rows.append(tree.last_format_ms() + ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    med = [statistics.median(r[i] for r in rows) for i in range(6)]
    written = int(out.pos_bytes) + int(out.neg_bytes)
    lines = [
        f"format_bench: {args.reads} reads of {READ_LEN} bases as FASTQ text ({n_bytes} bytes), {args.leaves} leaves, k {K}, threshold 1, "
        f"block {args.block}; median of {args.steps} after {args.warmup}",
        f"  POS {int(out.pos_records)} records, {int(out.pos_bytes)} bytes; NEG {int(out.neg_records)} records, {int(out.neg_bytes)} bytes; "
        f"{int(out.n_left)} runs left",
        f"  device: ids + blocks {med[0]:.3f} ms, sizes + scans {med[1]:.3f} ms, emit {med[2]:.3f} ms "
        f"({written / (med[2] * 1e-3) / 1e9:.0f} GB/s written, {args.reads / (sum(med[:3]) * 1e-3) / 1e6:.0f} M reads/s over the three stages)",
        f"  host clock: pfq_text_parse {med[3]:.1f} ms, pfq_text_query {med[4]:.1f} ms, pfq_text_format {med[5]:.1f} ms "
        f"(with the copy of {written} bytes to the host: {args.reads / (med[5] * 1e-3) / 1e6:.1f} M reads/s)",
    ]
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    os.makedirs(os.path.dirname(os.path.abspath(args.text)), exist_ok=True)
    with open(args.text, "a") as f:
        f.write(report)
    tree.close()


if __name__ == "__main__":
    main()
