"""The texts the deflate tests share (tests/test_deflate_cpu.py, tests/test_gpu_deflate.py), the stand-alone host program
tools/deflate_host.cpp as their reference, and the cutting rule of include/pfq.h restated."""
import os
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READS = os.path.join(ROOT, "tests", "golden", "examples", "reads")
GOLDEN = [os.path.join(READS, "sim_reads_c10000_n5_e0.0.fq"), os.path.join(READS, "sim_reads_c10000_n5_e0.01.fq")]
MEMBER = 65280
HEADER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])
FAR = 32768


def synthetic_fastq(records=700, seed=20):
    """Illumina-style: 100 .. 150 bases, qualities that start high and decay in runs."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(records):
        n = int(rng.integers(100, 151))
        seq = "".join("ACGT"[b] for b in rng.integers(0, 4, n))
        q, qual = 38.0, []
        while len(qual) < n:
            run = int(rng.integers(1, 12))
            qual += [chr(33 + max(2, min(40, int(q))))] * run
            q += float(rng.normal(-0.6, 3.0))
            q = min(q, 40.0)
        out.append(f"@SYN.{i} lane{i % 8}:{int(rng.integers(1, 3000))}:{int(rng.integers(1, 99999))}\n{seq}\n+\n{''.join(qual[:n])}\n")
    return "".join(out).encode()


def far_text():
    """'abcdefgh' recurs at distance exactly 32768 (a match is allowed) and 'ijklmnop' at 32769 (it must not be used): one member.
    The filler is one byte, so no other 4-gram comes between a gram and its return in the hash table."""
    t = bytearray(b"A" * 33200)
    for at, gram in ((0, b"abcdefgh"), (FAR, b"abcdefgh"), (100, b"ijklmnop"), (100 + FAR + 1, b"ijklmnop")):
        t[at:at + 8] = gram
    return bytes(t)


def de_bruijn(k, n):
    """Every word of n letters out of k exactly once, as one cyclic sequence of k ** n letters (the Lyndon words' concatenation)."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


def fibonacci_text(rare=13, seed=21):
    """Bytes 0 .. rare - 1 occur 1, 2, 3, 5, 8 .. 377 times (the end-of-block symbol is the other 1), strewn into 64000 bytes of 40
    other values in which no 3-gram repeats, so nothing matches and the literal counts are the byte counts: 1600 for each of the
    forty.  An unlimited Huffman code of these counts puts the rare symbols in a chain of 13 merges below a tree of 41 leaves: 19
    bits (tests/test_deflate_cpu.py counts the symbols of the member to be sure)."""
    fib = [1, 2]
    while len(fib) < rare:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(seed)
    filler = np.array(de_bruijn(40, 3), dtype=np.uint8) + 100
    rares = np.concatenate([np.full(c, i, dtype=np.uint8) for i, c in enumerate(fib)])
    rng.shuffle(rares)
    t = np.insert(filler, np.sort(rng.choice(len(filler), len(rares), replace=False)), rares)
    assert len(t) <= MEMBER
    return t.tobytes()


_ZOO = None


def zoo():
    """[(name, text, cuts)]; computed once and shared."""
    global _ZOO
    if _ZOO is None:
        rng = np.random.default_rng(22)
        z = [(f"byte_x{n}", b"Q" * n, ()) for n in (0, 1, 2, 3, 4, 257, 258, 259, MEMBER - 1, MEMBER, MEMBER + 1, 2 * MEMBER + 5)]
        z += [("period2", b"xy" * 2000, ()), ("period3", b"abc" * 23000, ()), ("period3_short", b"abc" * 2, ())]
        z.append(("all_bytes_once", bytes(range(256)), ()))
        z.append(("random_member", rng.integers(0, 256, MEMBER, dtype=np.uint8).tobytes(), ()))
        z.append(("far", far_text(), ()))
        z.append(("fibonacci", fibonacci_text(), ()))
        for path in GOLDEN:
            z.append((os.path.basename(path), open(path, "rb").read(), ()))
        syn = synthetic_fastq()
        z.append(("synthetic_fastq", syn, ()))
        z.append(("cuts", syn[:5000], (0, 0, 1, 2, 2, 3000, 5000, 5000)))
        z.append(("cuts_across_members", syn[:2 * MEMBER + 100], (MEMBER - 1, MEMBER, 2 * MEMBER + 50)))
        _ZOO = z
    return _ZOO


FASTQ_NAMES = [os.path.basename(p) for p in GOLDEN] + ["synthetic_fastq"]


def members_of(length, cuts):
    """The cutting rule: [(piece, text begin, text bytes)]."""
    bounds = [0] + list(cuts) + [length]
    out = []
    for piece in range(len(bounds) - 1):
        for at in range(bounds[piece], bounds[piece + 1], MEMBER):
            out.append((piece, at, min(MEMBER, bounds[piece + 1] - at)))
    return out


def build_host(exe, flags):
    subprocess.run(["g++", "-std=c++17"] + list(flags) + ["-I", os.path.join(ROOT, "phagefilter_amd", "csrc"),
                    os.path.join(ROOT, "tools", "deflate_host.cpp"), "-lz", "-o", exe], check=True)
    return exe


def run_host(exe, text, cuts, tmp, check=False):
    """The members the core makes of text: (gz, [(piece, text begin, text bytes, member bytes)])."""
    src, dst = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.gz")
    with open(src, "wb") as f:
        f.write(text)
    r = subprocess.run([exe] + (["--check"] if check else []) + [src, dst] + [str(c) for c in cuts], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])  # (a sanitizer report is on stderr and ends the program)
    lines = r.stdout.split("\n")[:-1]
    rows = [tuple(int(x) for x in line.split()[1:]) for line in lines[:-1]]
    gz = open(dst, "rb").read()
    assert lines[-1] == f"members {len(rows)} bytes {len(gz)}", lines[-1]
    return gz, rows


def check_members(gz, rows, text, cuts):
    """Every member is a BGZF member whose payload zlib inflates to its part of the text."""
    assert [r[:3] for r in rows] == members_of(len(text), cuts)
    at = 0
    for piece, begin, n, size in rows:
        m = gz[at:at + size]
        assert m[:16] == HEADER and struct.unpack("<H", m[16:18])[0] == size - 1, (begin, "header or BSIZE")
        assert size <= n + 31
        d = zlib.decompressobj(-15)
        part = text[begin:begin + n]
        assert d.decompress(m[18:-8]) == part and d.eof and not d.unused_data, (begin, "payload")
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(part), n), (begin, "CRC or ISIZE")
        at += size
    assert at == len(gz)


def zlib_total(text, level, strategy):
    """Bytes of the same members made by zlib."""
    total = 0
    for at in range(0, len(text), MEMBER):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += len(c.compress(text[at:at + MEMBER]) + c.flush()) + 26
    return total
