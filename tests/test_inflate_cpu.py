"""Blocked gzip without a device: pfq_gz_scan against its restatement (tests/bgzf_ref.py), the inflate core under the address
and undefined-behaviour sanitizers through the stand-alone program tools/inflate_host.cpp (the text the device kernel compiles:
phagefilter_amd/csrc/pfq_inflate_core.h), and `phage_filter bgzf`."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_ref as B
from phagefilter_amd import PfqError, _ffi, gz_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
STOPS = {B.END: "end", B.LIMIT: "limit", B.MORE: "more", B.FOREIGN: "foreign"}


def same_scan(gz, max_text=0, final=True):
    begin, text_begin, stop = B.scan(gz, max_text, final)
    got = gz_scan(gz, max_text, final)
    where = (len(gz), max_text, final)
    assert got["stop"] == STOPS[stop], where
    assert got["begin"].tolist() == begin and got["text_begin"].tolist() == text_begin, where
    assert (got["n_members"], got["consumed"], got["text_bytes"]) == (len(begin) - 1, begin[-1], text_begin[-1]), where
    return got


# ---- (a) the scan

def test_scan_ordinary_members():
    data = B.fastq_like(200000, 5)
    for block in (B.BLOCK, 997, 1):
        gz = B.write(data[:200000 if block > 1 else 300], block)
        got = same_scan(gz)
        assert got["stop"] == "end" and got["consumed"] == len(gz) and got["text_bytes"] == (200000 if block > 1 else 300)
        assert gzip.decompress(gz) == data[:got["text_bytes"]]
    assert same_scan(b"")["n_members"] == 0
    assert same_scan(B.EOF_MARKER)["n_members"] == 1                    # the end marker is an ordinary member


def test_scan_optional_header_parts():
    t = B.fastq_like(3000, 6)
    variants = [dict(before=[(b"XY", b"abc")]), dict(after=[(b"ZZ", b"")]), dict(before=[(b"AB", b"\0" * 40)], after=[(b"BD", b"12"), (b"CB", b"xy")]),
                dict(fname=b"reads.fq"), dict(fcomment=b"note"), dict(fhcrc=True), dict(fname=b"", fcomment=b"", fhcrc=True, before=[(b"BC", b"123")])]
    gz = b"".join(B.member(t, **v) for v in variants)
    got = same_scan(gz)
    assert got["n_members"] == len(variants) and got["stop"] == "end"
    assert gzip.decompress(gz) == t * len(variants)
    # not such members: no BC subfield, BC of another length only, a subfield that overruns XLEN, reserved flag bits, FNAME that
    # never ends, no payload byte, no FEXTRA
    ok = B.member(t)
    no_bc = ok[:12] + b"XC" + ok[14:]
    assert same_scan(ok + no_bc + ok)["n_members"] == 1
    overrun = ok[:14] + struct.pack("<H", 3) + ok[16:]
    assert same_scan(overrun + ok)["stop"] == "foreign"
    reserved = ok[:3] + bytes([ok[3] | 0x20]) + ok[4:]
    assert same_scan(ok + reserved)["n_members"] == 1
    endless = B.frame(b"\x03\x00", 0, 0)
    endless = endless[:3] + bytes([endless[3] | 8]) + endless[4:]       # FNAME flagged, and the only zero bytes lie in the trailer or beyond
    same_scan(endless + ok)
    no_payload = B.frame(b"", 0, 0)
    assert same_scan(no_payload + ok)["stop"] == "foreign"
    assert same_scan(gzip.compress(t))["stop"] == "foreign"
    assert same_scan(gzip.compress(t))["n_members"] == 0


def test_scan_three_members_cut_at_every_byte():
    t = B.fastq_like(900, 8)
    gz = B.member(t[:400], fname=b"a") + B.member(t[400:], before=[(b"XY", b"abc")], fhcrc=True) + B.member(b"")
    for cut in range(len(gz) + 1):
        for final in (True, False):
            same_scan(gz[:cut], 0, final)
    assert gz_scan(gz[:-1], final=False)["stop"] == "more" and gz_scan(gz[:-1], final=True)["stop"] == "foreign"


def test_scan_large_member_and_limits():
    text = B.four_letter(70000, 9)
    pay = B.deflate(text, 6)
    m70k = B.frame(pay, len(text), zlib.crc32(text))
    ok = B.member(text[:65536])
    got = same_scan(ok + m70k + ok)
    assert (got["n_members"], got["stop"]) == (1, "foreign")           # 70 000 bytes of text: not such a member
    gz = B.write(B.fastq_like(5 * B.BLOCK, 10))
    for max_text in (0, 65536, 65537, 2 * B.BLOCK - 1, 2 * B.BLOCK, 2 * B.BLOCK + 1, 5 * B.BLOCK, 1 << 40):
        same_scan(gz, max_text)
    assert gz_scan(gz, 2 * B.BLOCK)["n_members"] == 2 and gz_scan(gz, 2 * B.BLOCK)["stop"] == "limit"
    assert gz_scan(gz, 65536)["n_members"] == 1
    assert gz_scan(gz, 5 * B.BLOCK)["stop"] == "end"                    # (the empty end marker still fits)
    for bad in (1, 65535):
        with pytest.raises(PfqError) as e:
            gz_scan(gz, bad)
        assert e.value.code == -1
    out = _ffi.GzMembers()
    L = _ffi.lib()
    assert L.pfq_gz_scan(None, 5, 0, 0, C.byref(out)) == -1
    assert L.pfq_gz_scan(None, 0, 0, 2, C.byref(out)) == -1
    assert L.pfq_gz_scan(None, 0, 0, 0, None) == -1
    assert L.pfq_gz_scan(None, 0, 0, 1, C.byref(out)) == 0 and out.n_members == 0 and out.stop == _ffi.GZ_END


def test_scan_foreign_bytes_after_and_between_members():
    t = B.fastq_like(2000, 12)
    a, b = B.member(t[:1000]), B.member(t[1000:])
    junk = b"not gzip at all, and long enough to hold a header\n"
    for final in (True, False):
        assert same_scan(a + b + junk, 0, final)["stop"] == "foreign"
        assert same_scan(a + b + junk, 0, final)["n_members"] == 2
        assert same_scan(a + junk + b, 0, final)["n_members"] == 1
        assert same_scan(a + gzip.compress(t) + b, 0, final)["n_members"] == 1
        # magic bytes inside the junk are never searched for
        assert same_scan(a + b"xx" + b, 0, final)["n_members"] == 1
    assert same_scan(a + junk[:5], 0, False)["stop"] == "more"         # fewer bytes than a header: undecided until more arrive
    assert same_scan(a + junk[:5], 0, True)["stop"] == "foreign"


# ---- (b) the core under sanitizers

@pytest.fixture(scope="module")
def inflate_host(tmp_path_factory):
    """tools/inflate_host.cpp built with -fsanitize=address,undefined: a program of its own, run directly."""
    exe = str(tmp_path_factory.mktemp("inflate_host") / "inflate_host")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "phagefilter_amd", "csrc"), os.path.join(ROOT, "tools", "inflate_host.cpp"), "-o", exe], check=True)

    def run(members, tmp):
        src, dst = os.path.join(tmp, "in.gz"), os.path.join(tmp, "out.txt")
        with open(src, "wb") as f:
            f.write(b"".join(members))
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])   # (a sanitizer report is on stderr and ends the program)
        lines = r.stdout.split("\n")[:-1]
        assert lines[-1] == f"stop taken {sum(map(len, members))}", lines[-1]
        rows = [line.split() for line in lines[:-1]]
        assert len(rows) == len(members)
        texts, at, out = open(dst, "rb").read(), 0, []
        for row in rows:
            status, crc, isize, max_dist, max_len = int(row[1]), int(row[2], 16), int(row[3]), int(row[5]), int(row[6])
            text = None
            if status == 0:
                text, at = texts[at:at + isize], at + isize
            out.append((status, crc, text, max_dist, max_len))
        assert at == len(texts)
        return out
    return run


def test_core_zoo(inflate_host, tmp_path):
    zoo = B.zoo()
    for name, text, m in zoo:
        assert gzip.decompress(m) == text, name                         # the writer's members are gzip
    got = inflate_host([m for _, _, m in zoo], str(tmp_path))
    for (name, text, _), (status, crc, out, _, _) in zip(zoo, got):
        assert status == 0 and out == text and crc == zlib.crc32(text), name
    by_name = {name: g for (name, _, _), g in zip(zoo, got)}
    assert by_name["distance_32768"][3:] == (32768, 258)                # the largest distance and length deflate has
    assert by_name["rle_equal"][3:] == (1, 258)
    assert by_name["huffman_only_equal"][3:] == (0, 0) and by_name["random_stored"][3:] == (0, 0)


def test_core_corrupt_list(inflate_host, tmp_path):
    cor = B.corrupt_list()
    assert len(cor) > 2000
    got = inflate_host([m for _, _, m in cor], str(tmp_path))
    accepted = 0
    for (name, text, m), (status, crc, out, _, _) in zip(cor, got):
        if status == 0:                                                 # not rejected and equal to the trailer: then it is the text
            assert out == text, name
            accepted += 1
        if B.zlib_says(m) is None:
            assert status != 0, name
    # the only changes that leave a member valid: the five padding bits of the stored member's first block header
    assert accepted == 5 and all(got[i][0] == 0 for i, (name, _, _) in enumerate(cor) if name in {f"stored_flip{b}" for b in range(3, 8)})
    statuses = {name: g[0] for (name, _, _), g in zip(cor, got)}
    for kind in ("dynamic", "fixed", "stored"):
        assert statuses[f"{kind}_crc"] == 3 and statuses[f"{kind}_isize_minus"] == 2 and statuses[f"{kind}_isize_plus"] == 2, kind


# ---- (c) phage_filter bgzf

@pytest.mark.parametrize("source", ["plain", "gzip", "empty"])
def test_bgzf_command(tmp_path, source):
    data = b"" if source == "empty" else B.fastq_like(3 * B.BLOCK + 1234, 13)
    src, dst = str(tmp_path / ("in.fq.gz" if source == "gzip" else "in.fq")), str(tmp_path / "out.fq.gz")
    with open(src, "wb") as f:
        f.write(gzip.compress(data) if source == "gzip" else data)
    for level in (None, 0, 9):
        r = subprocess.run([CLI, "bgzf", "-i", src, "-o", dst] + ([] if level is None else ["--level", str(level)]), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        gz = open(dst, "rb").read()
        assert gzip.decompress(gz) == data
        got = same_scan(gz)
        assert got["stop"] == "end" and got["consumed"] == len(gz) and got["text_bytes"] == len(data)
        sizes = np.diff(got["text_begin"]).tolist()
        assert max(sizes) <= B.BLOCK and sizes[:-1] == [B.BLOCK] * (len(data) // B.BLOCK) + ([len(data) % B.BLOCK] if len(data) % B.BLOCK else [])
        assert gz.endswith(B.EOF_MARKER) and sizes[-1] == 0
    assert subprocess.run([CLI, "bgzf", "-i", src, "-o", dst, "--level", "10"], capture_output=True).returncode != 0
