"""The deflate core (phagefilter_amd/csrc/pfq_deflate_core.h, the text the device kernel compiles) without a device, through the
stand-alone program tools/deflate_host.cpp under the address and undefined-behaviour sanitizers: every member of a zoo of texts
must be a BGZF member that zlib and the project's own inflater take, the bytes must be a pure function of the text, and the
FASTQ inputs must come out smaller than each zlib coder that has only a part of what the core has."""
import heapq
import os
import subprocess
import zlib

import pytest

import deflate_zoo as Z
from phagefilter_amd import gz_scan

ROOT = Z.ROOT


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tools/deflate_host.cpp with -fsanitize=address,undefined: a program of its own, run directly."""
    exe = str(tmp_path_factory.mktemp("deflate_host") / "deflate_host")
    return Z.build_host(exe, ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


@pytest.fixture(scope="module")
def made(host, tmp_path_factory):
    """name -> (gz, rows, text, cuts): every zoo text through the sanitized program, with its own --check."""
    tmp = str(tmp_path_factory.mktemp("deflate_zoo"))
    return {name: Z.run_host(host, text, cuts, tmp, check=True) + (text, cuts) for name, text, cuts in Z.zoo()}


def canonical(lens):
    """(length, code as it is read, first bit first) -> symbol."""
    code, table = 0, {}
    for length in range(1, 16):
        for s, l in enumerate(lens):
            if l == length:
                table[(length, code)] = s
                code += 1
        code <<= 1
    return table


def read_block(payload, symbols=False):
    """(literal lengths, distance lengths[, literal/length symbol counts]) of the dynamic block a payload begins with, or None
    for another block type."""
    bits = int.from_bytes(payload, "little")
    at = 0

    def take(n):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += n
        return v

    def symbol(table):
        c = 0
        for length in range(1, 16):
            c = c << 1 | take(1)
            if (length, c) in table:
                return table[(length, c)]
        raise AssertionError("no such code")

    assert take(1) == 1                                                  # one block a member
    if take(2) != 2:
        return None
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    cl = [0] * 19
    for i in range(hclen):
        cl[order[i]] = take(3)
    assert max(cl) <= 7 and sum(2.0 ** -l for l in cl if l) == 1.0
    table = canonical(cl)
    lens = []
    while len(lens) < hlit + hdist:
        s = symbol(table)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        else:
            lens += [0] * (3 + take(3) if s == 17 else 11 + take(7))
    assert len(lens) == hlit + hdist
    if not symbols:
        return lens[:hlit], lens[hlit:]
    lit, dist, counts = canonical(lens[:hlit]), canonical(lens[hlit:]), [0] * 286
    while True:
        s = symbol(lit)
        counts[s] += 1
        if s == 256:
            return lens[:hlit], lens[hlit:], counts
        if s > 256:
            take(0 if s < 265 or s == 285 else (s - 261) >> 2)
            d = symbol(dist)
            take(0 if d < 4 else (d >> 1) - 1)


def tree_lengths(payload):
    return read_block(payload)


def test_zoo_members_are_bgzf(made):
    for name, (gz, rows, text, cuts) in made.items():
        try:
            Z.check_members(gz, rows, text, cuts)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")
        got = gz_scan(gz)
        assert (got["stop"], got["consumed"], got["text_bytes"], got["n_members"]) == ("end", len(gz), len(text), len(rows)), name
    assert made["byte_x0"][0] == b"" and len(made[f"byte_x{2 * Z.MEMBER + 5}"][1]) == 3
    assert [r[2] for r in made["cuts"][1]] == [1, 1, 2998, 2000]         # empty pieces have no member


def test_zoo_trees_have_two_codes(made):
    dynamic = 0
    for name, (gz, rows, text, cuts) in made.items():
        at = 0
        for _, _, n, size in rows:
            trees = tree_lengths(gz[at + 18:at + size - 8])
            at += size
            if trees is None:
                assert size == n + 31, name                              # the stored member
                continue
            dynamic += 1
            for lens in trees:
                assert sum(1 for l in lens if l) >= 2 and max(lens) <= 15, name
                assert sum(2.0 ** -l for l in lens if l) == 1.0, name    # complete codes: every inflater takes them
    assert dynamic > 20
    lit, dist = tree_lengths(made["all_bytes_once"][0][18:-8]) or ([], [])
    if lit:                                                              # (256 distinct bytes may also be stored)
        assert sum(1 for l in dist if l) == 2


def test_stored_fallback(made):
    gz, rows, text, _ = made["random_member"]
    assert len(rows) == 1 and len(gz) <= len(text) + 31
    assert tree_lengths(gz[18:-8]) is None


def test_distance_limit(made, tmp_path):
    """The gram at distance 32768 is matched, the one at 32769 is not: the largest distance in the member is 32768 exactly."""
    exe = str(tmp_path / "inflate_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "phagefilter_amd", "csrc"), os.path.join(ROOT, "tools", "inflate_host.cpp"),
                    "-o", exe], check=True)
    gz = made["far"][0]
    src = str(tmp_path / "far.gz")
    with open(src, "wb") as f:
        f.write(gz)
    r = subprocess.run([exe, src, str(tmp_path / "far.txt")], capture_output=True, text=True, check=True)
    rows = [line.split() for line in r.stdout.split("\n")[:-2]]
    assert len(rows) == 1 and int(rows[0][1]) == 0
    assert int(rows[0][5]) == Z.FAR
    assert open(str(tmp_path / "far.txt"), "rb").read() == made["far"][2]


def unlimited_depth(counts):
    """The longest code of a Huffman code of these counts."""
    heap = [(c, 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def test_fibonacci_counts_are_limited(made):
    """A member whose literal / length symbol counts, read back from the member itself, ask for codes beyond 15 bits: its lengths
    reach the limit and no further (that zlib takes the member is checked above)."""
    gz, rows, text, _ = made["fibonacci"]
    lit, _, counts = read_block(gz[18:-8], symbols=True)
    assert unlimited_depth(counts) > 15
    assert max(lit) == 15 and all((c > 0) == (l > 0) for c, l in zip(counts, lit))


def test_deterministic(host, made, tmp_path):
    """The same bytes on a second run, and from -O0 and -O2 builds without sanitizers."""
    others = [host, Z.build_host(str(tmp_path / "o0"), ["-O0"]), Z.build_host(str(tmp_path / "o2"), ["-O2"])]
    for name, (gz, rows, text, cuts) in made.items():
        if len(text) > 3 * Z.MEMBER:
            continue
        for exe in others:
            assert Z.run_host(exe, text, cuts, str(tmp_path)) == (gz, rows), (name, exe)


@pytest.mark.parametrize("name", Z.FASTQ_NAMES)
def test_smaller_than_partial_coders(made, name):
    gz, rows, text, _ = made[name]
    ours = len(gz)
    partial = {"huffman_only": Z.zlib_total(text, 6, zlib.Z_HUFFMAN_ONLY), "level1_fixed": Z.zlib_total(text, 1, zlib.Z_FIXED),
               "rle": Z.zlib_total(text, 6, zlib.Z_RLE)}
    print(name, len(text), ours, partial, "level 1", Z.zlib_total(text, 1, 0), "level 6", Z.zlib_total(text, 6, 0))
    for coder, theirs in partial.items():
        assert ours <= theirs, (coder, ours, theirs)
