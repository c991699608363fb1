"""Blocked gzip written on the device (pfq_bgzf_deflate, pfq_text_format_gz): the bytes must be those of the stand-alone host
program tools/deflate_host.cpp, which compiles the same core (tests/test_deflate_cpu.py holds that program against zlib), whatever
the grid; the tables must agree with pfq_gz_scan; the device's own inflater must take every member; and the deflated streams of
pfq_text_format_gz must inflate, piece by piece, to what pfq_text_format gives between the same left runs."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_zoo as Z
import format_cases as fc
from phagefilter_amd import BloomTree, PfqError, _ffi, gz_scan, pack_reads

pytestmark = pytest.mark.gpu

EX = os.path.join(Z.ROOT, "tests", "golden", "examples")
CLI = os.path.join(Z.ROOT, "phagefilter_amd", "phage_filter")
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
K, H, NBITS = 21, 4, 200003
PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -4, -6


@pytest.fixture(scope="module")
def host_made(tmp_path_factory):
    """name -> (gz, rows, text, cuts) by the host program, computed once."""
    tmp = tmp_path_factory.mktemp("deflate_host")
    exe = Z.build_host(str(tmp / "deflate_host"), ["-O2"])
    return {name: Z.run_host(exe, text, cuts, str(tmp)) + (text, cuts) for name, text, cuts in Z.zoo()}


@pytest.fixture(scope="module")
def trees(gpu, tmp_path_factory):
    """The two small trees of tests/test_gpu_format.py: the golden genomes' database and 130 leaves with names of every length."""
    rng = np.random.default_rng(8192)
    db = str(tmp_path_factory.mktemp("deflate") / "db")
    p = subprocess.run([CLI, "build", "--genomes", os.path.join(EX, "genomes"), "--db-path", db, "--seed1", str(SEEDS[0]), "--seed2", str(SEEDS[1])],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    gdir = os.path.join(EX, "genomes")
    golden_genomes = [b"".join(l.strip() for l in open(os.path.join(gdir, f), "rb").read().split(b"\n") if l[:1] != b">") for f in sorted(os.listdir(gdir))]
    genomes = [fc.dna(rng, 600) for _ in range(130)]
    ids = ["%d" % i + "n" * max(0, 1 + (i * 7) % 40 - len("%d" % i)) for i in range(130)]
    out = {"golden": (BloomTree.load(db), golden_genomes), "wide": (BloomTree.build_balanced(genomes, ids, K, NBITS, H, *SEEDS), genomes), "db": db}
    texts = {}
    for which in ("golden", "wide"):
        g = out[which][1]
        pick = rng.integers(0, len(g), 160).tolist()
        hits = [g[i][a:a + 150] for i, a in zip(pick, rng.integers(0, 300, 160).tolist())]
        reads = fc.odd_reads(rng) + hits + [fc.dna(rng, 150) for _ in range(100)] + [b"ACGT", b"A" * (K - 1), b""]
        texts[which] = dict(fc.texts(reads))
    out["texts"] = texts
    yield out
    out["golden"][0].close()
    out["wide"][0].close()


def same_as_host(gt, made):
    for name, (gz, rows, text, cuts) in made.items():
        got = gt.deflate_bytes(text, cuts)
        assert got["gz"] == gz, name                                     # byte for byte the host program's
        begin = np.concatenate([[0], np.cumsum([r[3] for r in rows])]).astype(np.uint64)
        assert got["n_members"] == len(rows) and got["member_begin"].tolist() == begin.tolist(), name
        scan = gz_scan(gz)
        assert scan["stop"] == "end" and scan["begin"].tolist() == begin.tolist() and scan["text_bytes"] == len(text), name
        first = {}                                                       # where every piece begins: at its first member, or where the next does
        for m, r in enumerate(rows):
            first.setdefault(r[0], int(begin[m]))
        want, at = [], len(gz)
        for piece in range(len(cuts), -1, -1):
            at = first.get(piece, at)
            want.append(at)
        assert got["piece_begin"].tolist() == want[::-1] + [len(gz)], name


def test_bytes_are_the_host_programs(trees, host_made):
    gt = trees["golden"][0]
    assert max(len(v[1]) for v in host_made.values()) >= 3
    same_as_host(gt, host_made)                                          # the default grid: a workgroup a member here


def test_one_workgroup_takes_every_member(trees, host_made):
    gt = trees["golden"][0]
    gt.set_option("PFQ_DEFLATE_BLOCKS", "1")
    try:
        same_as_host(gt, {k: v for k, v in host_made.items() if len(v[1]) >= 2 or k in ("far", "fibonacci", "random_member")})
    finally:
        gt.set_option("PFQ_DEFLATE_BLOCKS", None)
    for bad in ("0", "65536"):
        with pytest.raises(PfqError) as e:
            gt.set_option("PFQ_DEFLATE_BLOCKS", bad)
        assert e.value.code == PFQ_ERR_ARG


def test_round_trip_through_the_device(trees, host_made):
    gt = trees["wide"][0]
    for name, (gz, rows, text, cuts) in host_made.items():
        got = gt.deflate_bytes(text, cuts)["gz"]
        inf = gt.inflate_text(got)
        assert inf["stop"] == "end" and inf["n_good"] == len(rows) and inf["good_text"] == len(text) and not inf["status"].any(), name
        if name in Z.FASTQ_NAMES:
            parsed = gt.parse_inflated("fastq")
            assert parsed["consumed"] == len(text) and parsed["n_records"] == text.count(b"\n") // 4, name
            assert gt.read_text(0, len(text)) == text, name


@pytest.mark.parametrize("which", ["golden", "wide"])
def test_format_text_gz(trees, which):
    gt = trees[which][0]
    for text in ("fastq", "fasta_crlf"):
        data, fastq = trees["texts"][which][text]
        gt.parse_text(data, "fastq" if fastq else "fasta")
        gt.query_text(1.0, want_hits=True)
        for first, block in ((0, 7), (3, 64), (0, 100)):
            for pos, neg in ((True, True), (True, False), (False, True)):
                plain = gt.format_text(first, block, pos, neg)
                got = gt.format_text_gz(first, block, pos, neg)
                where = (text, first, block, pos, neg)
                for key in ("n_records", "pos_records", "neg_records", "left"):
                    assert got[key] == plain[key], (where, key)
                assert (got["pos_bytes"], got["neg_bytes"]) == (len(plain["pos"]), len(plain["neg"])), where
                for s, at in (("pos", 2), ("neg", 3)):
                    bounds = [0] + [x[at] for x in plain["left"]] + [len(plain[s])]
                    gz, pb = got[s + "_gz"], got[s + "_piece_begin"].tolist()
                    assert len(pb) == len(bounds) and pb[0] == 0 and pb[-1] == len(gz), where
                    for j in range(len(bounds) - 1):
                        piece = gz[pb[j]:pb[j + 1]]
                        want = plain[s][bounds[j]:bounds[j + 1]]
                        assert _members(piece) == want, (where, s, j)
                assert _plain(gt.format_text_gz(first, block, pos, neg)) == _plain(got), where   # repeated: the same bytes
                assert gt.format_text(first, block, pos, neg) == plain, where       # and format_text gives what it gave
    gt.reset_counts()


def _plain(d):
    return {k: v.tolist() if isinstance(v, np.ndarray) else v for k, v in d.items()}


def _members(gz):
    """Every member of gz inflated, one after the other (zlib.decompress takes only the first)."""
    out, rest = [], gz
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        assert d.eof
        rest = d.unused_data
    return b"".join(out)


def test_states_errors_and_times(trees, host_made):
    L = _ffi.lib()
    fresh = BloomTree.load(trees["db"])
    out, pg, ng, bg = _ffi.TextRecords(), _ffi.Bgzf(), _ffi.Bgzf(), _ffi.Bgzf()
    with pytest.raises(PfqError) as e:
        fresh.last_deflate_ms()
    assert e.value.code == PFQ_ERR_STATE                              # no deflate yet
    assert fresh.deflate_bytes(b"")["gz"] == b""
    assert fresh.deflate_bytes(b"", (0, 0))["piece_begin"].tolist() == [0, 0, 0, 0]
    with pytest.raises(PfqError) as e:
        fresh.last_deflate_ms()
    assert e.value.code == PFQ_ERR_STATE                              # none that had members

    def state(tree):
        with pytest.raises(PfqError) as e:
            tree.format_text_gz()
        assert e.value.code == PFQ_ERR_STATE

    state(fresh)                                                      # before any parse
    data = b"@a\nACGT\n+\nIIII\n@a\nACGT\n+\nIIII\n"
    fresh.parse_text(data, "fastq")
    state(fresh)                                                      # parsed, never classified
    fresh.query_text(1.0)
    state(fresh)                                                      # classified without PFQ_WANT_HITS
    fresh.query_text(1.0, want_hits=True, paired=True)
    state(fresh)                                                      # fragments
    fresh.query_text(1.0, want_hits=True)
    got = fresh.format_text_gz(0, 2)
    assert got["left"] == [(0, 2, 0, 0, "repeated_id")] and got["pos_gz"] == b"" and got["neg_gz"] == b""
    fresh.query_packed(*pack_reads([b"ACGT" * 10]), 1.0, want_hits=True)
    state(fresh)                                                      # another query call in between
    fresh.parse_text(data, "fastq")
    fresh.query_text(1.0, want_hits=True)
    for block, flags in ((0, 3), (8193, 3), (100, 0), (100, 4), (100, 7)):
        assert L.pfq_text_format_gz(fresh._h, 0, block, flags, C.byref(out), C.byref(pg), C.byref(ng)) == PFQ_ERR_ARG, (block, flags)
    assert L.pfq_text_format_gz(None, 0, 100, 3, C.byref(out), C.byref(pg), C.byref(ng)) == PFQ_ERR_ARG
    assert L.pfq_text_format_gz(fresh._h, 0, 100, 3, None, C.byref(pg), C.byref(ng)) == PFQ_ERR_ARG
    assert L.pfq_text_format_gz(fresh._h, 0, 100, 3, C.byref(out), None, C.byref(ng)) == PFQ_ERR_ARG
    assert L.pfq_text_format_gz(fresh._h, 0, 1, 3, C.byref(out), C.byref(pg), C.byref(ng)) == 0 and not out.pos and not out.neg
    assert pg.n_members == 1 and _members(C.string_at(pg.gz, pg.gz_bytes)) == fresh.format_text(0, 1)["pos"] != b""
    buf = np.zeros(10, dtype=np.uint8)
    cuts = np.array([3, 2], dtype=np.uint64)
    assert L.pfq_bgzf_deflate(fresh._h, buf.ctypes.data, 10, cuts.ctypes.data, 2, C.byref(bg)) == PFQ_ERR_ARG    # not ascending
    cuts[:] = (3, 11)
    assert L.pfq_bgzf_deflate(fresh._h, buf.ctypes.data, 10, cuts.ctypes.data, 2, C.byref(bg)) == PFQ_ERR_ARG    # beyond len
    assert L.pfq_bgzf_deflate(fresh._h, None, 10, None, 0, C.byref(bg)) == PFQ_ERR_ARG
    assert L.pfq_bgzf_deflate(fresh._h, buf.ctypes.data, 10, None, 2, C.byref(bg)) == PFQ_ERR_ARG
    assert L.pfq_bgzf_deflate(fresh._h, buf.ctypes.data, 10, None, 0, None) == PFQ_ERR_ARG
    assert L.pfq_bgzf_deflate(None, buf.ctypes.data, 10, None, 0, C.byref(bg)) == PFQ_ERR_ARG
    assert L.pfq_bgzf_deflate(fresh._h, buf.ctypes.data, 1 << 31, None, 0, C.byref(bg)) == PFQ_ERR_UNSUPPORTED
    assert L.pfq_debug_last_deflate(fresh._h, None) == PFQ_ERR_ARG
    before = fresh.info().device_bytes
    gz, rows, text, cuts = host_made["synthetic_fastq"]
    assert fresh.deflate_bytes(text)["gz"] == gz
    ms = fresh.last_deflate_ms()
    assert len(ms) == 3 and all(0.0 <= x < 10000.0 for x in ms)
    assert fresh.info().device_bytes >= before + len(text)            # the buffers are counted
    fresh.close()
