"""pfq_text_inflate / pfq_text_parse_inflated / pfq_text_read on the device: the member zoo and the corrupt list of
tests/bgzf_ref.py (what tests/test_inflate_cpu.py runs through the same decoder on the host under sanitizers first), the grid-stride
loop, then the parse of inflated text behind a carry against pfq_text_parse of the same text, its classification and its formatted
records, and the errors."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import bgzf_ref as B
import test_ingest as ing
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_abund import strain_families
from test_gpu_build import SEEDS, _dna
from test_gpu_text import FASTQ_VARIANTS, counts_of, wrap_fastq

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 4, 200003
PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -4, -6


@pytest.fixture(scope="module")
def case(gpu):
    class X:
        pass
    x = X()
    x.rng = np.random.default_rng(1952)
    x.genomes = strain_families(x.rng, 4, 3, 2000, 0.006, 4)
    x.ids = [f"T{i:02d}" for i in range(16)]
    x.gt = BloomTree.build_balanced(x.genomes, x.ids, K, NBITS, H, *SEEDS)
    x.zoo = B.zoo()
    x.corrupt = B.corrupt_list()
    yield x
    x.gt.close()


def inflated_text(gt, n):
    """The first n bytes of the text the last inflate_text() left, through a parse (whatever it makes of them) and read_text()."""
    gt.parse_inflated("fasta")
    return gt.read_text(0, n)


def test_zoo_in_one_call(case):
    gt = case.gt
    before = gt.info().device_bytes
    gz = b"".join(m for _, _, m in case.zoo)
    got = gt.inflate_text(gz)
    want = B.scan(gz)
    assert got["stop"] == "end" and got["begin"].tolist() == want[0] and got["text_begin"].tolist() == want[1]
    assert got["status"].tolist() == [0] * len(case.zoo), [n for (n, _, _), s in zip(case.zoo, got["status"]) if s]
    text = b"".join(t for _, t, _ in case.zoo)
    assert (got["n_good"], got["good_text"]) == (len(case.zoo), len(text))
    out = inflated_text(gt, len(text))
    for (name, t, _), a in zip(case.zoo, want[1]):
        assert out[a:a + len(t)] == t, name
    assert gt.info().device_bytes >= before + len(gz) + len(text)      # the chunk and the staging buffer are counted
    copy_ms, kernel_ms = gt.last_inflate_ms()
    assert copy_ms > 0 and kernel_ms > 0


@pytest.mark.parametrize("blocks", [1, 3])
def test_grid_stride_loop(case, blocks):
    gt = case.gt
    members = ([(t, m) for _, t, m in case.zoo] * 2)[:40]
    assert len(members) == 40
    gt.set_option("PFQ_INFLATE_BLOCKS", str(blocks))
    try:
        got = gt.inflate_text(b"".join(m for _, m in members))
        assert got["status"].tolist() == [0] * 40 and got["n_good"] == 40
        text = b"".join(t for t, _ in members)
        assert inflated_text(gt, len(text)) == text
    finally:
        gt.set_option("PFQ_INFLATE_BLOCKS", None)
    for bad in ("0", "65536", "-3"):
        with pytest.raises(PfqError) as e:
            gt.set_option("PFQ_INFLATE_BLOCKS", bad)
        assert e.value.code == PFQ_ERR_ARG


def test_corrupt_list(case):
    """Every corrupt member between good ones, in one call.  What zlib refuses, stops short in or finds different from the trailer
    must have a status other than 0; the five flips of a stored block's padding bits leave a valid member, which is status 0."""
    gt = case.gt
    good_text = B.fastq_like(500, 21)
    good = B.member(good_text)
    lead = 5
    members = [good] * lead
    for _, _, m in case.corrupt:
        members += [m, good]
    got = gt.inflate_text(b"".join(members))
    status = got["status"].tolist()
    assert len(status) == lead + 2 * len(case.corrupt) and got["stop"] == "end"
    assert status[:lead] == [0] * lead and set(status[lead + 1::2]) == {0}          # the members around them are unaffected
    harmless = {f"stored_flip{b}" for b in range(3, 8)}
    kinds = {}
    for (name, _, m), s in zip(case.corrupt, status[lead::2]):
        assert (s == 0) == (name in harmless), (name, s)
        if name not in harmless:
            assert B.zlib_says(m) is None, name
        kinds[name] = s
    for kind in ("dynamic", "fixed", "stored"):
        assert (kinds[f"{kind}_crc"], kinds[f"{kind}_isize_minus"], kinds[f"{kind}_isize_plus"]) == (3, 2, 2), kind
    assert 1 in kinds.values()
    first_bad = status.index(next(s for s in status if s))
    assert first_bad == lead
    assert (got["n_good"], got["good_text"]) == (lead, lead * len(good_text))
    assert inflated_text(gt, got["good_text"]) == good_text * lead
    # the good prefix when the first corrupt member is further in, and when a valid one sits where a corrupt one might
    flip = {name: m for name, _, m in case.corrupt}
    stored_text = next(t for name, t, _ in case.corrupt if name == "stored_flip3")
    got = gt.inflate_text(good + flip["stored_flip3"] + good + flip["fixed_cut7"] + good)
    assert got["status"].tolist() == [0, 0, 0, 1, 0] and got["n_good"] == 3
    assert inflated_text(gt, got["good_text"]) == good_text + stored_text + good_text


@functools.lru_cache(maxsize=None)
def member_of(chunk):
    return B.member(chunk, 6)


def as_members(data, size):
    return b"".join(member_of(data[i:i + size]) for i in range(0, len(data), size)) + B.EOF_MARKER


def cuts_of(data):
    """About 40 carry lengths: 0, the whole text, and bytes inside headers, sequences, '+' lines and quality lines of records
    spread over the text, none of them chosen for alignment (most are no multiple of 16)."""
    starts = [0] + [i + 1 for i, c in enumerate(data) if c == 10 and i + 1 < len(data)]
    cuts = {0, 1, 17, len(data) - 1, len(data)}
    for j in range(0, len(starts) - 1, max(1, len(starts) // 34)):
        a, b = starts[j], starts[j + 1]
        cuts.add(a + (b - a) // 2 if j % 3 else a + (j % 2))
    cuts = sorted(c for c in cuts if 0 <= c <= len(data))
    assert 30 <= len(cuts) <= 50 and sum(1 for c in cuts if c % 16) > 25
    return cuts


TEXTS = dict({f"fastq_{k}": (v, "fastq") for k, v in FASTQ_VARIANTS.items()}, fasta=(ing.tricky_fasta(24), "fasta"))


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_parse_inflated_equals_parse_text(case, name):
    gt = case.gt
    data, fmt = TEXTS[name]
    wants = {}
    for final in (True, False):
        want = gt.parse_text(data, fmt, None, final, want_records=True)
        wants[final] = (want, [a.tolist() for a in gt.text_csr()])
    assert wants[True][0]["n_records"] > 20
    lines = {"header": 0, "sequence": 0, "quality": 0}
    for c in cuts_of(data):
        line = data[:c].count(b"\n") % 4 if fmt == "fastq" else None
        for key, idx in (("header", 0), ("sequence", 1), ("quality", 3)):
            lines[key] += line == idx and c > 0 and data[c - 1:c] != b"\n"
        for size in (1, 7, 300, B.BLOCK):
            gz = as_members(data[c:], size)
            inf = gt.inflate_text(gz)
            assert inf["n_good"] == inf["n_members"] and inf["good_text"] == len(data) - c and inf["stop"] == "end", (c, size)
            for final in ((True, False) if size == 7 else (True,)):
                want, want_csr = wants[final]
                got = gt.parse_inflated(fmt, data[:c], None, final, want_records=True)
                where = (name, c, size, final)
                for key in ("n_records", "consumed", "n_bases", "stop"):
                    assert got[key] == want[key], (where, key)
                assert got["rec_begin"].tolist() == want["rec_begin"].tolist(), where
                assert [a.tolist() for a in gt.text_csr()] == want_csr, where
            assert gt.read_text(0, len(data)) == data, (c, size)
            assert gt.read_text(max(c - 3, 0), min(40, len(data) - max(c - 3, 0))) == data[max(c - 3, 0):max(c - 3, 0) + 40]
    if fmt == "fastq":
        assert all(lines.values()), lines                              # cuts inside a header, a sequence and a quality line
    # a limit, and a repeat after one inflate
    inf = gt.inflate_text(as_members(data[33:], 300))
    for limit in (0, 1, len(data) // 2, len(data)):
        want = gt.parse_text(data, fmt, limit, True, want_records=True)
        for _ in range(2):
            got = gt.parse_inflated(fmt, data[:33], limit, True, want_records=True)
            assert {k: got[k] for k in ("n_records", "consumed", "n_bases", "stop")} == {k: want[k] for k in ("n_records", "consumed", "n_bases", "stop")}
            assert got["rec_begin"].tolist() == want["rec_begin"].tolist()


@pytest.fixture(scope="module")
def reads(case):
    rng, g = case.rng, case.genomes
    out = [g[int(rng.integers(16))][a:a + n] for a, n in zip(rng.integers(0, 1700, 300).tolist(), rng.integers(30, 300, 300).tolist())]
    return out + [_dna(rng, 150) for _ in range(40)] + [b"ACGT", b"A" * K, g[3][:1000]]


def test_query_and_format_of_inflated_text(case, reads):
    gt = case.gt
    data = wrap_fastq(reads)
    gt.reset_counts()
    want_off, want_leaves = gt.query_packed(*pack_reads(reads), 1.0, want_hits=True)
    want_counts = counts_of(gt)
    assert want_counts.sum() > 0
    gt.reset_counts()
    gt.parse_text(data, "fastq")
    gt.query_text(1.0, want_hits=True)
    want_fmt = gt.format_text(0, 100)
    assert want_fmt["pos_records"] + want_fmt["neg_records"] > 0 and want_fmt["pos"]
    gt.reset_counts()
    # an inflate leaves the parsed block and the counters alone
    other = wrap_fastq(reads[:50])
    gt.parse_text(other, "fastq")
    c = 1234
    inf = gt.inflate_text(as_members(data[c:], 997))
    assert inf["n_good"] == inf["n_members"] > 30
    assert counts_of(gt).sum() == 0
    assert gt.read_text(0, len(other)) == other
    gt.query_text(1.0)
    small = counts_of(gt)
    gt.reset_counts()
    gt.query_packed(*pack_reads(reads[:50]), 1.0)
    assert small.tolist() == counts_of(gt).tolist()
    gt.reset_counts()
    got = gt.parse_inflated("fastq", data[:c])
    assert (got["n_records"], got["stop"], got["consumed"]) == (len(reads), "end", len(data))
    assert counts_of(gt).sum() == 0                                   # parsing changes no counter
    off, leaves = gt.query_text(1.0, want_hits=True)
    assert off.tolist() == want_off.tolist() and leaves.tolist() == want_leaves.tolist()
    assert counts_of(gt).tolist() == want_counts.tolist()
    fmt = gt.format_text(0, 100)
    assert fmt == want_fmt
    gt.reset_counts()


def test_errors(case):
    gt, L = case.gt, _ffi.lib()
    fresh = BloomTree.build_balanced(case.genomes[:2], case.ids[:2], K, NBITS, H, *SEEDS)
    with pytest.raises(PfqError) as e:
        fresh.parse_inflated("fastq")
    assert e.value.code == PFQ_ERR_STATE
    with pytest.raises(PfqError) as e:
        fresh.read_text(0, 0)
    assert e.value.code == PFQ_ERR_STATE
    with pytest.raises(PfqError) as e:
        fresh.last_inflate_ms()
    assert e.value.code == PFQ_ERR_STATE
    got = fresh.inflate_text(b"")                                      # nothing to inflate is an inflate
    assert (got["n_members"], got["n_good"], got["good_text"], got["stop"]) == (0, 0, 0, "end")
    assert fresh.parse_inflated("fastq", b"@a\nAC\n+\n!!\n")["n_records"] == 1
    assert fresh.read_text(3, 2) == b"AC"
    fresh.close()
    gz = B.member(b"@a\nAC\n+\n!!\n")
    buf = C.create_string_buffer(gz, len(gz))
    addr, inf, out = C.addressof(buf), _ffi.TextInflated(), _ffi.Text()
    assert L.pfq_text_inflate(None, addr, len(gz), 0, 1, C.byref(inf)) == PFQ_ERR_ARG
    assert L.pfq_text_inflate(gt._h, addr, len(gz), 0, 1, None) == PFQ_ERR_ARG
    assert L.pfq_text_inflate(gt._h, None, len(gz), 0, 1, C.byref(inf)) == PFQ_ERR_ARG
    assert L.pfq_text_inflate(gt._h, addr, len(gz), 100, 1, C.byref(inf)) == PFQ_ERR_ARG
    assert L.pfq_text_inflate(gt._h, addr, len(gz), 0, 2, C.byref(inf)) == PFQ_ERR_ARG
    assert L.pfq_text_inflate(gt._h, addr, len(gz), 0, 1, C.byref(inf)) == 0 and inf.n_good == 1 and inf.good_text == 11
    assert L.pfq_text_parse_inflated(gt._h, None, 5, 0, 1, 0, C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_text_parse_inflated(gt._h, None, 0, 0, 2, 0, C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_text_parse_inflated(gt._h, None, 0, 0, 1, 4, C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_text_parse_inflated(gt._h, None, 0, 0, 1, 0, None) == PFQ_ERR_ARG
    # an over-long text: refused before a byte of the carry is read
    assert L.pfq_text_parse_inflated(gt._h, addr, (1 << 31) - 11, 0, 1, 0, C.byref(out)) == PFQ_ERR_UNSUPPORTED
    assert L.pfq_text_parse_inflated(gt._h, addr, 1 << 40, 0, 1, 0, C.byref(out)) == PFQ_ERR_UNSUPPORTED
    assert L.pfq_text_parse_inflated(gt._h, None, 0, 1 << 62, 1, 1, C.byref(out)) == 0 and out.n_records == 1
    dst = C.create_string_buffer(16)
    assert L.pfq_text_read(gt._h, 0, 11, dst) == 0 and dst.raw[:11] == b"@a\nAC\n+\n!!\n"
    assert L.pfq_text_read(gt._h, 11, 0, None) == 0
    assert L.pfq_text_read(gt._h, 5, 7, dst) == PFQ_ERR_ARG
    assert L.pfq_text_read(gt._h, 12, 0, dst) == PFQ_ERR_ARG
    assert L.pfq_text_read(gt._h, 0, 4, None) == PFQ_ERR_ARG
    assert L.pfq_text_read(None, 0, 4, dst) == PFQ_ERR_ARG
    # a member with text the trailer does not announce: its neighbours' text is where the scan put it
    got = gt.inflate_text(gz + B.frame(B.deflate(b"ACGT" * 10), 30, zlib.crc32(b"ACGT" * 10)) + gz)
    assert got["status"].tolist() == [0, 2, 0] and got["n_good"] == 1
