"""pfq_text_parse / pfq_text_query on the device against tests/text_ref.py: every field, rec_begin and the parsed CSR exactly, with
the smallest text tile (256 bytes a block: lines begin on the first and last bytes of tiles, lines span many tiles) and with the
built-in one; then the classification of a parsed block against query_packed of the same reads."""
import ctypes as C

import numpy as np
import pytest

import test_ingest as ing
import text_ref
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_abund import strain_families
from test_gpu_build import SEEDS, _dna
from test_text_cpu import ADVERSARIAL, MALFORMED_TAILS

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 4, 200003
DEFAULT_TILE = 8192
TILES = [256, None]
PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -4, -6


class Case:
    def __init__(self):
        rng = self.rng = np.random.default_rng(90210)
        self.genomes = strain_families(rng, 4, 3, 2000, 0.006, 4)
        self.ids = [f"T{i:02d}" for i in range(16)]
        self.gt = BloomTree.build_balanced(self.genomes, self.ids, K, NBITS, H, *SEEDS)
        self._ref = {}

    def ref(self, data, fastq, limit, final):
        """The reference, computed once per input; nothing changes it."""
        key = (data, fastq, limit, final)
        if key not in self._ref:
            self._ref[key] = text_ref.scan(data, fastq, limit, final)
        return self._ref[key]

    def check(self, data, fastq, limit=None, final=True):
        seqs, begins, consumed, stop = self.ref(data, fastq, limit, final)
        got = self.gt.parse_text(data, "fastq" if fastq else "fasta", limit, final, want_records=True)
        where = (len(data), fastq, limit, final)
        assert (got["n_records"], got["consumed"], got["stop"]) == (len(seqs), consumed, stop), where
        assert got["n_bases"] == sum(map(len, seqs)), where
        assert got["rec_begin"].tolist() == begins, where
        seq, off = self.gt.text_csr()
        assert seq.tobytes() == b"".join(seqs), where
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in seqs], dtype=np.int64)]).tolist(), where
        return got


@pytest.fixture(scope="module")
def case(gpu):
    x = Case()
    yield x
    x.gt.close()


@pytest.fixture(params=TILES, ids=["tile256", "tile_default"])
def tiled(case, request):
    case.gt.set_option("PFQ_TEXT_TILE", None if request.param is None else str(request.param))
    yield case
    case.gt.set_option("PFQ_TEXT_TILE", None)


def single_line_fastq(eol=b"\n", final_newline=True):
    """About 60 records of 1 - 90 bases, one of 700 bases, one header of 300 bytes."""
    rng = np.random.default_rng(31337)
    out = []
    for i in range(62):
        L = 700 if i == 9 else int(rng.integers(1, 91))
        header = b"@r%d " % i + b"x" * 296 if i == 4 else b"@r%d extra /1" % i
        seq = _dna(rng, L)
        qual = bytes(rng.choice(np.frombuffer(b"@@@+++!IJ#5", dtype=np.uint8), L).astype(np.uint8))
        out.append(eol.join([header, seq, b"+" if i % 2 else b"+r%d" % i, qual]) + eol)
    data = b"".join(out)
    return data if final_newline else data[:-len(eol)]


FASTQ_VARIANTS = {"lf": single_line_fastq(), "crlf": single_line_fastq(b"\r\n"), "no_final_newline": single_line_fastq(final_newline=False)}


@pytest.mark.parametrize("variant", sorted(FASTQ_VARIANTS))
def test_fastq_every_cut(tiled, variant):
    data = FASTQ_VARIANTS[variant]
    assert tiled.check(data, True)["n_records"] == 62
    for cut in range(1501):
        for final in (True, False):
            tiled.check(data[:cut], True, None, final)


@pytest.mark.parametrize("variant", sorted(FASTQ_VARIANTS))
def test_fastq_limits_round_every_line_start(tiled, variant):
    data = FASTQ_VARIANTS[variant]
    starts = [0] + [i + 1 for i, c in enumerate(data) if c == 10 and i + 1 < len(data)]
    for s in starts:
        for limit in (s - 1, s, s + 1):
            if limit >= 0:
                tiled.check(data, True, limit, True)
    tiled.check(data, True, len(data) + 5, False)


def test_fastq_slow_paths(tiled):
    good = ing.tricky_fastq(50, multiline=False)
    one = good[:text_ref.scan(good, True, 1)[2]]                     # its first record
    multi = b"@m\nACGT\nAC\n+\n!!!!\n!!\n"
    got = tiled.check(ing.tricky_fastq(40, multiline=False) + multi + one, True)
    assert (got["stop"], got["n_records"]) == ("slow", 40)
    got = tiled.check(multi + good, True)
    assert (got["stop"], got["n_records"]) == ("slow", 0)
    got = tiled.check(ADVERSARIAL, True)
    assert (got["stop"], got["n_records"]) == ("slow", 0)
    tiled.check(ADVERSARIAL[ADVERSARIAL.index(b"@III1"):], True)      # a false record start
    for tail in MALFORMED_TAILS:
        got = tiled.check(good + tail, True)
        assert got["stop"] == "slow" and got["n_records"] >= 50
        tiled.check(good + tail, True, None, False)
    tiled.check(b"@a 1\nACGTACGT\n+\n!!!\n@b\nAC\n+\nIIIIIIII\n@c\n\n+\n!\n@d\nAC  \r\n+\r\n \t\r\n", True)


@pytest.mark.parametrize("crlf", [False, True])
def test_fasta(tiled, crlf):
    data = ing.tricky_fasta(24, crlf=crlf)
    assert tiled.check(data, False)["n_records"] == 24
    assert tiled.check(data, False, None, False)["stop"] == "more"
    headers = [i for i in range(len(data)) if data[i:i + 1] == b">" and (i == 0 or data[i - 1] == 10)]
    for h in headers:
        for limit in (h - 1, h, h + 1):
            if limit >= 0:
                tiled.check(data, False, limit, True)
    for limit in (0, 1, 5000, len(data)):
        tiled.check(data, False, limit, False)
    for cut in list(range(0, 300)) + [len(data) // 2, len(data) - 1]:
        for final in (True, False):
            tiled.check(data[:cut], False, None, final)
    tiled.check(data[:-1], False)                                     # no final newline


def test_small_and_odd_texts(tiled):
    for fastq in (True, False):
        for data in (b"", b"A", b"\n", b">", b"@", b"ACGT\n>a\nAC\n", b"@a\nAC\n+\n!!\n", b">a\nAC\n", b"\n\n\n\n\n\n\n\n", b"\r\n" * 40):
            for final in (True, False):
                for limit in (None, 0, 1):
                    tiled.check(data, fastq, limit, final)
    assert tiled.gt.parse_text(b"ACGT\n>a\nAC\n", "fasta")["stop"] == "slow"


def test_lengths_round_the_tiles(tiled):
    """Texts of 255, 256, 257 and k * tile +- 1 bytes, cut from a FASTQ file whose lines fall wherever they fall, from a FASTA file
    with one record of many tiles, and texts built so that a line begins exactly on a tile's first and last byte."""
    fq = ing.tricky_fastq(260, multiline=False)
    fa = b">long one\n" + b"\n".join(_dna(tiled.rng, 70) for _ in range(400)) + b"\n>next\n" + _dna(tiled.rng, 3 * DEFAULT_TILE + 5) + b"\n>last\nACGT\n"
    assert len(fq) > 3 * DEFAULT_TILE + 1 and len(fa) > 6 * DEFAULT_TILE
    lengths = [255, 256, 257, 511, 512, 513] + [k * DEFAULT_TILE + d for k in (1, 2, 3) for d in (-1, 0, 1)]
    for n in lengths:
        for final in (True, False):
            tiled.check(fq[:n], True, None, final)
            tiled.check(fa[:n], False, None, final)
    tiled.check(fa, False)
    for tile in (256, DEFAULT_TILE):
        for edge in (tile - 1, tile, tile + 1):                      # the second record's header begins at byte `edge`
            first = b"@a\nAAA\n+\n" + b"!" * (edge - 10) + b"\n"
            assert len(first) == edge
            tiled.check(first + b"@b\nACGT\n+\n!!!!\n", True)
            tiled.check(b">a\n" + b"C" * (edge - 4) + b"\n>b\nACGT\n", False)


def wrap_fastq(reads):
    return b"".join(b"@q%d\n%s\n+\n%s\n" % (i, r, b"I" * max(len(r), 1)) for i, r in enumerate(reads))


def wrap_fasta(reads):
    return b"".join(b">q%d some words\n%s\n" % (i, b"\n".join(r[j:j + 60] for j in range(0, len(r), 60))) for i, r in enumerate(reads))


def counts_of(gt):
    return np.array([c for _, c in gt.get_leaf_counts()], dtype=np.int64)


@pytest.fixture(scope="module")
def reads(case):
    rng, g = case.rng, case.genomes
    out = [g[int(rng.integers(16))][a:a + n] for a, n in zip(rng.integers(0, 1700, 300).tolist(), rng.integers(30, 300, 300).tolist())]
    return out + [_dna(rng, 150) for _ in range(40)] + [b"ACGT", b"A" * K, g[3][:1000]]


@pytest.mark.parametrize("thr", [1.0, 0.5])
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_classification_equals_query_packed(tiled, reads, fastq, thr):
    gt = tiled.gt
    data = wrap_fastq(reads) if fastq else wrap_fasta(reads)
    seqs = tiled.ref(data, fastq, None, True)[0]
    assert seqs == reads
    gt.reset_counts()
    want_off, want_leaves = gt.query_packed(*pack_reads(seqs), thr, want_hits=True)
    want_counts = counts_of(gt)
    assert want_counts.sum() > 0
    gt.reset_counts()
    tiled.check(data, fastq)
    assert counts_of(gt).sum() == 0                                   # parsing changes no counter
    gt.query_packed(*pack_reads(seqs[:7]), thr)                       # a query call between parse and query disturbs nothing
    between = counts_of(gt)
    off, leaves = gt.query_text(thr, want_hits=True)
    assert off.tolist() == want_off.tolist() and leaves.tolist() == want_leaves.tolist()
    assert (counts_of(gt) - between).tolist() == want_counts.tolist()
    assert gt.last_stats().n_reads == len(seqs)
    gt.query_text(thr)                                                # again on the same block: the increase doubles
    assert (counts_of(gt) - between).tolist() == (2 * want_counts).tolist()
    gt.reset_counts()


def test_errors(case):
    gt, L = case.gt, _ffi.lib()
    fresh = BloomTree.build_balanced(case.genomes[:2], case.ids[:2], K, NBITS, H, *SEEDS)
    with pytest.raises(PfqError) as e:
        fresh.query_text(1.0)
    assert e.value.code == PFQ_ERR_STATE
    fresh.close()
    out, buf = _ffi.Text(), C.create_string_buffer(b"@a\nAC\n+\n!!\n")
    addr = C.addressof(buf)
    assert L.pfq_text_parse(None, addr, 11, 11, 1, 0, C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_text_parse(gt._h, addr, 11, 11, 1, 0, None) == PFQ_ERR_ARG
    assert L.pfq_text_parse(gt._h, None, 11, 11, 1, 0, C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_text_parse(gt._h, addr, 11, 11, 2, 0, C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_text_parse(gt._h, addr, 11, 11, -1, 0, C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_text_parse(gt._h, addr, 11, 11, 1, 4, C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_text_parse(gt._h, addr, 1 << 31, 11, 1, 0, C.byref(out)) == PFQ_ERR_UNSUPPORTED   # (refused before a byte is read)
    assert L.pfq_text_parse(gt._h, None, 0, 11, 1, 0, C.byref(out)) == 0 and out.stop == _ffi.TEXT_END and out.n_records == 0
    for bad in ("100", "255", "300", "16384", "0"):
        with pytest.raises(PfqError) as e:
            gt.set_option("PFQ_TEXT_TILE", bad)
        assert e.value.code == PFQ_ERR_ARG
    before = gt.info().device_bytes
    gt.parse_text(b">a\n" + b"ACGT" * (1 << 18) + b"\n", "fasta")
    assert gt.info().device_bytes >= before + (1 << 20)               # the new buffers are counted
