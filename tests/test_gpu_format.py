"""pfq_text_format on the device against tests/format_ref.py, byte for byte: the two streams, the record counts and the runs left
to the caller, for every text of tests/format_cases.py, on the golden 12-genome database and on a balanced tree of 130 leaves
whose names are 1 to 40 bytes long (rows of more than 64 names), for every block size and first index, with the knobs that
force several grid trips and hash collisions; then what the call must leave alone, and its errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import format_cases as fc
import format_ref as fr
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_build import SEEDS, _one_child_db

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "examples")
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
K, H, NBITS = 21, 4, 200003
PFQ_ERR_ARG, PFQ_ERR_FORMAT, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -3, -4, -6
FLAGS = ((True, True), (True, False), (False, True))
COMBOS = [(first, block, pos, neg) for block in fc.BLOCKS for first in fc.first_indices(block) for pos, neg in FLAGS]


def genome_of(path):
    return b"".join(l.strip() for l in open(path, "rb").read().split(b"\n") if l[:1] != b">")


class Tree:
    def __init__(self, gt, genomes, rng):
        self.gt = gt
        self.names = [t.encode() for t, _ in gt.get_leaf_counts()]
        k = gt.kmer_size
        pick = rng.integers(0, len(genomes), 160).tolist()
        hits = [genomes[g][a:a + 150] for g, a in zip(pick, rng.integers(0, 300, 160).tolist())]
        # genome reads (a few names), random reads (none), reads shorter than k (every name), and the odd ones
        self.reads = fc.odd_reads(rng) + hits + [fc.dna(rng, 150) for _ in range(100)] + [b"ACGT", b"A" * (k - 1), b""]
        self.texts = dict(fc.texts(self.reads))
        self.texts.update(fc.SMALL)
        self._done = {}

    def classified(self, name, thr=1.0):
        """The text parsed and classified on the device; its records and rows by the reference, computed once per text."""
        data, fastq = self.texts[name]
        self.gt.parse_text(data, "fastq" if fastq else "fasta")
        off, leaves = self.gt.query_text(thr, want_hits=True)
        if (name, thr) not in self._done:
            recs = fr.records(data, fastq)
            assert len(recs) == len(off) - 1
            self._done[(name, thr)] = (recs, [leaves[int(off[r]):int(off[r + 1])] for r in range(len(recs))])
        return self._done[(name, thr)]

    def check(self, recs, rows, first, block, pos, neg):
        got = self.gt.format_text(first, block, pos, neg)
        want = fr.format_ref(recs, rows, self.names, first, block, pos, neg)
        where = (first, block, pos, neg)
        assert got["left"] == want["left"], where
        assert (got["n_records"], got["pos_records"], got["neg_records"]) == (len(recs), want["pos_records"], want["neg_records"]), where
        assert got["pos"] == want["pos"], where
        assert got["neg"] == want["neg"], where
        return got


@pytest.fixture(scope="module")
def trees(gpu, tmp_path_factory):
    rng = np.random.default_rng(8192)
    db = str(tmp_path_factory.mktemp("format") / "db")
    p = subprocess.run([CLI, "build", "--genomes", os.path.join(EX, "genomes"), "--db-path", db, "--seed1", str(SEEDS[0]), "--seed2", str(SEEDS[1])],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    gdir = os.path.join(EX, "genomes")
    golden = Tree(BloomTree.load(db), [genome_of(os.path.join(gdir, f)) for f in sorted(os.listdir(gdir))], rng)
    assert len(golden.names) == 12
    genomes = [fc.dna(rng, 600) for _ in range(130)]
    ids = ["%d" % i + "n" * max(0, 1 + (i * 7) % 40 - len("%d" % i)) for i in range(130)]
    assert {len(i) for i in ids} == set(range(1, 41))
    wide = Tree(BloomTree.build_balanced(genomes, ids, K, NBITS, H, *SEEDS), genomes, rng)
    out = {"golden": golden, "wide": wide, "db": db}
    yield out
    golden.gt.close()
    wide.gt.close()


@pytest.mark.parametrize("text", sorted(list(fc.SMALL) + ["fastq", "fastq_crlf", "fastq_unterminated", "fasta", "fasta_crlf", "fasta_unterminated"]))
@pytest.mark.parametrize("which", ["golden", "wide"])
def test_every_text_block_and_first_index(trees, which, text):
    t = trees[which]
    recs, rows = t.classified(text)
    if text == "fastq":
        assert sum(len(r) == len(t.names) for r in rows) >= 20 and sum(0 < len(r) < len(t.names) for r in rows) >= 100   # every name; a few
        assert sum(len(r) == 0 for r in rows) >= 90
    for first, block, pos, neg in COMBOS:
        t.check(recs, rows, first, block, pos, neg)


@pytest.mark.parametrize("thr", [1.0, 0.5])
@pytest.mark.parametrize("which", ["golden", "wide"])
def test_both_streams_fill(trees, which, thr):
    t = trees[which]
    recs, rows = t.classified("fastq", thr)
    got = t.check(recs, rows, 0, 1, True, True)                      # blocks of one record: nothing is left
    assert got["left"] == [] and got["pos_records"] > 100 and got["neg_records"] > 90
    assert got["pos_records"] + got["neg_records"] == len(recs)
    got = t.check(recs, rows, 0, 100, True, True)
    assert [x[4] for x in got["left"]] == ["repeated_id", "tail"] and got["pos"] and got["neg"]


@pytest.mark.parametrize("knob,value", [("PFQ_TEXT_TILE", "256"), ("PFQ_FMT_GRID", "1"), ("PFQ_FMT_HASH_BITS", "2")])
@pytest.mark.parametrize("text", ["fastq", "fasta_crlf"])
def test_knobs_change_nothing(trees, text, knob, value):
    t = trees["wide"]
    recs, rows = t.classified(text)
    plain = [t.gt.format_text(first, block, True, True) for first, block in ((0, 7), (3, 64), (0, 100))]
    t.gt.set_option(knob, value)
    try:
        recs2, rows2 = t.classified(text)                            # (parsed again: the text tile is the parser's)
        assert recs2 is recs
        for (first, block), want in zip(((0, 7), (3, 64), (0, 100)), plain):
            assert t.check(recs, rows, first, block, True, True) == want
    finally:
        t.gt.set_option(knob, None)
    for bad, name in (("0", "PFQ_FMT_HASH_BITS"), ("65", "PFQ_FMT_HASH_BITS"), ("0", "PFQ_FMT_GRID")):
        with pytest.raises(PfqError) as e:
            t.gt.set_option(name, bad)
        assert e.value.code == PFQ_ERR_ARG


def test_a_block_of_8192_records(trees):
    """The largest result block: 8192 keys in one workgroup's LDS; then the same text with the block's first and last id equal."""
    t = trees["golden"]
    for first_id in (b"i0", b"i8191"):
        data = b"".join(b"@%s\nAC\n+\n!!\n" % (first_id if i == 0 else b"i%d" % i) for i in range(8200))
        t.gt.parse_text(data, "fastq")
        off, leaves = t.gt.query_text(1.0, want_hits=True)
        recs = fr.records(data, True)
        rows = [leaves[int(off[r]):int(off[r + 1])] for r in range(len(recs))]
        assert all(len(r) == 12 for r in rows)                       # shorter than k: every leaf
        got = t.check(recs, rows, 0, 8192, True, True)
        assert got["left"] == ([(8192, 8, len(got["pos"]), 0, "tail")] if first_id == b"i0" else [(0, 8192, 0, 0, "repeated_id"), (8192, 8, 0, 0, "tail")])
        t.check(recs, rows, 8184, 8192, False, True)                 # a head of 8 records, then a whole block with every id once


def test_repeating_and_what_the_call_leaves_alone(trees):
    t = trees["golden"]
    gt, L = t.gt, _ffi.lib()
    data, fastq = t.texts["fastq"]
    gt.parse_text(data, "fastq")
    hits = _ffi.Hits()
    _ffi.check(L.pfq_text_query(gt._h, 1.0, _ffi.WANT_HITS, C.byref(hits)))
    n = int(hits.n_reads)
    off = np.ctypeslib.as_array(hits.offsets, shape=(n + 1,))
    leaves = np.ctypeslib.as_array(hits.leaves, shape=(int(off[-1]),))
    before = (off.copy(), leaves.copy(), gt.get_leaf_counts(), bytes(gt.last_stats()))
    first = gt.format_text(3, 64)
    for _ in range(3):
        assert gt.format_text(3, 64) == first                        # repeated: the same result
    assert gt.format_text(0, 7, neg=False)["neg"] == b"" and gt.format_text(3, 64) == first
    assert off.tolist() == before[0].tolist() and leaves.tolist() == before[1].tolist()
    assert gt.get_leaf_counts() == before[2] and bytes(gt.last_stats()) == before[3]
    seq, csr = gt.text_csr()
    assert seq.tobytes() == b"".join(r[1] for r in fr.records(data, fastq))   # the parsed block stands
    gt.reset_counts()


def test_stage_times_and_device_bytes(trees):
    t = trees["golden"]
    gt = t.gt
    t.classified("fastq")
    gt.format_text()
    with pytest.raises(PfqError) as e:
        gt.last_format_ms()
    assert e.value.code == PFQ_ERR_STATE                             # not timed
    gt.set_option("PFQ_FMT_TIME", "1")
    try:
        gt.format_text()
        ms = gt.last_format_ms()
        assert len(ms) == 3 and all(0.0 <= x < 1000.0 for x in ms)
    finally:
        gt.set_option("PFQ_FMT_TIME", None)
    before = gt.info().device_bytes
    data = b"".join(b"@big%d\n%s\n+\n%s\n" % (i, b"ACGT" * 1000, b"I" * 4000) for i in range(300))
    gt.parse_text(data, "fastq")
    gt.query_text(1.0, want_hits=True)
    parsed = gt.info().device_bytes
    got = gt.format_text(0, 100, True, True)
    assert got["left"] == [] and len(got["pos"]) + len(got["neg"]) > (2 << 20)
    assert gt.info().device_bytes >= max(before, parsed) + (2 << 20)   # the new buffers are counted
    gt.reset_counts()


def test_errors(trees, tmp_path):
    t = trees["golden"]
    gt, L = t.gt, _ffi.lib()
    out = _ffi.TextRecords()

    def state(tree):
        with pytest.raises(PfqError) as e:
            tree.format_text()
        assert e.value.code == PFQ_ERR_STATE

    fresh = BloomTree.load(trees["db"])
    state(fresh)                                                      # before any parse
    data, _ = t.texts["same_id"]
    fresh.parse_text(data, "fastq")
    state(fresh)                                                      # parsed, never classified
    fresh.query_text(1.0)
    state(fresh)                                                      # classified without PFQ_WANT_HITS
    fresh.query_text(1.0, want_hits=True, paired=True)
    state(fresh)                                                      # fragments
    fresh.query_text(1.0, want_hits=True)
    assert fresh.format_text(0, 2)["left"] == [(0, 2, 0, 0, "repeated_id")]
    fresh.query_packed(*pack_reads([b"ACGT" * 10]), 1.0, want_hits=True)
    state(fresh)                                                      # another query call in between
    fresh.query_text(1.0, want_hits=True)
    fresh.parse_text(data, "fastq")
    state(fresh)                                                      # another parse in between
    fresh.query_text(1.0, want_hits=True)
    for block, flags in ((0, 3), (8193, 3), (100, 0), (100, 4), (100, 7)):
        assert L.pfq_text_format(fresh._h, 0, block, flags, C.byref(out)) == PFQ_ERR_ARG, (block, flags)
    assert L.pfq_text_format(None, 0, 100, 3, C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_text_format(fresh._h, 0, 100, 3, None) == PFQ_ERR_ARG
    assert L.pfq_text_format(fresh._h, 0, 8192, 3, C.byref(out)) == 0 and out.n_left == 1
    assert L.pfq_debug_last_format(fresh._h, None) == PFQ_ERR_ARG
    fresh.close()
    shard = BloomTree.load_subtree(trees["db"], 1, 0)                 # partial rows
    shard.parse_text(data, "fastq")
    shard.query_text(1.0, want_hits=True)
    with pytest.raises(PfqError) as e:
        shard.format_text()
    assert e.value.code == PFQ_ERR_UNSUPPORTED
    shard.close()
    db = tmp_path / "one_child"                                       # a failed insertion is sticky here too
    genome = _one_child_db(db, False)
    bad = BloomTree.load(str(db))
    bad.set_option("PFQ_GREEDY_HOST", "1")
    with pytest.raises(PfqError):
        bad.insert(genome, "new")
    with pytest.raises(PfqError) as e:
        bad.format_text()
    assert e.value.code == PFQ_ERR_FORMAT and "only one child" in str(e.value)
    bad.close()
