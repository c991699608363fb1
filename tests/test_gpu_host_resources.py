"""The host library's events, streams and page-locked blocks through the calls that make, use and destroy them: the gates of the
eight stage timers (pfq_debug_last_*) with the messages a fresh tree answers, every lazily made resource through three
open-use-close cycles that must repeat each other, and the four staging slots of pfq_tree_insert through genomes that grow,
shrink and come round again.  What the calls compute is checked where they are tested; here a later cycle is held to the first."""
import ctypes as C
import math

import numpy as np
import pytest

import bgzf_ref as B
from hipbuf import hip
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads, query_batch
from test_gpu_build import SEEDS, _assert_same_tree, _dna
from test_gpu_deplete import HB, KB, NBITS_B
from test_gpu_overlap import AD33
from test_gpu_prep import H, K, NBITS, PFQ_ERR_STATE, counts_of, pack_quals

pytestmark = pytest.mark.gpu

N_GENOMES, GLEN, N_FRAGMENTS, READ_LEN = 8, 3000, 32, 100
PREP = dict(trim_quality=20, trim_window=4, min_length=K)
OVERLAP, ERRORS, HIGH, LOW = 30, 10, 30, 14
# what a tree answers before the call that arms the getter: copied from the library's source as it was before the timers had a
# type of their own, never read from the library under test; and how many intervals the getter documents
GATES = {
    "last_inflate_ms": ("pfq_debug_last_inflate before a pfq_text_inflate with members on this tree", 2),
    "last_deflate_ms": ("pfq_debug_last_deflate before a deflate call with members on this tree", 3),
    "last_format_ms": ("pfq_debug_last_format before a pfq_text_format with records and PFQ_FMT_TIME=1 on this tree", 3),
    "last_prep_ms": ("pfq_debug_last_prep before a pfq_prep_reads with reads on this tree", 3),
    "last_adapters_ms": ("pfq_debug_last_adapters: the last pfq_prep_reads with reads on this tree ran without adapters", 1),
    "last_overlap_ms": ("pfq_debug_last_overlap: the last pfq_prep_reads with reads on this tree ran without the mate overlap", 1),
    "last_corrections_ms": ("pfq_debug_last_corrections: the last pfq_prep_reads with reads on this tree wrote no patch list "
                            "(the mate correction and PFQ_PREP_WANT_READS)", 1),
    "last_deplete_ms": ("pfq_debug_last_deplete before a pfq_prep_deplete with units on this tree", 2),
}


class Data:
    """Built once and never changed: the genomes, a block of 32 fragments (64 reads of 100 bases with qualities: inserts of 150
    bases whose mates overlap by 50, every fourth of 80 with adapter read-through, every third with a wrong base of low quality
    against a good one inside the overlap), its FASTQ text and that text as blocked gzip."""

    def __init__(self):
        rng = np.random.default_rng(1917)
        self.genomes = [_dna(rng, GLEN) for _ in range(N_GENOMES)]
        self.ids = [f"R{i}" for i in range(N_GENOMES)]
        self.reads, self.quals = [], []
        for n in range(N_FRAGMENTS):
            size = 80 if n % 4 == 3 else 150
            g = self.genomes[n % N_GENOMES]
            at = int(rng.integers(0, GLEN - size + 1))
            ins = g[at:at + size]
            a = bytearray((ins + AD33 + _dna(rng, READ_LEN))[:READ_LEN])
            b = bytearray((orc.revcomp(ins) + _dna(rng, READ_LEN))[:READ_LEN])
            qa, qb = bytearray(b"I" * READ_LEN), bytearray(b"I" * READ_LEN)
            if n % 3 == 0 and size == 150:                            # position 70 of the insert lies in both mates
                a[70] = {65: 67, 67: 71, 71: 84, 84: 65}[a[70]]
                qa[70] = 2 + 33
            self.reads += [bytes(a), bytes(b)]
            self.quals += [bytes(qa), bytes(qb)]
        self.text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(self.reads, self.quals)))
        self.gz = B.member(self.text[:3000]) + B.member(self.text[3000:]) + B.EOF_MARKER

    def trees(self, device=0):
        main = BloomTree.build_balanced(self.genomes, self.ids, K, NBITS, H, *SEEDS, device=device)
        screen = BloomTree.build_balanced(self.genomes[:1], ["S0"], KB, NBITS_B, HB, *SEEDS, device=device)
        return main, screen

    def prep(self, tree, steps=True, reads=None):
        """The block (or `reads`, without qualities) through pfq_prep_reads, with the three optional steps or without."""
        if steps:
            tree.set_adapters([AD33])
            tree.set_mate_overlap(OVERLAP, ERRORS)
            tree.set_mate_correct(HIGH, LOW)
        try:
            if reads is not None:
                return tree.prep_reads(*pack_reads(reads), paired=True, want_reads=True, **PREP)
            return tree.prep_reads(*pack_quals(self.reads, self.quals), paired=True, want_reads=True, **PREP)
        finally:
            if steps:
                tree.set_adapters([])
                tree.set_mate_correct(0)
                tree.set_mate_overlap(0)


@pytest.fixture(scope="module")
def data(gpu):
    return Data()


# ---------------------------------------------------------------------------------------------------------------
# the gates
# ---------------------------------------------------------------------------------------------------------------
def refused(tree, getter):
    with pytest.raises(PfqError) as e:
        getattr(tree, getter)()
    assert e.value.code == PFQ_ERR_STATE, getter
    assert str(e.value) == f"libpfq error {PFQ_ERR_STATE}: {GATES[getter][0]}", getter


def answers(tree, getter):
    ms = np.atleast_1d(getattr(tree, getter)())
    assert len(ms) == GATES[getter][1] and all(math.isfinite(v) and v >= 0.0 for v in ms), (getter, ms)


def test_gates(data):
    main, screen = data.trees()
    try:
        for getter in GATES:
            refused(main, getter)
        assert main.inflate_text(data.gz)["n_good"] == 3              # two members of text and the end marker
        answers(main, "last_inflate_ms")
        assert main.deflate_bytes(data.text)["n_members"] == 1
        answers(main, "last_deflate_ms")
        assert main.parse_text(data.text, "fastq")["n_records"] == len(data.reads)
        main.query_text(1.0, want_hits=True)
        main.format_text()
        refused(main, "last_format_ms")                               # a format without PFQ_FMT_TIME=1
        main.set_option("PFQ_FMT_TIME", "1")
        main.format_text()
        main.set_option("PFQ_FMT_TIME", None)
        answers(main, "last_format_ms")
        assert data.prep(main, steps=False)["n_kept"] > 0             # reads, but none of the three steps
        answers(main, "last_prep_ms")
        for getter in ("last_adapters_ms", "last_overlap_ms", "last_corrections_ms", "last_deplete_ms"):
            refused(main, getter)
        assert data.prep(main)["n_kept"] > 0
        for getter in ("last_prep_ms", "last_adapters_ms", "last_overlap_ms", "last_corrections_ms"):
            answers(main, getter)
        assert main.prep_deplete(screen, 1.0, paired=True)["n_units"] > 0
        answers(main, "last_deplete_ms")
        assert data.prep(main, steps=False, reads=[])["n_reads"] == 0  # an empty prep clears nothing
        answers(main, "last_prep_ms")
        assert main.prep_deplete(screen, 1.0, paired=True)["n_units"] == 0
        answers(main, "last_deplete_ms")                              # nor does a depletion without units
        for getter in GATES:                                          # the screen was only ever queried
            refused(screen, getter)
    finally:
        main.close()
        screen.close()


# ---------------------------------------------------------------------------------------------------------------
# lifetimes
# ---------------------------------------------------------------------------------------------------------------
def cycle(data, close_screen_first, device=0):
    """Opens a tree and a screen, touches every resource the library makes lazily once, closes both; what the calls gave."""
    main, screen = data.trees(device)
    got = {}
    try:
        query_batch(main, data.reads, 1.0)
        got["host counts"] = counts_of(main).tolist()
        got["parsed"] = main.parse_text(data.text, "fastq")["n_records"]
        got["text rows"] = [x.tolist() for x in main.query_text(1.0, want_hits=True)]
        gz = main.format_text_gz(0, 16)                               # (whole result blocks only: four of 16 records)
        got["format"] = (gz["pos_gz"], gz["neg_gz"], gz["pos_records"], gz["neg_records"], gz["left"])
        got["inflated"] = main.inflate_text(data.gz)["good_text"]
        got["parsed inflated"] = main.parse_inflated("fastq")["n_records"]
        got["text"] = main.read_text(0, len(data.text))
        got["deflated"] = main.deflate_bytes(data.text, [1000])["gz"]
        prep = data.prep(main)
        got["prep"] = (prep["n_kept"], prep["bases_kept"], prep["kept"].tolist(), main.last_adapters()["n_found"],
                       main.last_overlap()["n_overlapped"], main.last_corrections()["n_bases"])
        dep = main.prep_deplete(screen, 1.0, paired=True)
        got["deplete"] = ([dep[k] for k in main.DEPLETE_TOTALS], dep["kept"].tolist())
        got["prep rows"] = [x.tolist() for x in main.query_prep(1.0, want_hits=True, paired=True)]
        main.profile_begin(4)
        main.query_packed(*pack_reads(data.reads), 1.0)
        got["profiled"] = int(main.profile_end().calls)
        grown = BloomTree.new(K, 0.01, GLEN, *SEEDS, device=device)
        try:
            grown.insert(data.genomes[0], "only")
            got["inserted"] = grown.node_filter(0).tobytes()
        finally:
            grown.close()
        main.set_option("PFQ_SIM_TIME", "1")
        got["similarity"] = main.similarity()["shared_bits"].tolist()
        assert main.last_similarity()[0] >= 0.0
        got["counts"] = (counts_of(main).tolist(), counts_of(screen).tolist())
    finally:
        for t in (screen, main) if close_screen_first else (main, screen):
            t.close()
    return got


@pytest.fixture(scope="module")
def first_cycle(data):
    got = cycle(data, False)
    # the cycle did something everywhere
    assert sum(got["host counts"]) > 0 and got["parsed"] == got["parsed inflated"] == len(data.reads) and got["inflated"] == len(data.text)
    assert got["text"] == data.text and got["format"][2] > 0 and len(got["deflated"]) > 0 and got["profiled"] == 1
    n_kept, _, _, n_adapters, n_overlapped, n_corrected = got["prep"]
    assert n_kept > 0 and n_adapters > 0 and n_overlapped > 0 and sum(n_corrected) > 0
    (n_units, units_removed, _, _, n_left, _), _ = got["deplete"]
    assert 0 < units_removed < n_units and n_left > 0 and sum(got["counts"][1]) > 0
    assert any(got["inserted"]) and len(got["similarity"]) == N_GENOMES
    return got


@pytest.mark.parametrize("close_screen_first", [True, False], ids=["screen closed first", "tree closed first"])
def test_cycles_repeat_the_first(data, first_cycle, close_screen_first):
    got = cycle(data, close_screen_first)
    assert got.keys() == first_cycle.keys()
    for k, v in first_cycle.items():
        assert got[k] == v, k


def test_closed_unused_and_after_a_parse_alone(data):
    main, screen = data.trees()
    screen.close()                                                    # nothing was ever made
    assert main.parse_text(data.text, "fastq")["n_records"] == len(data.reads)
    main.close()                                                      # the copy stream, the parse's events and its result block
    BloomTree.new(K, 0.01, GLEN, *SEEDS).close()


def test_a_tree_on_another_device(data, first_cycle):
    n = C.c_int(0)
    assert _ffi.lib().pfq_device_count(C.byref(n)) == 0
    if n.value < 2:
        pytest.skip("one device")
    main, screen = data.trees(device=1)
    try:
        assert hip().hipSetDevice(0) == 0
        query_batch(main, data.reads, 1.0)
        assert counts_of(main).tolist() == first_cycle["host counts"]
        assert main.parse_text(data.text, "fastq")["n_records"] == len(data.reads)
        data.prep(main)
        main.prep_deplete(screen, 1.0, paired=True)
        assert hip().hipSetDevice(0) == 0                             # device 0 is current when the trees of device 1 go
    finally:
        main.close()
        screen.close()
    assert cycle(data, True, device=1) == first_cycle


# ---------------------------------------------------------------------------------------------------------------
# the staging ring of pfq_tree_insert
# ---------------------------------------------------------------------------------------------------------------
def test_insert_staging_grows_and_wraps(gpu, tmp_path):
    """Four slots: 500, 4000, 1000 and 9000 bases fill them, then 6000 (slot 0 grows), 300 (slot 1 is large enough), 9000 (slot
    2 grows) and 9500 (slot 3, beyond what it asked for before, within what it was given or not) come round."""
    rng = np.random.default_rng(4)
    k, fpr, largest = 15, 0.01, 10000
    gt = BloomTree.new(k, fpr, largest, *SEEDS)
    try:
        ot = orc.OracleTree(k, gt.info().nbits, gt.info().num_hashes, *SEEDS, fpr, largest)
        for i, n in enumerate([500, 4000, 1000, 9000, 6000, 300, 9000, 9500]):
            g = _dna(rng, n)
            gt.insert(g, f"s{i}")
            orc.greedy_insert(ot, g, f"s{i}")
        _assert_same_tree(gt, ot, tmp_path, "staged")
    finally:
        gt.close()
