"""pfq_prep_reads / pfq_prep_query on the device against tests/prep_ref.py: begin, len, reason, kept, every total and the prepared
CSR exactly, over the parameter grid, over read lengths that cross every piece and group size of the kernels, over more reads
than one scan block and one grid trip hold, for pairs and for split blocks; then the classification of a prepared block against
query_packed of the same reads trimmed on the host."""
import ctypes as C
import itertools

import numpy as np
import pytest

import prep_ref
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_abund import same as same_abundance
from test_gpu_abund import strain_families
from test_gpu_build import SEEDS, _dna
from test_gpu_tax import random_taxonomy

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 4, 200003
PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -4, -6
# mirrors of pfq_kernels.h / pfq_prep.hip: a lane takes 16 aligned bytes; groups of 16 lanes take reads up to PREP_SHORT_MAX bases
# in pieces of 256 bytes, a wave up to PREP_WAVE_MAX in pieces of 1024, a block the rest in pieces of 4096; every kernel runs at
# most PREP_GRID blocks, which look at 256 reads a trip; launch_scan_u32 scans 4096 items a block
LANE_BYTES, PIECES = 16, (256, 1024, 4096)
PREP_SHORT_MAX, PREP_WAVE_MAX = 512, 4096
PREP_GRID, TRIP_READS, SCAN_ITEMS = 1024, 1024 * 256, 4096

QS, WS, PS = (0, 2, 20, 41), (1, 4, 50), (0, 1, 10)
MIN_LENGTHS, MAX_NS, CS = (0, 1, 21, 50), (0, 3, None), (0, 30, 100)
QUAL_ALPHABET = np.frombuffer(b"!#%+5?IJK", dtype=np.uint8)       # 0 2 4 10 20 30 40 41 42: sums land exactly on Q w
GOOD_ALPHABET = np.frombuffer(b"5?IJK", dtype=np.uint8)
SHORT_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 49, 50, 51, 63, 64, 65]
LONG_LENGTHS = [240, 241, 242, 255, 256, 257, 511, 512, 513, 700, 1023, 1024, 1025, 4095, 4096, 4097, 5000, 9000]
TOTALS = ("n_reads", "n_kept", "bases_in", "bases_kept", "n_trimmed", "n_reason")


def make_read(rng, L, kind):
    """(bases, qualities) of length L: `kind` picks the tail and the qualities."""
    s = bytearray(_dna(rng, L))
    if kind.startswith("tail") and L:                                 # a homopolymer tail of exactly that length, if it fits
        t = min(int(kind[4:]), L)
        if L > t:
            s[L - t - 1] = ord("A")
        s[L - t:] = b"G" * t
    elif kind == "mixed" and L:                                       # mixed case, an N tail
        t = int(rng.integers(1, min(L, 12) + 1))
        s[L - t:] = bytes(rng.choice(np.frombuffer(b"nN", dtype=np.uint8), t).astype(np.uint8))
        for j in rng.integers(0, L, L // 3).tolist():
            s[j] |= 0x20
    elif kind == "homopolymer":
        s[:] = b"T" * L
    elif kind == "ns" and L:
        for j in rng.integers(0, L, max(1, L // 8)).tolist():
            s[j] = ord("N")
    if kind == "allbad":
        q = b"#" * L
    elif kind == "deep":                                              # good for three quarters, then worthless
        q = b"K" * (3 * L // 4) + b"!" * (L - 3 * L // 4)
    elif kind == "allgood":
        q = b"K" * L
    else:                                                             # a few bad leading bases, a good stretch, then anything
        lead = int(rng.integers(0, 4)) if L > 8 else 0
        good = int(rng.integers(0, L - lead + 1))
        q = (b"#" * lead + bytes(rng.choice(GOOD_ALPHABET, good).astype(np.uint8)) +
             bytes(rng.choice(QUAL_ALPHABET, L - lead - good).astype(np.uint8)))
    return bytes(s), q


KINDS = ["plain", "plain", "allbad", "allgood", "tail0", "tail1", "tail2", "tail9", "tail10", "tail11", "mixed", "homopolymer", "ns"]


def make_block(rng, lengths, kinds=KINDS, no_qual_every=0):
    reads, quals = [], []
    for i, (L, kind) in enumerate(itertools.product(lengths, kinds)):
        s, q = make_read(rng, L, kind)
        reads.append(s)
        quals.append(None if no_qual_every and i % no_qual_every == no_qual_every - 1 else q)
    order = rng.permutation(len(reads)).tolist()
    return [reads[i] for i in order], [quals[i] for i in order]


def pack_quals(reads, quals):
    """The quality buffer aligned to the bases (a read without qualities: filler that must not be looked at) and has_qual."""
    seq, off = pack_reads(reads)
    qual, _ = pack_reads([q if q is not None else b"~" * len(r) for r, q in zip(reads, quals)])
    return seq, off, qual, np.array([q is not None for q in quals], dtype=np.uint8)


def counts_of(gt):
    return np.array([c for _, c in gt.get_leaf_counts()], dtype=np.int64)


class Case:
    def __init__(self):
        rng = self.rng = np.random.default_rng(5150)
        self.genomes = strain_families(rng, 4, 3, 2000, 0.006, 4)
        self.ids = [f"P{i:02d}" for i in range(16)]
        self.gt = BloomTree.build_balanced(self.genomes, self.ids, K, NBITS, H, *SEEDS)
        self.short = make_block(rng, SHORT_LENGTHS, no_qual_every=11)
        self.long = make_block(rng, LONG_LENGTHS, kinds=["plain", "deep", "allgood", "tail10", "mixed", "homopolymer"], no_qual_every=13)

    def check(self, reads, quals, paired=False, want_reads=True, packed=None, **params):
        """One device call against the reference: everything it reports and the CSR it prepared."""
        want = prep_ref.prep_block(reads, quals, paired=paired, **params)
        if quals is None:
            (seq, off), qual, hq = pack_reads(reads), None, None
        else:
            seq, off, qual, hq = packed or pack_quals(reads, quals)
        got = self.gt.prep_reads(seq, off, qual, hq, paired=paired, want_reads=want_reads, **params)
        tag = (len(reads), paired, params)
        for k in TOTALS:
            assert got[k] == want[k], (tag, k, got[k], want[k])
        if want_reads:
            for k in ("begin", "len", "reason", "kept"):
                g, w = got[k], np.array(want[k], dtype=np.uint32)
                assert g.dtype == np.uint32 and g.shape == w.shape, (tag, k)
                bad = np.flatnonzero(g != w)
                assert bad.size == 0, (tag, k, bad[:8], g[bad[:8]], w[bad[:8]], [len(reads[i]) for i in bad[:8]] if k != "kept" else None)
        else:
            assert all(got[k] is None for k in ("begin", "len", "reason", "kept")), tag
        cseq, coff = self.gt.prep_csr()
        assert coff.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in want["kept_reads"]], dtype=np.int64)]).tolist(), tag
        assert cseq.tobytes() == b"".join(want["kept_reads"]), tag
        return want


@pytest.fixture(scope="module")
def case(gpu):
    x = Case()
    yield x
    x.gt.close()


@pytest.mark.parametrize("Q", QS)
def test_parameter_grid_on_short_reads(case, Q):
    reads, quals = case.short
    assert {len(r) for r in reads} >= {0, 1, 2} | {W + d for W in WS for d in (-1, 0, 1)} | {LANE_BYTES + d for d in (-1, 0, 1)}
    assert any(q is None for q in quals) and any(q is not None for q in quals)
    packed = pack_quals(reads, quals)
    reasons = set()
    for n, (W, P, ml, mn, Cx) in enumerate(itertools.product(WS, PS, MIN_LENGTHS, MAX_NS, CS)):
        want = case.check(reads, quals, packed=packed, want_reads=n % 5 != 4, trim_quality=Q, trim_window=W, poly_x=P, min_length=ml, max_n=mn,
                          min_complexity=Cx)
        reasons |= set(want["reason"])
    assert reasons == {0, 1, 2, 3}


@pytest.mark.parametrize("Q", QS)
def test_lengths_round_every_piece_and_group(case, Q):
    reads, quals = case.long
    lengths = {len(r) for r in reads}
    for edge in (*PIECES, PIECES[0] - LANE_BYTES + 1, PREP_SHORT_MAX, PREP_WAVE_MAX):     # 241: the longest read whose every alignment is one piece
        assert {edge - 1, edge, edge + 1} <= lengths, edge
    assert {255, 256, 257, 700, 5000} <= lengths and max(lengths) > 2 * PIECES[2]
    packed = pack_quals(reads, quals)
    cut_deep = False
    filters = ((0, None, 0), (21, 3, 30), (50, 0, 100))
    for n, (W, P) in enumerate(itertools.product(WS, PS)):
        for ml, mn, Cx in (filters if (W, P) == (4, 10) else filters[n % 3:n % 3 + 1]):
            want = case.check(reads, quals, packed=packed, trim_quality=Q, trim_window=W, poly_x=P, min_length=ml, max_n=mn, min_complexity=Cx)
            cut_deep |= any(PIECES[2] < l < len(r) for l, r in zip(want["len"], reads))
    assert cut_deep or Q == 0                                         # some cut lies beyond a block's first piece


def test_without_qualities(case):
    reads, quals = case.short
    params = dict(trim_quality=20, trim_window=4, poly_x=10, min_length=5, max_n=3, min_complexity=30)
    none = case.check(reads, None, **params)
    assert none["begin"] == [0] * len(reads)                          # the quality step is skipped, the others apply
    assert none["n_reason"]["complexity"] > 0 and none["n_trimmed"] > 0
    full = [q if q is not None else b"I" * len(r) for r, q in zip(reads, quals)]
    seq, off, qual, _ = pack_quals(reads, full)
    want = prep_ref.prep_block(reads, full, **params)
    got = case.gt.prep_reads(seq, off, qual, None, want_reads=True, **params)           # has_qual None: every read has qualities
    assert got["len"].tolist() == want["len"] and got["reason"].tolist() == want["reason"] and any(want["begin"])
    assert {k: got[k] for k in TOTALS} == {k: want[k] for k in TOTALS}


def test_more_reads_than_a_scan_block_and_a_grid_trip(case):
    """Copies of the short cases (the reference works a distinct read out once), most of them kept, and behind the first trip of
    every kernel's grid some reads for the wave and the block builds."""
    rng = np.random.default_rng(99)
    base_r, base_q = make_block(rng, [30, 31, 33, 40, 47, 64, 65], kinds=["allgood"] * 6 + ["plain", "tail10", "tail11", "allbad"])
    long_r, long_q = make_block(rng, [600, 4200], kinds=["plain", "allgood"])
    idx = rng.integers(0, len(base_r), TRIP_READS + 12 * SCAN_ITEMS + 77).tolist()
    reads, quals = [base_r[i] for i in idx], [base_q[i] for i in idx]
    tail = rng.integers(0, len(long_r), 40).tolist()
    for j, i in enumerate(tail):
        at = len(reads) - 1 - 50 * j
        reads[at], quals[at] = long_r[i], long_q[i]
    assert len(reads) > TRIP_READS > SCAN_ITEMS and len(reads) - 50 * 40 > TRIP_READS
    want = case.check(reads, quals, trim_quality=20, trim_window=4, poly_x=10, min_length=8)
    assert want["n_kept"] > TRIP_READS and want["n_reason"]["short"] > SCAN_ITEMS and want["n_trimmed"] > SCAN_ITEMS
    assert sum(1 for i in want["kept"] if i > TRIP_READS and len(reads[i]) > PREP_WAVE_MAX) > 0
    assert sum(1 for i in want["kept"] if i > TRIP_READS and PREP_SHORT_MAX < len(reads[i]) <= PREP_WAVE_MAX) > 0
    pairs = case.check(reads[:-1] if len(reads) & 1 else reads, quals[:-1] if len(reads) & 1 else quals, paired=True, want_reads=False,
                       trim_quality=20, trim_window=4, poly_x=10, min_length=8)
    assert pairs["n_kept"] > SCAN_ITEMS and pairs["n_reason"]["mate"] > SCAN_ITEMS


def test_pairs(case):
    good, short, ns, low = b"ACGTTGCAACGTAGGCTAGCTAGGATC", b"ACGTA", b"ACGTNNNNACGTACGATCGATTAGC", b"AAAAAAAAAAAAAAAAAAAAAAAAAC"
    params = dict(min_length=10, max_n=2, min_complexity=30)
    assert [prep_ref.prep_read(s, None, **params)[2] for s in (good, short, ns, low)] == [0, 1, 2, 3]
    reads = [m for a in (good, short, ns, low) for b in (good, short, ns, low) for m in (a, b)]
    want = case.check(reads, None, paired=True, **params)
    assert want["kept"] == [0, 1] and want["n_reason"] == {"kept": 2, "short": 8, "n": 8, "complexity": 8, "mate": 6}
    assert len(case.gt.query_prep(1.0, want_hits=True, paired=True)[0]) == 2             # one fragment
    case.check(reads, None, paired=False, **params)
    with pytest.raises(PfqError) as e:
        case.gt.query_prep(1.0, paired=True)                          # PFQ_PAIRED on a block prepared without PFQ_PREP_PAIRED
    assert e.value.code == PFQ_ERR_ARG
    with pytest.raises(PfqError) as e:
        case.gt.prep_reads(*pack_reads(reads[:3]), paired=True)
    assert e.value.code == PFQ_ERR_ARG


def test_split_blocks_equal_one_block(case):
    reads, quals = case.short[0] + case.long[0], case.short[1] + case.long[1]
    if len(reads) & 1:
        reads, quals = reads[:-1], quals[:-1]
    params = dict(trim_quality=20, trim_window=4, poly_x=10, min_length=21, max_n=3, min_complexity=30)
    n = len(reads)
    cuts = [0, 2 * (n // 6), 2 * (n // 4) + 2, n]
    for paired in (False, True):
        whole = case.check(reads, quals, paired=paired, **params)
        parts = [case.check(reads[a:b], quals[a:b], paired=paired, **params) for a, b in zip(cuts, cuts[1:])]
        for k in ("begin", "len", "reason", "kept_reads"):
            assert sum((p[k] for p in parts), []) == whole[k], (paired, k)
        assert sum(([a + i for i in p["kept"]] for a, p in zip(cuts, parts)), []) == whole["kept"]
        assert prep_ref.add_totals(parts) == {k: whole[k] for k in TOTALS}


@pytest.fixture(scope="module")
def tailed(case):
    """Reads sampled from the tree's genomes with random tails appended and low qualities over those tails; some reads too short
    to keep, some of nothing but tail."""
    rng, g = case.rng, case.genomes
    reads, quals = [], []
    for a, n, t in zip(rng.integers(0, 1700, 400).tolist(), rng.integers(40, 280, 400).tolist(), rng.integers(25, 60, 400).tolist()):
        reads.append(g[int(rng.integers(16))][a:a + n] + _dna(rng, t))
        quals.append(b"I" * n + b"#" * t)
    for n in (0, 5, 20, 30):
        reads.append(_dna(rng, n) + _dna(rng, 30))
        quals.append(b"I" * n + b"#" * 30)
    order = rng.permutation(len(reads)).tolist()
    return [reads[i] for i in order], [quals[i] for i in order]


TRIM = dict(trim_quality=20, trim_window=4, min_length=K)


@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_classification_equals_query_packed_of_the_trimmed_reads(case, tailed, thr):
    gt = case.gt
    reads, quals = tailed
    want = prep_ref.prep_block(reads, quals, **TRIM)
    assert 0 < want["n_reason"]["short"] < 10 and want["n_trimmed"] == want["n_kept"]
    gt.reset_counts()
    raw_off, raw_leaves = gt.query_packed(*pack_reads(reads), thr, want_hits=True)
    gt.reset_counts()
    want_off, want_leaves, want_scores = gt.query_packed(*pack_reads(want["kept_reads"]), thr, want_hits=True, want_scores=True)
    want_counts = counts_of(gt)
    if thr == 1.0:                                                    # the feature doing its job: the tails hide every read, trimming finds them
        assert raw_leaves.size == 0 and int((np.diff(want_off.astype(np.int64)) > 0).sum()) >= 390
    gt.reset_counts()
    case.check(reads, quals, **TRIM)
    assert counts_of(gt).sum() == 0                                   # preparing changes no counter
    gt.query_packed(*pack_reads(reads[:7]), thr)                      # a query call between prep and query disturbs nothing
    between = counts_of(gt)
    off, leaves, scores = gt.query_prep(thr, want_hits=True, want_scores=True)
    assert off.tolist() == want_off.tolist() and leaves.tolist() == want_leaves.tolist() and scores.tolist() == want_scores.tolist()
    assert (counts_of(gt) - between).tolist() == want_counts.tolist()
    assert gt.last_stats().n_reads == want["n_kept"]
    gt.query_prep(thr)                                                # again on the same block: the increase doubles
    assert (counts_of(gt) - between).tolist() == (2 * want_counts).tolist()
    gt.reset_counts()


def test_paired_classification_with_taxonomy_and_abundance(case, tailed):
    gt = case.gt
    reads, quals = tailed
    want = prep_ref.prep_block(reads, quals, paired=True, **TRIM)
    assert want["n_reason"]["mate"] > 0 and want["n_kept"] % 2 == 0
    tax = random_taxonomy(17, 16)

    def run(query):
        gt.reset_counts()
        gt.set_taxonomy(*tax)
        res = query()
        return res, counts_of(gt).tolist(), gt.last_taxa().copy(), gt.taxon_counts(), gt.abundance()

    kw = dict(want_hits=True, want_scores=True, paired=True, taxa=True, abundance=True)
    ref = run(lambda: gt.query_packed(*pack_reads(want["kept_reads"]), 0.5, **kw))
    case.check(reads, quals, paired=True, **TRIM)
    got = run(lambda: gt.query_prep(0.5, **kw))
    assert len(ref[0][0]) == want["n_kept"] // 2 + 1 and ref[0][1].size > 0
    assert all(np.array_equal(a, b) for a, b in zip(got[0], ref[0])) and got[1] == ref[1]
    assert np.array_equal(got[2], ref[2]) and all(np.array_equal(a, b) for a, b in zip(got[3], ref[3]))
    same_abundance(got[4], ref[4], "query_prep")
    gt.reset_counts()


def test_state_and_arguments(case):
    gt, L = case.gt, _ffi.lib()
    fresh = BloomTree.build_balanced(case.genomes[:2], case.ids[:2], K, NBITS, H, *SEEDS)
    with pytest.raises(PfqError) as e:
        fresh.query_prep(1.0)
    assert e.value.code == PFQ_ERR_STATE
    seq, off = pack_reads([b"ACGTACGTAC", b"ACGT"])
    for bad in (dict(trim_quality=94), dict(trim_window=0), dict(trim_window=1025), dict(min_complexity=101)):
        with pytest.raises(PfqError) as e:
            fresh.prep_reads(seq, off, **bad)
        assert e.value.code == PFQ_ERR_ARG, bad
    par, out = _ffi.PrepParams(0, 4, 0, 0, 0xFFFFFFFF, 0, 0), _ffi.Prep()
    assert L.pfq_prep_reads(None, seq.ctypes.data, None, off.ctypes.data, None, 2, C.byref(par), C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_prep_reads(fresh._h, None, None, off.ctypes.data, None, 2, C.byref(par), C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_prep_reads(fresh._h, seq.ctypes.data, None, None, None, 2, C.byref(par), C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_prep_reads(fresh._h, seq.ctypes.data, None, off.ctypes.data, None, 2, None, C.byref(out)) == PFQ_ERR_ARG
    assert L.pfq_prep_reads(fresh._h, seq.ctypes.data, None, off.ctypes.data, None, 2, C.byref(par), None) == PFQ_ERR_ARG
    par.flags = 4
    assert L.pfq_prep_reads(fresh._h, seq.ctypes.data, None, off.ctypes.data, None, 2, C.byref(par), C.byref(out)) == PFQ_ERR_ARG
    with pytest.raises(PfqError) as e:
        fresh.query_prep(1.0)                                         # refused calls prepared nothing
    assert e.value.code == PFQ_ERR_STATE
    before = fresh.info().device_bytes
    assert fresh.prep_reads(*pack_reads([b"ACGT" * (1 << 18)]), poly_x=3)["bases_kept"] == 1 << 20
    assert fresh.info().device_bytes >= before + (2 << 20)            # the new buffers are counted
    fresh.close()
    # no reads; reads that are all dropped: nothing kept, the query is a no-op
    for reads in ([], [b"ACGT", b"AC", b""]):
        got = gt.prep_reads(*pack_reads(reads), min_length=5, want_reads=True)
        assert (got["n_reads"], got["n_kept"], got["bases_kept"], got["kept"].size) == (len(reads), 0, 0, 0)
        assert got["reason"].tolist() == [1] * len(reads) and got["n_reason"]["short"] == len(reads)
        cseq, coff = gt.prep_csr()
        assert cseq.size == 0 and coff.tolist() == [0]
        gt.reset_counts()
        off, leaves = gt.query_prep(1.0, want_hits=True)
        assert off.tolist() == [0] and leaves.size == 0 and counts_of(gt).sum() == 0
