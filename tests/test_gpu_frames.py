"""pfq_query_frames on the device against tests/frames_ref.py over the oracle: offsets, every field of every segment, the number
of frames and the leaf counters' increase, exactly — everything is integer work."""
import copy

import numpy as np
import pytest

import frames_ref as fr
from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, pack_reads
from test_gpu_abund import strain_families
from test_gpu_build import SEEDS, _dna
from test_gpu_lca import csr_of, oracle_sets

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 4, 200003
PFQ_ERR_ARG = -1
GRID = [(200, 100), (150, 50), (K, 1), (84, 84), (85, 17), (301, 7)]


def counts_of(gt):
    return [c for _, c in gt.get_leaf_counts()]


class Case:
    """16 leaves: 4 families of 3 strains and 4 unrelated genomes of 2000 bases.  The sequences: planted inserts, chimeras of two
    genomes, an insert from a strain family, one genome planted twice with a gap wider than any frame, a whole genome, unrelated
    sequences; seqs(F, S) adds the lengths where the frame rule changes."""

    def __init__(self):
        rng = np.random.default_rng(7741)
        self.rng = rng
        g = self.genomes = strain_families(rng, 4, 3, 2000, 0.006, 4)
        self.ids = [f"F{i:02d}" for i in range(16)]
        self.ot = orc.build_balanced_tree(g, self.ids, K, NBITS, H, *SEEDS)
        self.gt = BloomTree.build_balanced(g, self.ids, K, NBITS, H, *SEEDS)
        self.ref = fr.Ref(self.ot)
        r = lambda n: _dna(rng, n)
        self.long = [
            r(1000) + g[12][200:1200] + r(1000),                                  # a planted insert
            g[13][0:1500] + g[14][300:1800],                                      # chimeras
            g[0][0:1000] + orc.revcomp(g[15][0:1000]),
            r(800) + g[3][100:1300] + r(700),                                     # from a family: several leaves a frame
            r(500) + g[12][100:700] + r(900) + g[12][1000:1600] + r(400),         # twice, the gap wider than any frame
            g[13],                                                                # a whole genome: one long segment
            g[6] + r(37) + g[6][:2000],                                           # 4037 bases, odd
            r(1500), r(300), r(5999),                                             # unrelated
        ]
        self.short = [g[14][500:500 + n] for n in (0, 4, K - 1, K, K + 1, 64, 84, 85, 130, 217)] + [r(90), r(K), g[0][100:420]]
        assert all(len(x) <= 6000 for x in self.long)
        self._want = {}

    def seqs(self, F, S):
        if (F, S) == (K, 1):
            return self.short
        edge = [self.genomes[14][300:300 + n] for n in (0, 4, K - 1, K, K + 1, F - 1, F, F + 1, F + S, F + S + 1)]
        return self.long + edge + self.short[-3:]

    def want(self, F, S, thr, seqs=None):
        """The reference, computed once per case; nothing changes it."""
        key = (F, S, thr)
        if seqs is not None:
            return self.ref.query(seqs, F, S, thr)
        if key not in self._want:
            self._want[key] = self.ref.query(self.seqs(F, S), F, S, thr)
        return self._want[key]


@pytest.fixture(scope="module")
def case(gpu):
    x = Case()
    assert len(x.seqs(200, 100)) <= 60
    yield x
    x.gt.close()


def run(gt, seqs, F, S, thr):
    """(per-sequence tuples, n_frames, the counters' increase) of one call."""
    before = counts_of(gt)
    seq, off = pack_reads(seqs)
    offs, segs = gt.query_frames(seq, off, F, S, thr)
    assert offs.dtype == np.uint64 and len(offs) == len(seqs) + 1 and offs[0] == 0 and segs.dtype.names == fr.FIELDS
    assert int(offs[-1]) == len(segs)
    per = [fr.as_tuples(segs[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])]
    return per, gt.last_n_frames, [b - a for a, b in zip(before, counts_of(gt))]


def same(got, want, tag):
    per, n_frames, delta = got
    wper, wframes, wcounts, _ = want
    for i, (a, b) in enumerate(zip(per, wper)):
        assert a == fr.as_tuples(b), (tag, "sequence", i, a, fr.as_tuples(b))
    assert len(per) == len(wper) and n_frames == wframes and delta == wcounts, (tag, n_frames, wframes, delta, wcounts)


# ---------------------------------------------------------------------------------------------------------------
# 1. against the reference
# ---------------------------------------------------------------------------------------------------------------
def test_the_case_is_what_it_says(case):
    per, _, counts, sets = case.want(200, 100, 1.0)
    flat = [s for segs in per for s in segs]
    assert any(s["n_frames"] >= 5 for s in flat)
    assert any(len(segs) != len({s["leaf"] for s in segs}) for segs in per)      # two segments of one leaf in a sequence
    assert sum(1 for segs in per if not segs) >= 3                                # sequences with none
    assert any(s["longest_run"] >= 130 for s in flat)                             # a run across windows of 64, whatever its start
    per5, _, _, sets5 = case.want(200, 100, 0.5)
    flat5 = [s for segs in per5 for s in segs]                                    # (below threshold 1 a frame passes with misses)
    assert any(s["match_begin"] > s["begin"] for s in flat5) and any(s["match_end"] < s["end"] for s in flat5)
    assert any(0 < s["matched"] < s["kmers"] for s in flat5)
    assert any(3 <= len(h) < 16 for row in sets5 for h in row)                    # a frame row of several leaves
    assert any(len(h) == 16 for row in sets for h in row)                         # and the every-leaf rows of the short ones


@pytest.mark.parametrize("thr", [1.0, 0.5])
@pytest.mark.parametrize("F,S", GRID)
def test_against_reference(case, F, S, thr):
    same(run(case.gt, case.seqs(F, S), F, S, thr), case.want(F, S, thr), (F, S, thr))


def test_threshold_zero(case):
    want = case.want(150, 50, 0.0)
    assert all(len(segs) == 16 and all(s["n_frames"] == len(row) for s in segs) for segs, row in zip(want[0], want[3]))
    same(run(case.gt, case.seqs(150, 50), 150, 50, 0.0), want, "theta 0")


# ---------------------------------------------------------------------------------------------------------------
# 2. nothing depends on the cut into calls, the path or a knob
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_split_and_reversed(case, thr):
    F, S, gt, seqs = 200, 100, case.gt, case.seqs(200, 100)
    want = case.want(F, S, thr)
    n = len(seqs)
    per, frames, delta = [], 0, [0] * 16
    for a, b in ((0, n // 5), (n // 5, n // 2), (n // 2, n)):
        p, f, d = run(gt, seqs[a:b], F, S, thr)
        per, frames, delta = per + p, frames + f, [x + y for x, y in zip(delta, d)]
    same((per, frames, delta), want, "three calls")
    p, f, d = run(gt, seqs[::-1], F, S, thr)
    same((p[::-1], f, d), want, "reversed")


@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_paths(case, thr):
    gt = case.gt
    try:
        for path in (0, 1):
            gt.set_path(path)
            same(run(gt, case.seqs(150, 50), 150, 50, thr), case.want(150, 50, thr), ("path", path))
            assert gt.last_stats().path == path and gt.last_stats().n_reads == case.want(150, 50, thr)[1]
    finally:
        gt.set_path(-1)


@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_piece_sizes(case, thr):
    gt = case.gt
    try:
        for piece in ("64", "128", None):
            gt.set_option("PFQ_FRAME_PIECE", piece)
            same(run(gt, case.seqs(301, 7), 301, 7, thr), case.want(301, 7, thr), ("piece", piece))
        for bad in ("0", "100", "-64"):
            with pytest.raises(PfqError) as e:
                gt.set_option("PFQ_FRAME_PIECE", bad)
            assert e.value.code == PFQ_ERR_ARG
    finally:
        gt.set_option("PFQ_FRAME_PIECE", None)


def test_inner_retry(case):
    gt = case.gt
    try:
        gt.set_option("PFQ_HIT_SLOTS", "8")
        same(run(gt, case.seqs(200, 100), 200, 100, 0.5), case.want(200, 100, 0.5), "hit slots")
        assert gt.last_capacity()["attempts"] == 2
    finally:
        gt.set_option("PFQ_HIT_SLOTS", None)


# ---------------------------------------------------------------------------------------------------------------
# 3. beside the per-read calls
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_one_frame_equals_reads(case, thr):
    gt, seqs = case.gt, case.seqs(200, 100)
    seq, off = pack_reads(seqs)
    c0 = counts_of(gt)
    roffs, rleaves = gt.query_packed(seq, off, thr, want_hits=True)
    c1 = counts_of(gt)
    per, frames, delta = run(gt, seqs, 10000, 5000, thr)
    assert frames == len(seqs) and delta == [b - a for a, b in zip(c0, c1)]
    assert [[s[0] for s in segs] for segs in per] == [rleaves[int(a):int(b)].tolist() for a, b in zip(roffs[:-1], roffs[1:])]
    assert all(s[1:5] == (0, 1, 0, len(x)) for segs, x in zip(per, seqs) for s in segs)


def test_plain_queries_around(case):
    gt, seqs = case.gt, case.seqs(200, 100)
    seq, off = pack_reads(seqs)
    before = gt.query_packed(seq, off, 0.5, want_hits=True, want_scores=True)
    run(gt, seqs, 200, 100, 0.5)
    with pytest.raises(PfqError) as e:
        gt.last_hit_scores()
    assert e.value.code == PFQ_ERR_ARG
    with pytest.raises(PfqError) as e:
        gt.last_lca()
    assert e.value.code == PFQ_ERR_ARG
    c1 = counts_of(gt)
    after = gt.query_packed(seq, off, 0.5, want_hits=True, want_scores=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    woff, wleaves = csr_of(oracle_sets(case.ot, seqs, 0.5))
    assert np.array_equal(after[0], woff) and np.array_equal(after[1], wleaves)
    assert [b - a for a, b in zip(c1, counts_of(gt))] == np.bincount(wleaves, minlength=16).tolist()


# ---------------------------------------------------------------------------------------------------------------
# 4. guard columns and subtree shards
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_guard_column(case, thr, tmp_path):
    ot = copy.deepcopy(case.ot)
    internal = [v for v in range(ot.n_nodes) if not ot.is_leaf(v)]
    ot.bits[ot.filter_of[internal[1]]][::2] = 0                 # an internal filter that lost bits: no superset of its children
    d = str(tmp_path / "db")
    fmt.write_db(ot, d)
    gt = BloomTree.load(d)
    try:
        assert gt.info().superset_verified == 0
        seqs = case.seqs(200, 100)
        want = fr.Ref(ot).query(seqs, 200, 100, thr)
        assert want[2] != case.want(200, 100, thr)[2]           # (the guard decides something)
        same(run(gt, seqs, 200, 100, thr), want, ("guard", thr))
    finally:
        gt.close()


def test_subtree_shards(case, tmp_path):
    d = str(tmp_path / "db")
    case.gt.save(d)
    F, S, thr = 150, 50, 0.5
    seqs = case.seqs(F, S)
    wper, wframes, wcounts, _ = case.want(F, S, thr)
    assert BloomTree.shard_count(d, 1) == 2
    first = 0
    for index in range(2):
        st = BloomTree.load_subtree(d, 1, index)
        try:
            info = st.info()
            lo, hi = int(info.shard_first_leaf), int(info.shard_first_leaf) + int(info.n_leaves)
            assert lo == first and int(info.tree_leaves) == 16
            first = hi
            per, frames, delta = run(st, seqs, F, S, thr)
            local = [[dict(s, leaf=s["leaf"] - lo) for s in segs if lo <= s["leaf"] < hi] for segs in wper]
            same((per, frames, delta), (local, wframes, wcounts[lo:hi], None), ("shard", index))
        finally:
            st.close()
    assert first == 16


# ---------------------------------------------------------------------------------------------------------------
# 5. arguments
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_empty_call(case):
    import ctypes as C
    from phagefilter_amd import _ffi
    gt = case.gt
    seq, off = pack_reads([case.long[0]])
    c0 = counts_of(gt)
    for F, S in ((K - 1, 1), (0, 0), (100, 0), (100, 101), (5, 5)):
        with pytest.raises(PfqError) as e:
            gt.query_frames(seq, off, F, S, 1.0)
        assert e.value.code == PFQ_ERR_ARG, (F, S)
    out = _ffi.Segments()
    for flags in (1, 4, 16, 64, 128, 256):
        rc = _ffi.lib().pfq_query_frames(gt._h, seq.ctypes.data, off.ctypes.data, 1, 100, 50, 1.0, flags, C.byref(out))
        assert rc == PFQ_ERR_ARG, flags
    assert _ffi.lib().pfq_query_frames(gt._h, seq.ctypes.data, off.ctypes.data, 1, 100, 50, 1.0, 0, None) == PFQ_ERR_ARG
    assert counts_of(gt) == c0
    offs, segs = gt.query_frames(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 100, 50, 1.0)
    assert offs.tolist() == [0] and len(segs) == 0 and gt.last_n_frames == 0 and counts_of(gt) == c0
