"""The tail of a query call: how the hit CSR, the scores, the LCAs, the leaf and clade counters and the abundance log come
out of one call, for single reads and for fragments (PFQ_PAIRED, either / both), under every combination of the result flags,
on both query paths, for a mixed block, a block without a single hit and the empty block.

Nothing expected here comes from the library.  The reads' sets are the oracle's (oracle_sets), fragments are combined from
the mates' sets (combine), scores are the oracle's k-mer by k-mer counts (expected_scores / pair_scores), LCAs are found
naively on the oracle tree (Clades) and the abundance log is the restatement of tests/abund_ref.py.  Every call is also held
against the same call with PFQ_WANT_HITS alone."""
import numpy as np
import pytest

import abund_ref
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, pack_reads
from test_gpu_abund import same
from test_gpu_build import SEEDS, _dna, _mutate
from test_gpu_lca import NO, Clades, Device, best_sets, csr_of, oracle_sets, pair_scores
from test_gpu_paired import combine
from test_gpu_scores import Contains, expected_scores

pytestmark = pytest.mark.gpu

K, NBITS, H = 21, 50021, 6
N_LEAVES = 8
THR = 0.7
UNITS = ("reads", "either", "both")
# (name, scores, lca, abundance, hits)
FLAG_SETS = (
    ("hits", False, None, False, True),
    ("hits+scores", True, None, False, True),
    ("hits+lca", False, "all", False, True),
    ("hits+scores+best", True, "best", False, True),
    ("lca alone", False, "all", False, False),
    ("hits+abundance", False, None, True, True),
    ("everything", True, "best", True, True),
)
EVERYTHING = FLAG_SETS[-1]


class Expected:
    """What one block gives in one unit mode at one threshold, from the oracle alone."""

    def __init__(self, fx, reads, units, thr):
        mates = oracle_sets(fx.ot, reads, thr) if reads else []
        self.sets = mates if units == "reads" else combine(mates, units)
        self.n = len(self.sets)
        self.offs, self.leaves = csr_of(self.sets)
        if units == "reads":
            self.scores = expected_scores(fx.ot, reads, self.offs, self.leaves, fx.contains)
        else:
            self.scores = pair_scores(fx.ot, reads, self.sets, fx.contains)
        self.lca = {"all": fx.cm.expected(self.sets), "best": fx.cm.expected(best_sets(self.sets, self.scores))}
        self.leaf_counts = [sum(c in s for s in self.sets) for c in range(N_LEAVES)]
        self.rows = [sorted(s) for s in self.sets]


class Fixture:
    """8 leaves in two families of 4: every genome is its family's base a few substitutions apart (reads from there are
    shared with the sisters) followed by a stretch of its own (reads from there hit one leaf)."""

    def __init__(self, device=True):
        rng = np.random.default_rng(417)
        self.genomes = []
        for _ in range(2):
            base = _dna(rng, 1200)
            self.genomes += [_mutate(rng, base, 5) + _dna(rng, 500) for _ in range(4)]
        self.ids = [f"R{i}" for i in range(N_LEAVES)]
        self.ot = orc.build_balanced_tree(self.genomes, self.ids, K, NBITS, H, *SEEDS)
        self.gt = BloomTree.build_balanced(self.genomes, self.ids, K, NBITS, H, *SEEDS) if device else None
        self.cm = Clades(self.ot)
        self.contains = Contains(self.ot)
        self.blocks = {"a": self.mixed(rng), "b": [_dna(rng, 100) for _ in range(40)], "c": []}
        self.blocks["aa"] = self.blocks["a"] + self.blocks["a"]
        self._exp = {}

    def mixed(self, rng):
        """Fragments (m1, m2); read as single reads the block holds the same mates one by one.  Mates: from the shared part
        of every genome, from its own stretch, foreign, empty, of k - 1 and of k bases."""
        g = self.genomes

        def shared(i):
            o = int(rng.integers(0, 1100))
            r = g[i][o:o + 100]
            return orc.revcomp(r) if rng.random() < 0.5 else r

        def own(i):
            o = int(rng.integers(1200, 1600))
            return g[i][o:o + 100]

        def foreign():
            return _dna(rng, 100)

        pairs = []
        for i in range(N_LEAVES):
            pairs += [(shared(i), shared(i)), (shared(i), foreign()), (foreign(), shared(i)),
                      (own(i), orc.revcomp(own(i))), (own(i), foreign()), (own(i), shared(i)),
                      (own(i), b""), (_dna(rng, K - 1), shared(i)), (g[i][1300:1300 + K], own(i)),
                      (shared(i), g[(i + 4) % N_LEAVES][100:200])]
        pairs += [(foreign(), foreign()) for _ in range(8)]
        pairs += [(b"", b""), (_dna(rng, K - 1), b"A"), (b"", _dna(rng, K - 1)), (_dna(rng, K), _dna(rng, K))]
        pairs = [pairs[i] for i in rng.permutation(len(pairs))]
        return [m for p in pairs for m in p]

    def exp(self, block, units, thr=THR):
        key = (block, units, thr)
        if key not in self._exp:
            self._exp[key] = Expected(self, self.blocks[block], units, thr)
        return self._exp[key]


@pytest.fixture(scope="module")
def fx(gpu):
    x = Fixture()
    yield x
    x.gt.close()


def run(gt, dev, seq, off, thr, units, flag_set):
    """One call; the CSR (and scores) as copies, or None without PFQ_WANT_HITS (the device-resident entry)."""
    _, scores, lca, abundance, hits = flag_set
    kw = dict(paired=units != "reads", pair_mode=units if units != "reads" else "either", lca=lca)
    if not hits:
        gt.query_device(dev.seq.ptr, dev.off.ptr, dev.n, dev.total, thr, stream=dev.stream, **kw)
        return None
    return gt.query_packed(seq, off, thr, want_hits=True, want_scores=scores, abundance=abundance, **kw)


def check_call(gt, cm, e, res, flag_set, tag):
    """The results of one call, on counters and a log that were empty before it, against `e`."""
    name, scores, lca, abundance, hits = flag_set
    if hits:
        assert res[0].dtype == np.uint64 and np.array_equal(res[0], e.offs), tag
        assert res[1].dtype == np.uint32 and np.array_equal(res[1], e.leaves), tag
        assert len(res) == (3 if scores else 2), tag
    else:
        assert res is None, tag
    if scores:
        assert res[2].dtype == np.uint32 and np.array_equal(res[2].astype(np.int64), e.scores), tag
    assert [n for _, n in gt.get_leaf_counts()] == e.leaf_counts, tag
    here, below = gt.clade_counts()
    if lca:
        got, want = gt.last_lca(), e.lca[lca]
        assert got.dtype == np.uint32 and np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:10] if got.shape == want.shape else got.shape)
        want_here, want_below = cm.here_below(want)
        assert np.array_equal(here, want_here) and np.array_equal(below, want_below), tag
    else:
        assert not here.any() and not below.any(), tag
    log = abund_ref.classify(e.rows if abundance else [], N_LEAVES)
    same(gt.abundance(3, 0), abund_ref.estimate(log, 3, 0), tag)


# ---------------------------------------------------------------------------------------------------------------
# the blocks are what they say, on the oracle's values alone
# ---------------------------------------------------------------------------------------------------------------
def test_blocks_hold_every_class_of_unit(fx):
    for units in UNITS:
        e = fx.exp("a", units)
        sizes = [len(s) for s in e.sets]
        n_amb = sum(1 for n in sizes if 1 < n < N_LEAVES)
        print(units, "units", e.n, "unhit", sizes.count(0), "single", sizes.count(1), "ambiguous", n_amb, "all", sizes.count(N_LEAVES))
        assert e.n <= 400 and sizes.count(0) >= 1 and sizes.count(1) >= 1 and n_amb >= 1 and sizes.count(N_LEAVES) >= 1, units
        assert all(c > 0 for c in e.leaf_counts), units                       # positives from every genome
        assert (e.lca["all"] != e.lca["best"]).any(), units                     # PFQ_LCA_BEST is not PFQ_WANT_LCA here
        b = fx.exp("b", units)
        assert b.n == (40 if units == "reads" else 20) and int(b.offs[-1]) == 0 and (b.lca["all"] == NO).all(), units
        c = fx.exp("c", units)
        assert c.n == 0 and len(c.offs) == 1 and len(c.leaves) == 0, units
    lens = {len(r) for r in fx.blocks["a"]}
    assert {0, K - 1, K} <= lens
    both_short = [f for f in range(len(fx.blocks["a"]) // 2) if max(len(fx.blocks["a"][2 * f]), len(fx.blocks["a"][2 * f + 1])) < K]
    assert both_short and all(len(fx.exp("a", "both").sets[f]) == N_LEAVES for f in both_short)


# ---------------------------------------------------------------------------------------------------------------
# units x flag sets x paths x blocks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", ["a", "b", "c"])
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("units", UNITS)
def test_flag_matrix(fx, units, path, block):
    gt, cm = fx.gt, fx.cm
    e = fx.exp(block, units)
    seq, off = pack_reads(fx.blocks[block])
    dev = Device(seq, off)
    gt.set_path(path)
    try:
        plain = None
        for flag_set in FLAG_SETS:
            tag = (units, path, block, flag_set[0])
            gt.reset_counts()
            res = run(gt, dev, seq, off, THR, units, flag_set)
            check_call(gt, cm, e, res, flag_set, tag)
            if flag_set[0] == "hits":
                plain = res
            elif res is not None:                                             # the CSR of the same call with hits only
                assert np.array_equal(res[0], plain[0]) and np.array_equal(res[1], plain[1]), tag
            if block != "c" and 0 < THR <= 1:
                assert gt.last_stats().path == path, tag
    finally:
        dev.close()
        gt.set_path(-1)
        gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# the hit buffer overflows: the block runs again, everything is delivered once
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("units", UNITS)
def test_retry_delivers_once(fx, units):
    gt, cm = fx.gt, fx.cm
    e = fx.exp("a", units)
    seq, off = pack_reads(fx.blocks["a"])
    gt.set_option("PFQ_HIT_SLOTS", "0")
    try:
        for path in (0, 1):
            gt.set_path(path)
            gt.reset_counts()
            res = run(gt, None, seq, off, THR, units, EVERYTHING)
            c = gt.last_capacity()
            assert c["attempts"] == 2 and c["hit_cap"] == 0 < c["hit_cursor"], (units, path, c)
            check_call(gt, cm, e, res, EVERYTHING, (units, path, "retry"))
    finally:
        gt.set_option("PFQ_HIT_SLOTS", None)
        gt.set_path(-1)
        gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# one tree, call after call: the buffers of the call before are reused
# ---------------------------------------------------------------------------------------------------------------
def test_sequence_reuses_buffers(fx):
    """The mixed block doubled, the empty block, the block without hits, the mixed block; reads and fragments and the flag
    sets alternate.  Every call's results are checked; the counters and the log hold the sum of the calls."""
    gt, cm = fx.gt, fx.cm
    by_name = {f[0]: f for f in FLAG_SETS}
    steps = [("aa", "reads", "everything", 0.7), ("c", "either", "hits+scores", 1.0), ("b", "reads", "hits+abundance", 0.7),
             ("a", "both", "everything", 1.0), ("aa", "either", "hits", 0.7), ("c", "reads", "everything", 0.7),
             ("b", "both", "hits+scores+best", 1.0), ("a", "reads", "hits+lca", 1.0), ("a", "either", "everything", 0.7),
             ("b", "either", "lca alone", 0.7), ("a", "reads", "hits+scores", 0.7), ("aa", "both", "hits+abundance", 0.7)]
    gt.reset_counts()
    leaf_counts = [0] * N_LEAVES
    here_sum = np.zeros(len(cm.table), dtype=np.uint64)
    rows = []
    for i, (block, units, name, thr) in enumerate(steps):
        flag_set = by_name[name]
        _, scores, lca, abundance, hits = flag_set
        tag = (i, block, units, name, thr)
        e = fx.exp(block, units, thr)
        seq, off = pack_reads(fx.blocks[block])
        dev = Device(seq, off)
        try:
            res = run(gt, dev, seq, off, thr, units, flag_set)
            if hits:
                assert np.array_equal(res[0], e.offs) and np.array_equal(res[1], e.leaves), tag
            if scores:
                assert np.array_equal(res[2].astype(np.int64), e.scores), tag
            else:
                with pytest.raises(Exception):                                # no scores left over from the call before
                    gt.last_hit_scores()
            if lca:
                assert np.array_equal(gt.last_lca(), e.lca[lca]), tag
                here_sum += cm.here_below(e.lca[lca])[0]
            else:
                with pytest.raises(Exception):
                    gt.last_lca()
        finally:
            dev.close()
        leaf_counts = [a + b for a, b in zip(leaf_counts, e.leaf_counts)]
        if abundance:
            rows += e.rows
        assert [n for _, n in gt.get_leaf_counts()] == leaf_counts, tag
        assert np.array_equal(gt.clade_counts()[0], here_sum), tag
        same(gt.abundance(3, 0), abund_ref.estimate(abund_ref.classify(rows, N_LEAVES), 3, 0), tag)
    gt.reset_counts()
