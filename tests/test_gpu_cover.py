"""PFQ_WANT_COVERAGE on the device against tests/cover_ref.py over the oracle's rows: registers, units, matched, filter_bits,
n_units and precision exactly; distinct and genome_kmers — one formula applied to identical integers on both sides, so only
libm's rounding differs — at relative 1e-9."""
import ctypes as C
import math

import numpy as np
import pytest

import cover_ref
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_abund import reads_from, strain_families
from test_gpu_build import SEEDS, _dna
from test_gpu_lca import csr_of, oracle_sets
from test_gpu_paired import combine, mate_sets

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 4, 200003
PFQ_ERR_ARG, PFQ_ERR_STATE = -1, -6
INT_KEYS = ("units", "matched", "filter_bits")


def rows_of(sets):
    return [sorted(s) for s in sets]


def same(got, ref, tag=None):
    """A coverage() dict against a cover_ref.TreeSketcher."""
    sk = ref.sk
    assert (got["n_leaves"], got["precision"], got["n_units"]) == (sk.n_leaves, sk.p, sk.n_units), tag
    assert got["registers"].dtype == np.uint8 and got["registers"].shape == (sk.n_leaves, 1 << sk.p), tag
    assert np.array_equal(got["registers"], np.array(sk.registers, dtype=np.uint8)), tag
    for k, want in (("units", sk.units), ("matched", sk.matched), ("filter_bits", ref.filter_bits())):
        assert got[k].dtype == np.uint64 and got[k].tolist() == want, (tag, k, got[k].tolist(), want)
    for k, want in (("distinct", sk.distinct()), ("genome_kmers", ref.genome_kmers())):
        assert got[k].dtype == np.float64 and got[k].tolist() == pytest.approx(want, rel=1e-9, abs=0), (tag, k)


def equal(a, b, tag=None):
    """Two coverage() dicts."""
    for k in ("n_leaves", "precision", "n_units"):
        assert a[k] == b[k], (tag, k)
    for k in ("registers",) + INT_KEYS + ("distinct", "genome_kmers"):
        assert np.array_equal(a[k], b[k]), (tag, k)


def is_empty(cov, n_leaves, p=12):
    return (cov["n_leaves"] == n_leaves and cov["precision"] == p and cov["n_units"] == 0 and cov["registers"].shape == (n_leaves, 1 << p) and
            not cov["registers"].any() and not cov["units"].any() and not cov["matched"].any() and not cov["distinct"].any())


class Fam:
    """16 leaves: 4 families of 3 strains and 4 unrelated genomes.  540 reads of 100 bp (80 k-mers: a full window of 64 and
    a tail) from five of the genomes, unrelated reads, and reads of exactly k, shorter than k and empty."""

    def __init__(self):
        rng = np.random.default_rng(1217)
        self.genomes = strain_families(rng, 4, 3, 2000, 0.006, 4)
        self.ids = [f"C{i:02d}" for i in range(16)]
        self.ot = orc.build_balanced_tree(self.genomes, self.ids, K, NBITS, H, *SEEDS)
        self.gt = self.new_tree()
        reads = reads_from(rng, self.genomes, [0, 3, 6, 12, 13], 500, 100)
        g = self.genomes[9]
        reads += [_dna(rng, 100) for _ in range(28)] + [b"", b"ACGT", _dna(rng, K - 1), g[40:40 + K], g[700:700 + K + 1], _dna(rng, K)] * 2
        self.reads = [reads[i] for i in rng.permutation(len(reads))]
        assert len(self.reads) <= 600
        self.seq, self.off = pack_reads(self.reads)
        self.rng = rng
        self._rows, self._want = {}, {}
        self.cache = cover_ref.TreeSketcher(self.ot)                      # (only its memory of the oracle's answers is used)

    def new_tree(self):
        return BloomTree.build_balanced(self.genomes, self.ids, K, NBITS, H, *SEEDS)

    def rows(self, thr):
        if thr not in self._rows:
            self._rows[thr] = rows_of(oracle_sets(self.ot, self.reads, thr))
        return self._rows[thr]

    def sketcher(self, p=12):
        return cover_ref.TreeSketcher(self.ot, p, share=self.cache)

    def want(self, thr):
        """The reference over all reads at `thr`, computed once; nothing changes it."""
        if thr not in self._want:
            self._want[thr] = self.sketcher().add_reads(self.rows(thr), self.reads)
        return self._want[thr]

    def parts(self):
        n = len(self.reads)
        return [(0, n // 6), (n // 6, n // 2), (n // 2, n)]


@pytest.fixture(scope="module")
def fam(gpu):
    x = Fam()
    yield x
    x.gt.close()


def sketch_reads(gt, reads, thr, **kw):
    seq, off = pack_reads(reads)
    return gt.query_packed(seq, off, thr, want_hits=True, coverage=True, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 1. against the reference: the shortcut (threshold 1) and the probing path
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_against_reference(fam, thr):
    gt, rows, want = fam.gt, fam.rows(thr), fam.want(thr)
    # the case is what it says: shared and single rows, every-leaf rows of the short reads, reads without hits
    assert sum(1 for r in rows if len(r) == 16) == 6 and sum(1 for r in rows if 1 < len(r) < 16) >= 80, [len(r) for r in rows]
    assert sum(1 for r in rows if len(r) == 1) >= 100 and sum(1 for r in rows if not r) >= 20
    assert sum(1 for m in want.sk.matched if m) >= 7
    gt.reset_counts()
    res = sketch_reads(gt, fam.reads, thr)
    woff, wleaves = csr_of([set(r) for r in rows])
    assert np.array_equal(res[0], woff) and np.array_equal(res[1], wleaves)
    same(gt.coverage(), want, thr)
    same(gt.coverage(), want, (thr, "again"))                              # the sketch is not consumed
    gt.query_packed(fam.seq, fam.off, thr, want_hits=True)                 # calls without the flag sketch nothing
    gt.query_packed(fam.seq, fam.off, thr)
    same(gt.coverage(), want, (thr, "after calls without the flag"))
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 2. call splitting and launch shape
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_split_and_launch_shape(fam, thr):
    gt, want = fam.gt, fam.want(thr)
    try:
        for blocks in (None, "1", "3", "5000"):
            gt.set_option("PFQ_COVER_BLOCKS", blocks)
            gt.coverage_reset()
            sketch_reads(gt, fam.reads, thr)
            one = gt.coverage()
            same(one, want, ("one call", blocks))
            gt.coverage_reset()
            for a, b in fam.parts():
                sketch_reads(gt, fam.reads[a:b], thr)
            equal(gt.coverage(), one, ("three calls", blocks))
            gt.coverage_reset()
            sketch_reads(gt, fam.reads[::-1], thr)
            equal(gt.coverage(), one, ("reversed", blocks))
    finally:
        gt.set_option("PFQ_COVER_BLOCKS", None)
        gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 3. beside the scores, the counters and the LCAs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_scores_counts_and_lca(fam, thr):
    gt = fam.gt
    n = len(fam.reads)
    gt.reset_counts()
    for a, b in ((0, n // 3), (n // 3, n)):                                # (the second call: deltas on a sketch that holds something)
        seq, off = pack_reads(fam.reads[a:b])
        counts0 = [c for _, c in gt.get_leaf_counts()]
        plain = gt.query_packed(seq, off, thr, want_hits=True, want_scores=True, lca="best")
        lca_plain = gt.last_lca()
        counts1 = [c for _, c in gt.get_leaf_counts()]
        before = gt.coverage()
        res = gt.query_packed(seq, off, thr, want_hits=True, want_scores=True, lca="best", coverage=True)
        assert all(np.array_equal(x, y) for x, y in zip(res, plain)) and np.array_equal(gt.last_lca(), lca_plain)
        counts2 = [c for _, c in gt.get_leaf_counts()]
        delta = [y - x for x, y in zip(counts0, counts1)]
        assert [y - x for x, y in zip(counts1, counts2)] == delta         # the flag changes no counter
        after = gt.coverage()
        offs, leaves, scores = res
        want_matched, want_units = [0] * 16, [0] * 16
        for l, s in zip(leaves.tolist(), scores.tolist()):
            want_matched[l] += s
            want_units[l] += 1
        assert (after["matched"] - before["matched"]).tolist() == want_matched
        assert (after["units"] - before["units"]).tolist() == want_units == delta
        assert after["n_units"] - before["n_units"] == b - a
    same(gt.coverage(), fam.want(thr), thr)
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 4. paired
# ---------------------------------------------------------------------------------------------------------------
def make_pairs(fam):
    rng, g, pairs = np.random.default_rng(4), fam.genomes, []
    for i in range(100):
        a = g[[0, 3, 6, 12][i % 4]]
        o = int(rng.integers(0, len(a) - 350))
        pairs.append((a[o:o + 100], orc.revcomp(a[o + 250:o + 350])))
    for i in range(30):                                                    # mates from different genomes
        a, b = g[int(rng.integers(0, 16))], g[int(rng.integers(0, 16))]
        oa, ob = int(rng.integers(0, len(a) - 100)), int(rng.integers(0, len(b) - 100))
        pairs.append((a[oa:oa + 100], b[ob:ob + 100]))
    for i in range(12):                                                    # one mate shorter than k, empty, or of exactly k
        a = g[3 * (i % 4)]
        o = int(rng.integers(0, len(a) - 100))
        short = [b"", b"ACGT", _dna(rng, K - 1), a[5:5 + K]][i % 4]
        pairs.append((short, a[o:o + 100]) if i % 2 else (a[o:o + 100], short))
    pairs += [(_dna(rng, 100), _dna(rng, 100)) for _ in range(6)] + [(b"", b""), (b"A", _dna(rng, K - 1))]
    return [pairs[i] for i in rng.permutation(len(pairs))]


@pytest.mark.parametrize("mode", ["either", "both"])
def test_paired(fam, mode):
    gt = fam.gt
    pairs = make_pairs(fam)
    r1, r2 = [p[0] for p in pairs], [p[1] for p in pairs]
    for thr in (1.0, 0.5):
        mates = mate_sets(fam.ot, [m for p in pairs for m in p], thr)
        for v in range(fam.ot.n_nodes):
            fam.ot.mapped_reads[v] = 0
        rows = rows_of(combine(mates, mode))
        assert sum(1 for r in rows if len(r) == 16) >= 2 and sum(1 for r in rows if 0 < len(r) < 16) >= 80, (mode, thr)
        want = fam.sketcher().add_pairs(rows, pairs)
        gt.reset_counts()
        plain = gt.query_pairs(r1, r2, thr, mode=mode)
        counts = gt.get_leaf_counts()
        gt.reset_counts()
        got = gt.query_pairs(r1, r2, thr, mode=mode, coverage=True)
        assert got == plain == rows and gt.get_leaf_counts() == counts
        cov = gt.coverage()
        assert cov["n_units"] == len(pairs)                                # units are fragments
        same(cov, want, (mode, thr))
        assert cov["units"].tolist() == [c for _, c in counts]
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 5. rows longer than 64 leaves
# ---------------------------------------------------------------------------------------------------------------
def test_long_rows(gpu):
    """72 leaves at threshold 0: every read lists every leaf, in chunks of 64 and 8, and every k-mer is probed in every
    leaf's filter."""
    rng = np.random.default_rng(72)
    genomes = strain_families(rng, 3, 4, 1500, 0.01, 60)
    ids = [f"L{i:02d}" for i in range(72)]
    ot = orc.build_balanced_tree(genomes, ids, K, NBITS, H, *SEEDS)
    gt = BloomTree.build_balanced(genomes, ids, K, NBITS, H, *SEEDS)
    try:
        reads = reads_from(rng, genomes, [0, 5, 9, 40, 71], 6, 100) + [_dna(rng, 100), b"ACGT", genomes[70][3:3 + K]]
        rows = rows_of(oracle_sets(ot, reads, 0.0))
        assert all(r == list(range(72)) for r in rows)
        want = cover_ref.TreeSketcher(ot).add_reads(rows, reads)
        assert sum(1 for m in want.sk.matched[64:] if m) >= 2 and sum(1 for m in want.sk.matched[:64] if m) >= 4
        sketch_reads(gt, reads, 0.0)
        same(gt.coverage(), want)
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. precision
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 16])
def test_precision(fam, p):
    gt = fam.new_tree()
    try:
        gt.set_option("PFQ_COVER_P", str(p))
        assert is_empty(gt.coverage(), 16, p)
        reads, rows = fam.reads[:120], fam.rows(0.5)[:120]
        sketch_reads(gt, reads, 0.5)
        same(gt.coverage(), fam.sketcher(p).add_reads(rows, reads), p)
        gt.set_option("PFQ_COVER_P", str(p))                               # the value it has: nothing to change
        for other in ("12", None):
            with pytest.raises(PfqError) as e:
                gt.set_option("PFQ_COVER_P", other)
            assert e.value.code == PFQ_ERR_STATE and "PFQ_COVER_P" in str(e.value)
        assert gt.coverage()["precision"] == p
        for bad in ("3", "17", "-2"):
            with pytest.raises(PfqError) as e:
                gt.set_option("PFQ_COVER_P", bad)
            assert e.value.code == PFQ_ERR_ARG
        gt.coverage_reset()
        gt.set_option("PFQ_COVER_P", None)                                 # an empty sketch takes a new precision
        assert is_empty(gt.coverage(), 16, 12)
        sketch_reads(gt, reads, 0.5)
        same(gt.coverage(), fam.sketcher(12).add_reads(rows, reads), "default again")
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. absorb
# ---------------------------------------------------------------------------------------------------------------
def test_absorb(fam):
    thr = 0.5
    a, b = fam.new_tree(), fam.new_tree()
    try:
        n = len(fam.reads)
        sketch_reads(a, fam.reads[:n // 2], thr)
        sketch_reads(b, fam.reads[n // 2:], thr)
        counts_b = b.get_leaf_counts()
        same(b.coverage(), fam.sketcher().add_reads(fam.rows(thr)[n // 2:], fam.reads[n // 2:]), "b alone")
        a.coverage_absorb(b)
        same(a.coverage(), fam.want(thr), "absorbed")
        assert is_empty(b.coverage(), 16) and b.get_leaf_counts() == counts_b
        a.coverage_absorb(b)                                               # an empty sketch adds nothing
        same(a.coverage(), fam.want(thr), "absorbed an empty sketch")
        b.coverage_absorb(a)                                               # into a tree that has none yet
        same(b.coverage(), fam.want(thr), "moved")
        assert is_empty(a.coverage(), 16)
        with pytest.raises(PfqError) as e:
            a.coverage_absorb(a)
        assert e.value.code == PFQ_ERR_ARG
        a.set_option("PFQ_COVER_P", "10")
        with pytest.raises(PfqError) as e:
            b.coverage_absorb(a)
        assert e.value.code == PFQ_ERR_ARG and "precision" in str(e.value)
        with pytest.raises(PfqError) as e:
            a.coverage_absorb(b)
        assert e.value.code == PFQ_ERR_ARG and "precision" in str(e.value)
        same(b.coverage(), fam.want(thr), "refused: unchanged")
        small = BloomTree.build_balanced(fam.genomes[:8], fam.ids[:8], K, NBITS, H, *SEEDS)
        try:
            with pytest.raises(PfqError) as e:
                b.coverage_absorb(small)
            assert e.value.code == PFQ_ERR_ARG
        finally:
            small.close()
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. state and errors
# ---------------------------------------------------------------------------------------------------------------
def test_state_and_errors(fam, tmp_path):
    gt, thr = fam.new_tree(), 1.0
    try:
        first = gt.coverage()                                              # before any flagged call
        assert is_empty(first, 16)
        ref = fam.sketcher()
        assert first["filter_bits"].tolist() == ref.filter_bits() and all(b > 0 for b in ref.filter_bits())
        assert first["genome_kmers"].tolist() == pytest.approx(ref.genome_kmers(), rel=1e-9, abs=0)
        # the flag without the hits
        L, hits = _ffi.lib(), _ffi.Hits()
        seq, off = pack_reads(fam.reads[:50])
        for flags in (_ffi.WANT_COVERAGE, _ffi.WANT_COVERAGE | _ffi.WANT_LCA, _ffi.WANT_COVERAGE | _ffi.PAIRED):
            rc = L.pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, 50, thr, flags, C.byref(hits))
            assert rc == PFQ_ERR_ARG and b"PFQ_WANT_COVERAGE" in L.pfq_last_error(), flags
        assert L.pfq_coverage_get(gt._h, None) == PFQ_ERR_ARG
        assert is_empty(gt.coverage(), 16)
        # device memory: the registers and two counters per leaf, from the first flagged call to the reset
        # (the call's own scratch buffers settle with the second call of a kind: the hit buffer is sized by the first one's hits)
        sketch_bytes = (16 << 12) + 2 * 8 * 16
        for _ in range(2):
            gt.query_packed(fam.seq, fam.off, thr, want_hits=True)
        bytes0 = int(gt.info().device_bytes)
        sketch_reads(gt, fam.reads, thr)
        assert int(gt.info().device_bytes) == bytes0 + sketch_bytes
        same(gt.coverage(), fam.want(thr), "first")
        counts = gt.get_leaf_counts()
        gt.coverage_reset()                                                # clears the sketch, not the leaf counters
        assert is_empty(gt.coverage(), 16) and gt.get_leaf_counts() == counts
        assert int(gt.info().device_bytes) == bytes0
        gt.query_packed(fam.seq, fam.off, thr, want_hits=True)            # without the flag no sketch is made
        assert int(gt.info().device_bytes) == bytes0
        # pfq_leaf_counts_reset
        sketch_reads(gt, fam.reads[:100], thr)
        assert gt.coverage()["n_units"] == 100
        gt.reset_counts()
        assert is_empty(gt.coverage(), 16)
        # the sketch is not stored
        sketch_reads(gt, fam.reads[:100], thr)
        d = str(tmp_path / "db")
        gt.save(d)
        t2 = BloomTree.load(d)
        assert is_empty(t2.coverage(), 16)
        t2.close()
        # prune: the leaf columns change meaning
        gt.prune_tree(2)
        cov = gt.coverage()
        assert is_empty(cov, 4) and all(b > 0 for b in cov["filter_bits"].tolist())
    finally:
        gt.close()
    # insert
    rng = np.random.default_rng(8)
    genomes = [_dna(rng, 1500) for _ in range(3)]
    t = BloomTree.new(K, 0.001, 2000, *SEEDS)
    try:
        for g, i in zip(genomes[:2], ("a", "b")):
            t.insert(g, i)
        sketch_reads(t, [genomes[0][:100], genomes[1][50:150]], 1.0)
        cov = t.coverage()
        assert cov["n_units"] == 2 and cov["units"].tolist() == [1, 1] and cov["matched"].tolist() == [80, 80]
        t.insert(genomes[2], "c")
        cov = t.coverage()
        assert is_empty(cov, 3) and all(b > 0 for b in cov["filter_bits"].tolist())
    finally:
        t.close()


@pytest.mark.parametrize("path", [0, 1])
def test_hit_buffer_retry_sketches_once(fam, path):
    gt, thr = fam.gt, 1.0
    gt.reset_counts()
    gt.set_path(path)
    gt.set_option("PFQ_HIT_SLOTS", "0")
    try:
        sketch_reads(gt, fam.reads, thr)
        c = gt.last_capacity()
        assert c["attempts"] == 2 and c["hit_cap"] == 0 < c["hit_cursor"], c
        same(gt.coverage(), fam.want(thr), path)
    finally:
        gt.set_option("PFQ_HIT_SLOTS", None)
        gt.set_path(-1)
        gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 9. subtree shards
# ---------------------------------------------------------------------------------------------------------------
def test_shards(fam, tmp_path):
    gt, thr = fam.gt, 0.5
    d = str(tmp_path / "db")
    gt.reset_counts()
    gt.save(d)
    sketch_reads(gt, fam.reads, thr)
    whole = gt.coverage()
    gt.reset_counts()
    n_shards = BloomTree.shard_count(d, 2)
    assert n_shards == 4
    seen = 0
    for i in range(n_shards):
        shard = BloomTree.load_subtree(d, 2, i)
        try:
            info = shard.info()
            lo, nl = int(info.shard_first_leaf), int(info.n_leaves)
            assert lo == seen and nl > 0
            sketch_reads(shard, fam.reads, thr)
            cov = shard.coverage()
            assert (cov["n_leaves"], cov["precision"], cov["n_units"]) == (nl, 12, len(fam.reads))
            for k in ("registers",) + INT_KEYS + ("distinct", "genome_kmers"):
                assert np.array_equal(cov[k], whole[k][lo:lo + nl]), (i, k)
            seen += nl
        finally:
            shard.close()
    assert seen == 16


# ---------------------------------------------------------------------------------------------------------------
# 10. end to end: one genome tiled by its reads
# ---------------------------------------------------------------------------------------------------------------
def test_tiled_genome_distinct_kmers(gpu):
    """The estimate against the exact number of distinct matched canonical k-mers (a Python set), within 4 standard errors
    (4 * 1.04 / sqrt(4096) = 6.5 %): the bound tests/test_cover_cpu.py derives for the estimator, which the reference is
    checked against for this fixture as well."""
    rng = np.random.default_rng(10)
    genomes = [_dna(rng, 6000) for _ in range(4)]
    ids = ["g0", "g1", "g2", "g3"]
    ot = orc.build_balanced_tree(genomes, ids, K, NBITS, H, *SEEDS)
    gt = BloomTree.build_balanced(genomes, ids, K, NBITS, H, *SEEDS)
    try:
        g = genomes[1]
        reads = [g[o:o + 100] for o in range(0, len(g) - 99, 10)]          # every k-mer about eight times
        reads = [orc.revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
        assert len(reads) <= 600
        rows = rows_of(oracle_sets(ot, reads, 1.0))
        assert all(1 in r for r in rows)
        exact = len({c for r in reads for c in orc.get_kmers(r, K)})
        assert 5900 <= exact <= 5980
        sketch_reads(gt, reads, 1.0)
        cov = gt.coverage()
        ref = cover_ref.TreeSketcher(ot).add_reads(rows, reads)
        same(cov, ref)
        bound = 4 * 1.04 / math.sqrt(4096)
        for name, est in (("reference", ref.sk.distinct()[1]), ("library", float(cov["distinct"][1]))):
            print(f"{name}: distinct {est:.1f} of {exact}, relative error {est / exact - 1:+.4f}, bound {bound:.4f}")
            assert abs(est / exact - 1) <= bound, (name, est, exact)
        assert cov["units"][1] == len(reads) and cov["matched"][1] == 80 * len(reads)
    finally:
        gt.close()
