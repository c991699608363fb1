"""PFQ_WANT_ABUNDANCE on the device against the oracle: the rows every unit logs are the oracle's query_batch rows (fragments:
the mates' rows combined), and the estimate over them is the plain-Python restatement of tests/abund_ref.py.  Every comparison
is exact: mass, unique, the class counters, iterations, converged and last_delta."""
import ctypes as C

import numpy as np
import pytest

import abund_ref
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_build import SEEDS, _dna, _mutate
from test_gpu_lca import Device, csr_of, oracle_sets
from test_gpu_paired import combine, mate_sets

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 4, 200003
PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -4, -6
KEYS = ("n_units", "n_unhit", "n_unique", "n_ambiguous", "n_all_leaves", "n_entries", "iterations", "converged", "last_delta")


def rows_of(sets):
    return [sorted(s) for s in sets]


def expect(rows, n_leaves, iters=200, tol=0):
    return abund_ref.estimate(abund_ref.classify(rows, n_leaves), iters, tol)


def same(got, want, tag=None):
    for k in KEYS:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    for k in ("unique", "mass"):                                              # (`want`: the restatement's lists, or another estimate)
        assert got[k].dtype == np.uint64 and got[k].tolist() == [int(x) for x in want[k]], (tag, k)


def is_empty(est, n_leaves):
    return (all(est[k] == 0 for k in KEYS[:6]) and est["iterations"] == 1 and est["converged"] == 1 and est["last_delta"] == 0 and
            est["mass"].tolist() == [0] * n_leaves and est["unique"].tolist() == [0] * n_leaves)


def strain_families(rng, n_fam, strains, length, rate, singles):
    """`n_fam` families of `strains` genomes a few substitutions apart, and unrelated genomes; family f's strains are
    genomes [f * strains, (f + 1) * strains)."""
    out = []
    for _ in range(n_fam):
        base = _dna(rng, length)
        out += [_mutate(rng, base, rng.binomial(length, rate)) for _ in range(strains)]
    return out + [_dna(rng, length) for _ in range(singles)]


def reads_from(rng, genomes, sources, n, length):
    out = []
    for _ in range(n):
        g = genomes[sources[int(rng.integers(0, len(sources)))]]
        o = int(rng.integers(0, len(g) - length + 1))
        r = g[o:o + length]
        out.append(orc.revcomp(r) if rng.random() < 0.5 else r)
    return out


class Fam:
    """16 leaves: 4 families of 3 strains whose reads are mostly shared with the sister strains, 4 unrelated genomes.  Reads
    come from the first strain of every family and from two of the unrelated genomes; some reads are shorter than k (they hit
    every leaf), some match nothing."""

    def __init__(self, device=True):
        rng = np.random.default_rng(2024)
        self.genomes = strain_families(rng, 4, 3, 2000, 0.006, 4)
        self.ids = [f"A{i:02d}" for i in range(16)]
        self.ot = orc.build_balanced_tree(self.genomes, self.ids, K, NBITS, H, *SEEDS)
        self.gt = BloomTree.build_balanced(self.genomes, self.ids, K, NBITS, H, *SEEDS) if device else None
        reads = reads_from(rng, self.genomes, [0, 3, 6, 9, 12, 13], 2400, 100)
        reads += [_dna(rng, 100) for _ in range(150)] + [b"", b"ACGT", _dna(rng, K - 1)] * 4
        self.reads = [reads[i] for i in rng.permutation(len(reads))]
        self.seq, self.off = pack_reads(self.reads)
        self.rng = rng
        self._rows = {}

    def new_tree(self):
        return BloomTree.build_balanced(self.genomes, self.ids, K, NBITS, H, *SEEDS)

    def rows(self, thr):
        if thr not in self._rows:
            self._rows[thr] = rows_of(oracle_sets(self.ot, self.reads, thr))
        return self._rows[thr]

    def parts(self):
        """Three runs of the reads, of unequal size."""
        n = len(self.reads)
        return [(0, n // 6), (n // 6, n // 2), (n // 2, n)]


@pytest.fixture(scope="module")
def fam(gpu):
    x = Fam()
    yield x
    x.gt.close()


def log_reads(gt, reads, thr, **kw):
    seq, off = pack_reads(reads)
    return gt.query_packed(seq, off, thr, want_hits=True, abundance=True, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 1. related strains
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_related_strains(fam, thr):
    gt, rows = fam.gt, fam.rows(thr)
    log = abund_ref.classify(rows, 16)
    # the case is what it says: every class occurs, and the strains share reads
    assert log["n_unhit"] >= 100 and log["n_all_leaves"] == 12 and log["n_unique"] >= 300 and log["n_ambiguous"] >= 500, log
    gt.reset_counts()
    plain = gt.query_packed(fam.seq, fam.off, thr, want_hits=True)
    counts = gt.get_leaf_counts()
    gt.reset_counts()
    res = gt.query_packed(fam.seq, fam.off, thr, want_hits=True, abundance=True)
    assert all(np.array_equal(a, b) for a, b in zip(res, plain)) and gt.get_leaf_counts() == counts
    woff, wleaves = csr_of([set(r) for r in rows])
    assert np.array_equal(res[0], woff) and np.array_equal(res[1], wleaves)
    for iters in (1, 7, 200):
        same(gt.abundance(iters, 0), abund_ref.estimate(log, iters, 0), (thr, iters))
    same(gt.abundance(), abund_ref.estimate(log), (thr, "defaults"))          # 200 iterations, tol 65
    full = gt.abundance(200, 0)
    # the estimate does what it is for: the sister strains keep far less than the reads that list them
    listed = [n for _, n in counts]
    for f in range(4):
        present, sisters = 3 * f, (3 * f + 1, 3 * f + 2)
        assert all(int(full["mass"][s]) >> 16 < listed[s] // 2 for s in sisters), (f, full["mass"], listed)
        assert int(full["mass"][present]) > max(int(full["mass"][s]) for s in sisters)
    # with the scores and the LCAs beside it, nothing changes
    gt.reset_counts()
    res2 = gt.query_packed(fam.seq, fam.off, thr, want_hits=True, want_scores=True, lca="best", abundance=True)
    assert np.array_equal(res2[0], woff) and np.array_equal(res2[1], wleaves) and gt.get_leaf_counts() == counts
    same(gt.abundance(7, 0), abund_ref.estimate(log, 7, 0), (thr, "with scores and lca"))
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 2. order and split of the calls, launch shape, LDS
# ---------------------------------------------------------------------------------------------------------------
def test_order_split_and_knobs(fam):
    gt, thr = fam.gt, 0.5
    want = expect(fam.rows(thr), 16, 200, 0)
    want7 = expect(fam.rows(thr), 16, 7, 0)
    try:
        for blocks, lds in ((None, None), ("1", None), ("5000", None), (None, "0"), ("3", "0")):
            gt.set_option("PFQ_ABUND_BLOCKS", blocks)
            gt.set_option("PFQ_ABUND_LDS", lds)
            gt.abundance_reset()
            log_reads(gt, fam.reads, thr)
            same(gt.abundance(200, 0), want, ("one call", blocks, lds))
            gt.abundance_reset()
            for a, b in fam.parts():
                log_reads(gt, fam.reads[a:b], thr)
            same(gt.abundance(200, 0), want, ("three calls", blocks, lds))
            same(gt.abundance(7, 0), want7, ("three calls, 7", blocks, lds))
            gt.abundance_reset()
            log_reads(gt, fam.reads[::-1], thr)
            same(gt.abundance(200, 0), want, ("reversed", blocks, lds))
    finally:
        gt.set_option("PFQ_ABUND_BLOCKS", None)
        gt.set_option("PFQ_ABUND_LDS", None)
    # the device-resident entry on a stream of its own, in two calls
    gt.abundance_reset()
    n = len(fam.reads)
    for a, b in ((n // 3, n), (0, n // 3)):
        seq, off = pack_reads(fam.reads[a:b])
        dev = Device(seq, off)
        try:
            res = gt.query_device_hits(dev.seq.ptr, dev.off.ptr, dev.n, dev.total, thr, stream=dev.stream, abundance=True)
            woff, wleaves = csr_of([set(r) for r in fam.rows(thr)[a:b]])
            assert np.array_equal(res[0], woff) and np.array_equal(res[1], wleaves)
        finally:
            dev.close()
    same(gt.abundance(200, 0), want, "device entry")
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 3. long rows
# ---------------------------------------------------------------------------------------------------------------
def test_long_rows(gpu):
    """96 leaves, 80 of them strains of one genome that each lost a window of their own: a read lists the strains whose
    window it does not touch, most rows hold more than 64 leaves (a wave takes such a row) and fewer than all 96."""
    rng = np.random.default_rng(96)
    base = _dna(rng, 2000)
    strains = []
    for _ in range(80):
        o = int(rng.integers(0, 2000 - 150))
        strains.append(_mutate(rng, base[:o] + _dna(rng, 150) + base[o + 150:], 3))
    genomes = strains + [_dna(rng, 2000) for _ in range(16)]
    order = rng.permutation(96)
    genomes = [genomes[i] for i in order]
    ids = [f"L{i:02d}" for i in range(96)]
    ot = orc.build_balanced_tree(genomes, ids, K, NBITS, H, *SEEDS)
    gt = BloomTree.build_balanced(genomes, ids, K, NBITS, H, *SEEDS)
    try:
        reads = reads_from(rng, [base], [0], 1500, 100) + reads_from(rng, genomes, list(range(96)), 500, 100)
        reads += [_dna(rng, 100) for _ in range(50)]
        zero = reads[:40] + [b"", b"ACGT"]                                   # threshold 0: every leaf
        rows = rows_of(oracle_sets(ot, reads, 0.5))
        n_long = sum(1 for r in rows if 64 < len(r) < 96)
        n_short = sum(1 for r in rows if 1 < len(r) <= 64)
        assert n_long >= 300 and n_short >= 50, (n_long, n_short)           # both kinds of row, from the oracle
        rows0 = rows_of(oracle_sets(ot, zero, 0.0))
        assert all(len(r) == 96 for r in rows0)
        log_reads(gt, reads, 0.5)
        log_reads(gt, zero, 0.0)
        log = abund_ref.classify(rows + rows0, 96)
        assert log["n_all_leaves"] >= len(zero)
        for iters in (1, 5, 60):
            same(gt.abundance(iters, 0), abund_ref.estimate(log, iters, 0), iters)
        gt.set_option("PFQ_ABUND_LDS", "0")
        same(gt.abundance(5, 0), abund_ref.estimate(log, 5, 0), "global atomics")
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. growth and cap
# ---------------------------------------------------------------------------------------------------------------
def test_growth_and_cap(fam):
    gt, thr, L = fam.gt, 0.5, _ffi.lib()
    rows = fam.rows(thr)
    parts = fam.parts()
    ent = [abund_ref.classify(rows[a:b], 16)["n_entries"] for a, b in parts]
    assert all(e > 0 for e in ent)
    gt.reset_counts()
    try:
        gt.set_option("PFQ_ABUND_SLOTS", ent[0] + ent[1] - 1)                # the second call's rows do not fit
        log_reads(gt, fam.reads[parts[0][0]:parts[0][1]], thr)
        seq, off = pack_reads(fam.reads[parts[1][0]:parts[1][1]])
        hits = _ffi.Hits()
        flags = _ffi.WANT_HITS | _ffi.WANT_ABUNDANCE
        rc = L.pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, len(off) - 1, thr, flags, C.byref(hits))
        msg = L.pfq_last_error().decode()
        assert rc == PFQ_ERR_UNSUPPORTED and "abundance log" in msg and "PFQ_ABUND_SLOTS" in msg, (rc, msg)
        # its hits and counts stand
        n = len(off) - 1
        woff, wleaves = csr_of([set(r) for r in rows[parts[1][0]:parts[1][1]]])
        assert int(hits.n_reads) == n
        assert np.array_equal(np.ctypeslib.as_array(hits.offsets, shape=(n + 1,)), woff)
        assert np.array_equal(np.ctypeslib.as_array(hits.leaves, shape=(int(woff[-1]),)), wleaves)
        want_counts = [0] * 16
        for r in rows[:parts[1][1]]:
            for l in r:
                want_counts[l] += 1
        assert [c for _, c in gt.get_leaf_counts()] == want_counts
        with pytest.raises(PfqError) as e:
            gt.abundance()
        assert e.value.code == PFQ_ERR_STATE and "incomplete" in str(e.value)
        with pytest.raises(PfqError) as e:                                    # and it stays incomplete until the reset
            log_reads(gt, fam.reads[parts[2][0]:parts[2][1]], thr)
        assert e.value.code == PFQ_ERR_UNSUPPORTED and "abundance log" in str(e.value)
        with pytest.raises(PfqError) as e:
            gt.abundance(5, 0)
        assert e.value.code == PFQ_ERR_STATE
    finally:
        gt.set_option("PFQ_ABUND_SLOTS", None)
    gt.abundance_reset()
    assert is_empty(gt.abundance(), 16)
    # without the cap the log grows call by call: it starts at 1024 entries and at most doubles, unless a call needs more, so
    # these sizes force two reallocations that have to keep what the log held
    cap1 = max(ent[0], 1024)
    assert ent[0] + ent[1] > cap1
    cap2 = max(ent[0] + ent[1], 2 * cap1)
    assert sum(ent) > cap2
    held = 0
    for (a, b), e_part in zip(parts, ent):
        log_reads(gt, fam.reads[a:b], thr)
        held += e_part
        assert gt.abundance(1, 0)["n_entries"] == held
    same(gt.abundance(200, 0), expect(rows, 16, 200, 0), "after growth")
    # a cap that is just enough is not an overflow
    gt.abundance_reset()
    gt.set_option("PFQ_ABUND_SLOTS", sum(ent))
    try:
        for a, b in parts:
            log_reads(gt, fam.reads[a:b], thr)
        same(gt.abundance(7, 0), expect(rows, 16, 7, 0), "exact cap")
    finally:
        gt.set_option("PFQ_ABUND_SLOTS", None)
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 5. paired
# ---------------------------------------------------------------------------------------------------------------
def make_pairs(fam):
    rng, g, pairs = np.random.default_rng(5), fam.genomes, []
    for i in range(600):
        a = g[[0, 3, 6, 9, 12][i % 5]]
        o = int(rng.integers(0, len(a) - 350))
        pairs.append((a[o:o + 100], orc.revcomp(a[o + 250:o + 350])))
    for i in range(100):
        a, b = g[int(rng.integers(0, 16))], g[int(rng.integers(0, 16))]
        oa, ob = int(rng.integers(0, len(a) - 100)), int(rng.integers(0, len(b) - 100))
        pairs.append((a[oa:oa + 100], b[ob:ob + 100]))
    for i in range(30):
        a = g[3 * (i % 4)]
        o = int(rng.integers(0, len(a) - 100))
        short = [b"", b"ACGT", _dna(rng, K - 1)][i % 3]
        pairs.append((short, a[o:o + 100]) if i % 2 else (a[o:o + 100], short))
    pairs += [(_dna(rng, 100), _dna(rng, 100)) for _ in range(40)] + [(b"", b""), (b"A", _dna(rng, K - 1))]
    return [pairs[i] for i in rng.permutation(len(pairs))]


@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_paired(fam, thr):
    gt = fam.gt
    pairs = make_pairs(fam)
    r1, r2 = [p[0] for p in pairs], [p[1] for p in pairs]
    mates = mate_sets(fam.ot, [m for p in pairs for m in p], thr)
    for v in range(fam.ot.n_nodes):
        fam.ot.mapped_reads[v] = 0
    for mode in ("either", "both"):
        rows = rows_of(combine(mates, mode))
        log = abund_ref.classify(rows, 16)
        assert log["n_ambiguous"] >= 100 and log["n_unique"] >= 30 and log["n_all_leaves"] >= 1 and log["n_unhit"] >= 10, (mode, log)
        gt.reset_counts()
        plain = gt.query_pairs(r1, r2, thr, mode=mode)
        counts = gt.get_leaf_counts()
        gt.reset_counts()
        got = gt.query_pairs(r1, r2, thr, mode=mode, abundance=True)
        assert got == plain == rows and gt.get_leaf_counts() == counts
        assert gt.abundance(1, 0)["n_units"] == len(pairs)                    # units are fragments
        for iters in (3, 200):
            same(gt.abundance(iters, 0), abund_ref.estimate(log, iters, 0), (thr, mode, iters))
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 6. a block that ran twice is logged once
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 1])
def test_hit_buffer_retry_logs_once(fam, path):
    gt, thr = fam.gt, 1.0
    gt.reset_counts()
    gt.set_path(path)
    gt.set_option("PFQ_HIT_SLOTS", "0")
    try:
        log_reads(gt, fam.reads, thr)
        c = gt.last_capacity()
        assert c["attempts"] == 2 and c["hit_cap"] == 0 < c["hit_cursor"], c
        est = gt.abundance(9, 0)
        assert est["n_units"] == len(fam.reads)
        same(est, expect(fam.rows(thr), 16, 9, 0), path)
        pairs = make_pairs(fam)[:200]
        gt.abundance_reset()
        gt.query_pairs([p[0] for p in pairs], [p[1] for p in pairs], thr, abundance=True)
        assert gt.last_capacity()["attempts"] == 2 and gt.abundance(1, 0)["n_units"] == 200
    finally:
        gt.set_option("PFQ_HIT_SLOTS", None)
        gt.set_path(-1)
        gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 7. lifecycle
# ---------------------------------------------------------------------------------------------------------------
def test_lifecycle(gpu, tmp_path):
    rng = np.random.default_rng(31)
    genomes = strain_families(rng, 2, 3, 2000, 0.006, 3)
    ids = [f"S{i:02d}" for i in range(len(genomes))]
    n0 = len(genomes) - 1
    ot = orc.build_greedy_tree(genomes[:n0], ids[:n0], K, 0.001, 2000, *SEEDS)
    gt = BloomTree.new(K, 0.001, 2000, *SEEDS)
    try:
        for g, i in zip(genomes[:n0], ids[:n0]):
            gt.insert(g, i)
        assert is_empty(gt.abundance(), n0)                                   # nothing logged yet
        reads = reads_from(rng, genomes, [0, 3, 6], 600, 100) + [_dna(rng, 100) for _ in range(30)] + [b"ACGT"]
        rows = rows_of(oracle_sets(ot, reads, 1.0))
        want = expect(rows, n0, 50, 0)
        assert want["n_ambiguous"] >= 100
        log_reads(gt, reads, 1.0)
        first = gt.abundance(50, 0)
        same(first, want, "first")
        same(gt.abundance(50, 0), want, "estimating again")                   # the log is not consumed
        seq, off = pack_reads(reads)
        gt.query_packed(seq, off, 1.0, want_hits=True)                        # a call without the flag logs nothing
        gt.query_packed(seq, off, 1.0)
        same(gt.abundance(50, 0), want, "after calls without the flag")
        log_reads(gt, reads[:100], 1.0)                                       # and more may follow an estimate
        same(gt.abundance(50, 0), expect(rows + rows[:100], n0, 50, 0), "more rows")
        counts = gt.get_leaf_counts()
        gt.abundance_reset()                                                  # clears the log, not the leaf counters
        assert is_empty(gt.abundance(), n0) and gt.get_leaf_counts() == counts
        # the log is not stored
        log_reads(gt, reads, 1.0)
        d = str(tmp_path / "db")
        gt.save(d)
        t2 = BloomTree.load(d)
        assert is_empty(t2.abundance(), n0)
        t2.close()
        # pfq_leaf_counts_reset
        gt.reset_counts()
        assert is_empty(gt.abundance(), n0)
        # insert: the leaf columns change meaning
        log_reads(gt, reads, 1.0)
        assert gt.abundance(1, 0)["n_units"] == len(reads)
        gt.insert(genomes[n0], ids[n0])
        orc.greedy_insert(ot, genomes[n0], ids[n0])
        orc.renumber_preorder(ot)
        assert is_empty(gt.abundance(), n0 + 1)
        rows = rows_of(oracle_sets(ot, reads, 1.0))
        log_reads(gt, reads, 1.0)
        same(gt.abundance(50, 0), expect(rows, n0 + 1, 50, 0), "after insert")
        # prune
        gt.prune_tree(2)
        ot.prune(2)
        nl = len(ot.leaves_dfs())
        assert nl < n0 + 1 and is_empty(gt.abundance(), nl)
        rows = rows_of(oracle_sets(ot, reads, 1.0))
        log_reads(gt, reads, 1.0)
        same(gt.abundance(50, 0), expect(rows, nl, 50, 0), "after prune")
        # documented errors
        L, hits = _ffi.lib(), _ffi.Hits()
        seq, off = pack_reads(reads[:50])
        before = gt.abundance(3, 0)
        for flags in (_ffi.WANT_ABUNDANCE, _ffi.WANT_ABUNDANCE | _ffi.WANT_LCA, _ffi.WANT_ABUNDANCE | _ffi.PAIRED):
            rc = L.pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, 50, 1.0, flags, C.byref(hits))
            assert rc == PFQ_ERR_ARG and b"PFQ_WANT_ABUNDANCE" in L.pfq_last_error(), flags
        same(gt.abundance(3, 0), before, "refused calls log nothing")
        with pytest.raises(PfqError) as e:
            gt.abundance(0, 0)
        assert e.value.code == PFQ_ERR_ARG
        assert L.pfq_abundance_estimate(gt._h, 5, 0, None) == PFQ_ERR_ARG
        # a subtree shard sees only its own leaves
        shard = BloomTree.load_subtree(d, 1, 0)
        try:
            with pytest.raises(PfqError) as e:
                log_reads(shard, reads[:50], 1.0)
            assert e.value.code == PFQ_ERR_UNSUPPORTED and "shard" in str(e.value)
            assert shard.query_packed(seq, off, 1.0, want_hits=True) is not None   # it still answers without the flag
            with pytest.raises(PfqError) as e:
                gt.abundance_absorb(shard)
            assert e.value.code == PFQ_ERR_ARG
        finally:
            shard.close()
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. absorb
# ---------------------------------------------------------------------------------------------------------------
def test_absorb(fam):
    thr = 0.5
    a, b = fam.new_tree(), fam.new_tree()
    try:
        n = len(fam.reads)
        log_reads(a, fam.reads[:n // 2], thr)
        log_reads(b, fam.reads[n // 2:], thr)
        counts_b = b.get_leaf_counts()
        same(b.abundance(9, 0), expect(fam.rows(thr)[n // 2:], 16, 9, 0), "b alone")
        a.abundance_absorb(b)
        same(a.abundance(200, 0), expect(fam.rows(thr), 16, 200, 0), "absorbed")
        assert is_empty(b.abundance(), 16) and b.get_leaf_counts() == counts_b
        a.abundance_absorb(b)                                                 # an empty log adds nothing
        same(a.abundance(9, 0), expect(fam.rows(thr), 16, 9, 0), "absorbed an empty log")
        log_reads(b, fam.reads[:100], thr)                                    # both go on logging
        log_reads(a, fam.reads[100:200], thr)
        a.abundance_absorb(b)
        same(a.abundance(9, 0), expect(fam.rows(thr) + fam.rows(thr)[:200], 16, 9, 0), "absorbed again")
        with pytest.raises(PfqError) as e:
            a.abundance_absorb(a)
        assert e.value.code == PFQ_ERR_ARG
        small = BloomTree.build_balanced(fam.genomes[:8], fam.ids[:8], K, NBITS, H, *SEEDS)
        try:
            with pytest.raises(PfqError) as e:
                a.abundance_absorb(small)
            assert e.value.code == PFQ_ERR_ARG and "replicas" in str(e.value)
        finally:
            small.close()
    finally:
        a.close()
        b.close()
