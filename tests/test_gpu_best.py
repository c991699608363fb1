"""PFQ_ROWS_BEST: the taxonomy, the abundance log and the coverage sketch take every unit's best-scoring genomes,
B(u) = the entries of its row whose score is the row's highest, and last_best_rows() gives those rows.

Nothing expected here comes from the library.  The rows are the oracle's (oracle_sets; fragments: combine), the scores are
expected_scores / pair_scores, the reduction is best_sets of tests/test_gpu_lca.py, and the consumers' expectations are
tax_ref.Nodes.counts, abund_ref.classify + estimate and cover_ref.TreeSketcher fed the best rows.  Every comparison is exact
and covers every unit.  Everything else of a flagged call — leaf counts, CSR, scores, statistics, clade counts and LCAs — must
be what the same call gives without the flag.  Workload W and its helpers are those of tests/test_gpu_lca.py."""
import ctypes as C

import numpy as np
import pytest

import abund_ref
import cover_ref
import tax_ref
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_abund import same as same_abundance
from test_gpu_build import _dna, _mutate
from test_gpu_cover import same as same_coverage
from test_gpu_lca import K, Device, W, best_sets, csr_of, knobs, oracle_sets, pair_scores
from test_gpu_paired import combine
from test_gpu_parity import gpu_tree, oracle_tree
from test_gpu_scores import Contains, expected_scores
from test_gpu_tax import random_taxonomy, stats_of

pytestmark = pytest.mark.gpu

PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED = -1, -4
TAX_SEED = 101
N_LEAVES = 80


class ProbeContains(Contains):
    """Contains.count for many leaves per read: the oracle's probe indices of every distinct k-mer of `reads` are taken once
    (orc.probe_indices), and a filter row answers all of them with one gather of its bits (Lsb0 words, as the oracle's
    bf_contains reads them).  θ 0 scores every read on all 80 leaves: k-mer by k-mer that is a minute, this way seconds.
    test_w_expectations checks it against Contains itself."""

    def __init__(self, ot, reads):
        super().__init__(ot)
        self.ids, probes = {}, []
        for x in reads:
            for c in orc.get_kmers(x, ot.kmer_size):
                if c not in self.ids:
                    self.ids[c] = len(probes)
                    probes.append(orc.probe_indices(ot.seed1, ot.seed2, ot.num_hashes, ot.nbits, c))
        self.probes = np.array(probes, dtype=np.uint64).reshape(len(probes), ot.num_hashes)
        self.member, self.last, self.last_ids = {}, None, None

    def count(self, r, kmers):
        if not len(kmers):
            return 0
        if r not in self.member:
            w = np.asarray(self.ot.bits[r], dtype=np.uint64)
            self.member[r] = ((w[self.probes >> np.uint64(6)] >> (self.probes & np.uint64(63))) & np.uint64(1)).all(axis=1)
        if kmers is not self.last:                                    # (expected_scores hands one list per read, leaf after leaf)
            self.last, self.last_ids = kmers, np.array([self.ids[c] for c in kmers], dtype=np.int64)
        return int(self.member[r][self.last_ids].sum())


class BW:
    """Workload W with the references over best rows, each computed once and left unchanged."""

    def __init__(self):
        self.w = W()
        w = self.w
        self.gt, self.ot = w.gt, w.ot
        self.probe = ProbeContains(w.ot, w.reads)
        self.tax = random_taxonomy(TAX_SEED, N_LEAVES)
        self.ref = tax_ref.Nodes([w.ot.tax_id[v] for v in w.ot.leaves_dfs()], *self.tax)   # (leaf order, not the order of insertion)
        self.cache = cover_ref.TreeSketcher(w.ot)                     # (only its memory of the oracle's answers is used)
        self._scores, self._best, self._want = {}, {}, {}

    def scores(self, thr):
        if thr not in self._scores:
            offs, leaves = csr_of(self.w.sets(thr))
            self._scores[thr] = expected_scores(self.ot, self.w.reads, offs, leaves, self.probe)
        return self._scores[thr]

    def best(self, thr):
        if thr not in self._best:
            self._best[thr] = best_sets(self.w.sets(thr), self.scores(thr))
        return self._best[thr]

    def want(self, thr):
        if thr not in self._want:
            self._want[thr] = Want(self, self.best(thr), reads=self.w.reads)
        return self._want[thr]


class Want:
    """What the three consumers must hold after one call whose units have the rows `sets`."""

    def __init__(self, bw, sets, reads=None, pairs=None):
        rows = [sorted(s) for s in sets]
        self.csr = csr_of(sets)
        self.taxa = bw.ref.counts(sets)
        self.log = abund_ref.classify(rows, N_LEAVES)
        self.est = abund_ref.estimate(self.log, 200, 0)
        sk = cover_ref.TreeSketcher(bw.ot, share=bw.cache)
        self.sketch = sk.add_pairs(rows, pairs) if pairs is not None else sk.add_reads(rows, reads)


@pytest.fixture(scope="module")
def bw(gpu):
    x = BW()
    x.gt.set_taxonomy(*x.tax)
    assert x.gt.taxa() == x.ref.table
    yield x
    x.gt.close()


def call(gt, seq, off, thr, *, dev=None, paired=False, mode="either", **kw):
    """One call with hits and scores through the host entry or (dev) the device-resident one: the CSR and the scores as copies."""
    if dev is None:
        return gt.query_packed(seq, off, thr, want_hits=True, want_scores=True, paired=paired, pair_mode=mode, **kw)
    res = gt.query_device_hits(dev.seq.ptr, dev.off.ptr, dev.n, dev.total, thr, stream=dev.stream, want_scores=True, paired=paired,
                               pair_mode=mode, **kw)
    return tuple(np.array(a) for a in res)


def observe(gt, lca):
    out = {"counts": gt.get_leaf_counts(), "stats": stats_of(gt)}
    if lca:
        out["clades"] = gt.clade_counts()
        out["lca"] = gt.last_lca()
    return out


def same_call(a, b, res_a, res_b, tag):
    """Two calls' own results: CSR, scores, leaf counts, statistics, and the clade side where it was asked for."""
    assert len(res_a) == len(res_b) == 3 and all(np.array_equal(x, y) for x, y in zip(res_a, res_b)), tag
    assert a["counts"] == b["counts"] and a["stats"] == b["stats"], tag
    if "lca" in a:
        assert np.array_equal(a["lca"], b["lca"]), tag
        assert all(np.array_equal(x, y) for x, y in zip(a["clades"], b["clades"])), tag


def check_best_rows(gt, want_csr, tag):
    offs, leaves = gt.last_best_rows()
    w_offs, w_leaves = want_csr
    assert offs.dtype == np.uint64 and leaves.dtype == np.uint32, tag
    assert np.array_equal(offs, w_offs), (tag, np.flatnonzero(offs != w_offs)[:10] if offs.shape == w_offs.shape else (offs.shape, w_offs.shape))
    assert np.array_equal(leaves, w_leaves), tag


def check_consumers(gt, want, tag):
    """last_best_rows(), the taxon counters, the abundance estimate and the coverage sketch against a Want."""
    check_best_rows(gt, want.csr, tag)
    w_last, w_here, w_below, w_any = want.taxa
    last = gt.last_taxa()
    assert last.dtype == np.uint32 and np.array_equal(last, w_last), (tag, np.flatnonzero(last != w_last)[:10])
    here, below, any_ = gt.taxon_counts()
    for name, got, exp in (("here", here, w_here), ("below", below, w_below), ("any", any_, w_any)):
        assert np.array_equal(got, exp), (tag, name, np.flatnonzero(got != exp)[:10])
    same_abundance(gt.abundance(200, 0), want.est, tag)
    same_coverage(gt.coverage(), want.sketch, tag)


def flagged_against_plain(gt, seq, off, thr, want, tag, **kw):
    """The call with the flag and all three consumers against the references over best rows and against the same call
    without the flag; then the flag beside both kinds of LCA, against the same calls without it."""
    gt.reset_counts()
    p_res = call(gt, seq, off, thr, **kw)
    plain = observe(gt, None)
    gt.reset_counts()
    res = call(gt, seq, off, thr, taxa=True, abundance=True, coverage=True, best=True, **kw)
    same_call(observe(gt, None), plain, res, p_res, tag)
    check_consumers(gt, want, tag)
    for lca in ("all", "best"):
        gt.reset_counts()
        l_res = call(gt, seq, off, thr, lca=lca, **kw)
        without = observe(gt, lca)
        gt.reset_counts()
        res = call(gt, seq, off, thr, lca=lca, best=True, **kw)
        same_call(observe(gt, lca), without, res, l_res, (tag, lca))
        same_call(observe(gt, None), plain, res, p_res, (tag, lca, "plain"))
        check_best_rows(gt, want.csr, (tag, lca))
    gt.reset_counts()
    return p_res


# ---------------------------------------------------------------------------------------------------------------
# 1. workload W
# ---------------------------------------------------------------------------------------------------------------
def test_w_expectations(bw):
    """Asserted on the references alone: the reduction bites, ties stay, and the fast scorer is the oracle's."""
    w = bw.w
    offs, leaves = csr_of(w.sets(0.7))
    n = 400
    cut = int(offs[n])
    assert np.array_equal(bw.scores(0.7)[:cut], expected_scores(bw.ot, w.reads[:n], offs[:n + 1], leaves[:cut], w.contains))
    for thr in (0.7, 0.3):
        sets, best = w.sets(thr), bw.best(thr)
        n_hit = sum(1 for s in sets if s)
        differ = sum(1 for s, b in zip(sets, best) if s != b)
        ties = sum(1 for b in best if len(b) > 1)
        whole_here = bw.ref.counts(sets)[1]
        whole_log = abund_ref.classify([sorted(s) for s in sets], N_LEAVES)
        want = bw.want(thr)
        print(f"theta {thr}: hit {n_hit} best differs {differ} ties {ties} ambiguous {whole_log['n_ambiguous']} -> {want.log['n_ambiguous']}")
        assert all(b <= s and bool(b) == bool(s) for s, b in zip(sets, best))
        assert differ >= 0.2 * n_hit and ties >= 0.25 * n_hit
        assert not np.array_equal(want.taxa[1], whole_here)
        assert want.log["n_ambiguous"] < whole_log["n_ambiguous"]


@pytest.mark.parametrize("path", [0, 1])
def test_w_paths_thresholds_entries(bw, path):
    """θ 0.7 and 0.3 x forced path x host / device-resident entry."""
    gt, w = bw.gt, bw.w
    knobs(gt, path, None)
    dev = Device(w.seq, w.off)
    try:
        for thr in (0.7, 0.3):
            for d in (None, dev):
                res = flagged_against_plain(gt, w.seq, w.off, thr, bw.want(thr), (path, thr, d is not None), dev=d)
                assert np.array_equal(res[2], bw.scores(thr)), (path, thr)    # (the scores the reduction read are the oracle's)
    finally:
        dev.close()
        knobs(gt, -1, None)


# ---------------------------------------------------------------------------------------------------------------
# 2. the ends of the threshold range
# ---------------------------------------------------------------------------------------------------------------
def test_w_threshold_one_changes_nothing(bw):
    gt, w = bw.gt, bw.w
    sets = w.sets(1.0)
    assert bw.best(1.0) == sets                                       # every listed leaf scores n_kmers
    flagged_against_plain(gt, w.seq, w.off, 1.0, bw.want(1.0), 1.0)
    got = {}
    for best in (False, True):
        gt.reset_counts()
        call(gt, w.seq, w.off, 1.0, taxa=True, abundance=True, coverage=True, best=best)
        got[best] = (gt.last_taxa(), gt.taxon_counts(), gt.abundance(200, 0), gt.coverage())
    assert np.array_equal(got[True][0], got[False][0])
    assert all(np.array_equal(a, b) for a, b in zip(got[True][1], got[False][1]))
    same_abundance(got[True][2], got[False][2])
    assert all(np.array_equal(got[True][3][k], got[False][3][k]) for k in ("registers", "units", "matched"))
    gt.reset_counts()


def test_w_threshold_zero_reduces_whole_leaf_rows(bw):
    """Every row lists all 80 leaves: every row goes to a wave, and only the units without k-mers keep them all."""
    gt, w = bw.gt, bw.w
    sets, best = w.sets(0.0), bw.best(0.0)
    assert all(len(s) == N_LEAVES for s in sets)
    short = [i for i, r in enumerate(w.reads) if len(r) < K]
    assert {w.reads[i] for i in short} >= {b"", b"ACGT"}
    assert all(len(best[i]) == N_LEAVES for i in short)
    assert all(len(best[i]) < N_LEAVES for i in range(3000))           # the reads drawn from the genomes: the top scorers only
    want = bw.want(0.0)
    assert want.log["n_all_leaves"] >= len(short) and want.log["n_unhit"] == 0
    flagged_against_plain(gt, w.seq, w.off, 0.0, want, 0.0)


# ---------------------------------------------------------------------------------------------------------------
# 3. rows of exactly 64, 65 and 130 entries
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_leaves", [64, 65, 130])
def test_row_length_boundaries(gpu, n_leaves):
    """θ 0 on balanced trees: 64 entries are the last row a thread takes, 65 the first a wave takes (one entry in its second
    chunk), 130 three chunks with the running base.  Mutated copies far apart in leaf order tie across the chunks."""
    rng = np.random.default_rng(6400 + n_leaves)
    genomes = [_dna(rng, 400) for _ in range(n_leaves)]
    copies = [(n_leaves - 1, 3), (n_leaves // 2, 10), (5, n_leaves - 2)]
    for dst, src in copies:
        genomes[dst] = _mutate(rng, genomes[src], 2)
    genomes[7] = genomes[n_leaves - 3]                                # an exact copy: ties on every read of it
    nbits, h = 20011, 4
    ot, ids = oracle_tree(genomes, K, nbits, h)
    gt = gpu_tree(genomes, ids, K, nbits, h)
    try:
        reads = []
        for i in range(36):
            g = genomes[[3, 10, n_leaves - 2, n_leaves - 3, int(rng.integers(0, n_leaves))][i % 5]]
            o = int(rng.integers(0, 400 - 120))
            r = g[o:o + 120]
            reads.append(orc.revcomp(r) if i % 2 else r)
        reads += [_dna(rng, 120), _dna(rng, 120), b"", b"ACGT"]
        sets = oracle_sets(ot, reads, 0.0)
        assert all(len(s) == n_leaves for s in sets)
        offs, leaves = csr_of(sets)
        best = best_sets(sets, expected_scores(ot, reads, offs, leaves))
        assert sum(1 for b in best if len(b) > 1) >= 10 and sum(1 for b in best if len(b) == 1) >= 3
        assert sum(1 for b in best if len(b) == n_leaves) >= 2       # the reads without k-mers: whole rows kept
        if n_leaves > 64:
            assert any(min(b) < 64 <= max(b) for b in best if len(b) < n_leaves)   # a tie across the first chunk's end
        seq, off = pack_reads(reads)
        for path in (0, 1):
            gt.set_path(path)
            res = gt.query_packed(seq, off, 0.0, want_hits=True, want_scores=True, best=True)
            assert np.array_equal(res[0], offs) and np.array_equal(res[1], leaves)
            check_best_rows(gt, csr_of(best), (n_leaves, path))
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. fragments
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["either", "both"])
def test_w_fragments(bw, mode):
    gt, w = bw.gt, bw.w
    pairs, preads = w.pairs(), w.pair_reads()
    seq, off = pack_reads(preads)
    frag = combine(w.pair_sets(0.7), mode)
    best = best_sets(frag, pair_scores(bw.ot, preads, frag, w.contains))
    assert sum(1 for s, b in zip(frag, best) if s != b) >= 0.2 * sum(1 for s in frag if s)
    assert sum(1 for b in best if len(b) == N_LEAVES) >= 2            # all-leaf fragments stay whole: their scores are all 0 ...
    if mode == "either":                                              # ... unless one mate has k-mers: then the top scorers only
        assert any(len(s) == N_LEAVES and len(b) < N_LEAVES for s, b in zip(frag, best))
    want = Want(bw, best, pairs=pairs)
    flagged_against_plain(gt, seq, off, 0.7, want, mode, paired=True, mode=mode)


# ---------------------------------------------------------------------------------------------------------------
# 5. call split and the overflow retry
# ---------------------------------------------------------------------------------------------------------------
def test_call_split_and_overflow_retry(bw):
    gt, w = bw.gt, bw.w
    thr, want = 0.7, bw.want(0.7)
    n = len(w.reads)
    kw = dict(taxa=True, abundance=True, coverage=True, best=True)
    gt.reset_counts()
    best = bw.best(thr)
    for lo, hi in ((0, n // 7), (n // 7, n // 2), (n // 2, n)):
        seq, off = pack_reads(w.reads[lo:hi])
        call(gt, seq, off, thr, **kw)
        check_best_rows(gt, csr_of(best[lo:hi]), (lo, hi))
        assert np.array_equal(gt.last_taxa(), want.taxa[0][lo:hi])
    here, below, any_ = gt.taxon_counts()
    assert np.array_equal(here, want.taxa[1]) and np.array_equal(below, want.taxa[2]) and np.array_equal(any_, want.taxa[3])
    same_abundance(gt.abundance(200, 0), want.est, "split")
    same_coverage(gt.coverage(), want.sketch, "split")
    for path in (0, 1):
        knobs(gt, path, None)
        gt.set_option("PFQ_HIT_SLOTS", "100")
        try:
            gt.reset_counts()
            call(gt, w.seq, w.off, thr, **kw)
            c = gt.last_capacity()
            assert c["attempts"] == 2 and c["hit_cap"] == 100 < c["hit_cursor"], (path, c)
            check_consumers(gt, want, ("retry", path))
        finally:
            gt.set_option("PFQ_HIT_SLOTS", None)
            knobs(gt, -1, None)
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 6. arguments and state
# ---------------------------------------------------------------------------------------------------------------
def test_documented_error_codes_and_the_flag_alone(bw, tmp_path):
    gt, w = bw.gt, bw.w
    reads = w.reads[:60]
    seq, off = pack_reads(reads)
    L, hits = _ffi.lib(), _ffi.Hits()
    for flags in (_ffi.ROWS_BEST, _ffi.ROWS_BEST | _ffi.WANT_HITS, _ffi.ROWS_BEST | _ffi.WANT_SCORES,
                  _ffi.ROWS_BEST | _ffi.WANT_HITS | _ffi.WANT_TAXA):
        rc = L.pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, len(reads), 0.7, flags, C.byref(hits))
        assert rc == PFQ_ERR_ARG and b"PFQ_ROWS_BEST" in L.pfq_last_error(), flags
        with pytest.raises(PfqError) as e:
            gt.last_best_rows()
        assert e.value.code == PFQ_ERR_ARG
    for kw in (dict(want_hits=True), dict(want_scores=True), dict()):
        with pytest.raises(ValueError):
            gt.query_packed(seq, off, 0.7, best=True, **kw)
    # the flag alone with hits and scores: accepted, and no counter, log or sketch moves
    gt.reset_counts()
    plain = call(gt, seq, off, 0.7)
    counts = gt.get_leaf_counts()
    before = (gt.taxon_counts(), gt.abundance(10, 0), gt.coverage())
    gt.reset_counts()
    res = call(gt, seq, off, 0.7, best=True)
    assert all(np.array_equal(a, b) for a, b in zip(res, plain)) and gt.get_leaf_counts() == counts
    sets = w.sets(0.7)[:60]
    check_best_rows(gt, csr_of(bw.best(0.7)[:60]), "alone")
    assert any(s != b for s, b in zip(sets, bw.best(0.7)[:60]))
    after = (gt.taxon_counts(), gt.abundance(10, 0), gt.coverage())
    assert all(not x.any() for x in after[0]) and all(np.array_equal(a, b) for a, b in zip(after[0], before[0]))
    same_abundance(after[1], before[1])
    assert after[1]["n_units"] == 0 and after[2]["n_units"] == 0 and not after[2]["units"].any()
    with pytest.raises(PfqError) as e:                                # (asked for none of them)
        gt.last_taxa()
    assert e.value.code == PFQ_ERR_ARG
    # a call without the flag, and a frames call, end the validity
    call(gt, seq, off, 0.7)
    with pytest.raises(PfqError) as e:
        gt.last_best_rows()
    assert e.value.code == PFQ_ERR_ARG and "PFQ_ROWS_BEST" in str(e.value)
    call(gt, seq, off, 0.7, best=True)
    assert len(gt.last_best_rows()[0]) == 61
    gt.query_frames(seq, off, 100, 50, 0.7)
    with pytest.raises(PfqError) as e:
        gt.last_best_rows()
    assert e.value.code == PFQ_ERR_ARG
    # an empty call: no unit, no row
    e_seq, e_off = pack_reads([])
    call(gt, e_seq, e_off, 0.7, best=True)
    offs, leaves = gt.last_best_rows()
    assert offs.tolist() == [0] and leaves.size == 0
    gt.reset_counts()
    # a subtree shard sees partial rows — with coverage too, which otherwise accepts shards
    d = str(tmp_path / "db")
    gt.save(d)
    shard = BloomTree.load_subtree(d, 2, 1)
    try:
        for kw in (dict(), dict(coverage=True)):
            with pytest.raises(PfqError) as e:
                shard.query_packed(seq, off, 0.7, want_hits=True, want_scores=True, best=True, **kw)
            assert e.value.code == PFQ_ERR_UNSUPPORTED and "shard" in str(e.value) and "PFQ_ROWS_BEST" in str(e.value)
        assert len(shard.query_packed(seq, off, 0.7, want_hits=True, want_scores=True, coverage=True)) == 3
    finally:
        shard.close()


def test_text_entry_and_conveniences(bw):
    """Through pfq_text_query, query_pairs and query_batch."""
    from phagefilter_amd.query import query_batch
    gt, w = bw.gt, bw.w
    n = 400
    text = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(w.reads[:n]))
    assert gt.parse_text(text, "fasta")["n_records"] == n
    gt.reset_counts()
    res = gt.query_text(0.7, want_hits=True, want_scores=True, taxa=True, abundance=True, coverage=True, best=True)
    assert np.array_equal(res[0], csr_of(w.sets(0.7)[:n])[0])
    check_consumers(gt, Want(bw, bw.best(0.7)[:n], reads=w.reads[:n]), "text")
    gt.reset_counts()
    query_batch(gt, w.reads[:n], 0.7, best=True)
    check_best_rows(gt, csr_of(bw.best(0.7)[:n]), "query_batch")
    pairs = w.pairs()[:100]
    preads = [m for p in pairs for m in p]
    frag = combine(w.pair_sets(0.7), "both")[:100]
    gt.reset_counts()
    rows = gt.query_pairs([p[0] for p in pairs], [p[1] for p in pairs], 0.7, mode="both", best=True)
    assert [set(r) for r in rows] == frag
    check_best_rows(gt, csr_of(best_sets(frag, pair_scores(bw.ot, preads, frag, w.contains))), "query_pairs")
    gt.reset_counts()
