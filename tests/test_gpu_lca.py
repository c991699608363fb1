"""PFQ_WANT_LCA / PFQ_LCA_BEST: every unit (a read; with PFQ_PAIRED a fragment) is assigned to the lowest common ancestor of
the leaves of its hit set, as a clade index (clades = nodes reachable from the root, pre-order), and the clade counters count
units at their LCA (`here`) and at or below a clade (`below`).

Nothing expected here comes from the library.  The hit sets are the oracle's (orc.query_batch; fragments combined from the
mates' sets as tests/test_gpu_paired.py does; scores from tests/test_gpu_scores.py's k-mer by k-mer count), the clades come
from a pre-order walk of the oracle tree's left / right / root, and the LCA of a set is found naively: walk up the parents
until the set meets.  Every case asserts last_lca() == expected per unit, here == the histogram of expected, below == its
subtree sums, and that leaf counts, hit CSR and scores equal those of the same call without the new flags."""
import os
import shutil

import numpy as np
import pytest

from hipbuf import DeviceBuffer, stream_create, stream_destroy, stream_synchronize
from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_build import SEEDS, _dna, _mutate, _one_child_db
from test_gpu_paired import combine, mate_sets
from test_gpu_parity import RNG, gpu_tree, make_reads, oracle_tree, rand_dna
from test_gpu_scores import Contains, expected_scores
from test_gpu_two_level import _genomes, _random_shape_tree
from test_gpu_wide_and_shards import _h4_tree

pytestmark = pytest.mark.gpu

NO = _ffi.NO_CLADE
PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED = -1, -4
K = 21


# ---------------------------------------------------------------------------------------------------------------
# the clades of an oracle tree and the naive LCA
# ---------------------------------------------------------------------------------------------------------------
class Clades:
    """Pre-order numbering of the nodes reachable from the oracle tree's root (node, left, right), parents, depths, leaf
    ranges and names; lca() walks up parent pointers."""

    def __init__(self, ot):
        self.idx, self.par, self.dep, self.nodes = {}, [], [], []
        self.memo = {}
        st = [(ot.root, -1, 0)] if ot.root >= 0 else []
        while st:
            v, p, d = st.pop()
            self.idx[v] = len(self.nodes)
            self.nodes.append(v)
            self.par.append(p)
            self.dep.append(d)
            if ot.right[v] >= 0:
                st.append((ot.right[v], self.idx[v], d + 1))
            if ot.left[v] >= 0:
                st.append((ot.left[v], self.idx[v], d + 1))
        self.leaf_clade = [self.idx[v] for v in ot.leaves_dfs()]
        self.is_leaf = set(self.leaf_clade)
        first, count = [None] * len(self.nodes), [0] * len(self.nodes)
        for col, c in enumerate(self.leaf_clade):                   # every ancestor-or-self of a leaf holds its column
            while c >= 0:
                first[c] = col if first[c] is None else min(first[c], col)
                count[c] += 1
                c = self.par[c]
        names = [ot.tax_id[v] if ot.tax_id[v] is not None else os.path.basename(ot.bf_path[v])[:-len(".bf")] for v in self.nodes]
        self.table = [(self.par[c], self.dep[c], first[c], count[c], names[c]) for c in range(len(self.nodes))]
        self.top = self.lca(range(len(self.leaf_clade))) if self.leaf_clade else NO

    def lca(self, cols):
        """Deepest clade that is an ancestor-or-self of every leaf column in `cols`; NO for none."""
        cl = tuple(self.leaf_clade[c] for c in cols)
        if not cl:
            return NO
        if cl in self.memo:                                         # (the reads that hit every leaf share one set)
            return self.memo[cl]
        a = cl[0]
        for b in cl[1:]:
            while a != b:
                if self.dep[a] >= self.dep[b]:
                    a = self.par[a]
                else:
                    b = self.par[b]
        self.memo[cl] = a
        return a

    def expected(self, sets):
        return np.array([self.lca(sorted(s)) for s in sets], dtype=np.uint32)

    def here_below(self, lcas):
        here = np.zeros(len(self.nodes), dtype=np.uint64)
        for c in lcas:
            if c != NO:
                here[int(c)] += 1
        below = here.copy()
        for c in range(len(self.nodes) - 1, 0, -1):
            below[self.par[c]] += below[c]
        return here, below


def oracle_sets(ot, reads, thr):
    """Per read its set of leaf columns, from the oracle's query_batch."""
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    ohits, _, _ = orc.query_batch(ot, reads, thr, threads=8)
    col = {v: i for i, v in enumerate(ot.leaves_dfs())}
    sets = [set() for _ in reads]
    for r, v in ohits:
        sets[r].add(col[v])
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    return sets


def csr_of(sets):
    offs = np.zeros(len(sets) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in sets])
    leaves = np.array([c for s in sets for c in sorted(s)], dtype=np.uint32)
    return offs, leaves


def best_sets(sets, scores):
    """Every unit's set reduced to the entries with its highest score (`scores` aligned with the CSR of `sets`)."""
    out, j = [], 0
    for s in sets:
        cols = sorted(s)
        sc = [int(x) for x in scores[j:j + len(cols)]]
        j += len(cols)
        out.append({c for c, x in zip(cols, sc) if x == max(sc)} if cols else set())
    return out


def pair_scores(ot, reads, frag_sets, contains):
    """Per (fragment, listed leaf): both mates' matched k-mers on that leaf's filter, summed (as check_pairs counts them)."""
    col_row = [ot.filter_of[v] for v in ot.leaves_dfs()]
    out = []
    for f, s in enumerate(frag_sets):
        if not s:
            continue
        k1, k2 = orc.get_kmers(reads[2 * f], ot.kmer_size), orc.get_kmers(reads[2 * f + 1], ot.kmer_size)
        out += [contains.count(col_row[c], k1) + contains.count(col_row[c], k2) for c in sorted(s)]
    return np.array(out, dtype=np.int64)


class Device:
    """A block resident in HBM and a non-default stream for the device-resident entry."""

    def __init__(self, seq, off):
        self.seq, self.off = DeviceBuffer.from_numpy(seq), DeviceBuffer.from_numpy(off)
        self.n, self.total = len(off) - 1, int(off[-1])
        self.stream = stream_create()

    def close(self):
        stream_synchronize(self.stream)
        stream_destroy(self.stream)
        self.seq.free()
        self.off.free()


def call(gt, seq, off, thr, *, hits, lca=None, scores=False, paired=False, mode="either", dev=None):
    """One query call through the host entry, or (dev) the device-resident entry on the device's own stream.  Returns the
    CSR (and scores) as copies, or None."""
    if dev is None:
        return gt.query_packed(seq, off, thr, want_hits=hits, want_scores=scores, paired=paired, pair_mode=mode, lca=lca)
    if not hits:
        gt.query_device(dev.seq.ptr, dev.off.ptr, dev.n, dev.total, thr, stream=dev.stream, paired=paired, pair_mode=mode, lca=lca)
        return None
    res = gt.query_device_hits(dev.seq.ptr, dev.off.ptr, dev.n, dev.total, thr, stream=dev.stream, want_scores=scores,
                               paired=paired, pair_mode=mode, lca=lca)
    return tuple(np.array(a) for a in res)


def check(gt, cm, seq, off, thr, want_sets, *, hits, lca="all", scores=False, paired=False, mode="either", dev=None, tag=None):
    """The call with the LCA flags against the same call without them (leaf counts, CSR, scores) and against the expected
    LCAs of `want_sets` (per unit, the set the LCA is taken over); the counters start from zero.  Returns the LCAs."""
    kw = dict(hits=hits, scores=scores, paired=paired, mode=mode, dev=dev)
    gt.reset_counts()
    plain = call(gt, seq, off, thr, **kw)
    counts = gt.get_leaf_counts()
    gt.reset_counts()
    res = call(gt, seq, off, thr, lca=lca, **kw)
    got = gt.last_lca()
    assert gt.get_leaf_counts() == counts, tag
    assert (plain is None) == (res is None), tag
    if res is not None:
        assert len(res) == len(plain) and all(np.array_equal(a, b) for a, b in zip(res, plain)), tag
    want = cm.expected(want_sets)
    assert got.dtype == np.uint32 and got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, bad[:10], got[bad[:10]], want[bad[:10]])
    here, below = gt.clade_counts()
    want_here, want_below = cm.here_below(want)
    assert np.array_equal(here, want_here) and np.array_equal(below, want_below), tag
    if len(below):
        assert int(below[0]) == int((want != NO).sum()), tag
        leaf_counts = [n for _, n in counts]
        assert all(int(here[c]) <= leaf_counts[col] for col, c in enumerate(cm.leaf_clade)), tag
    return got


# ---------------------------------------------------------------------------------------------------------------
# workload W: nested families on a greedy tree
# ---------------------------------------------------------------------------------------------------------------
def nested_families(rng, n_fam, sub_per_fam, strains_per_sub, length, sub_rate, strain_rate, singles):
    out = []
    for _ in range(n_fam):
        base = _dna(rng, length)
        for _ in range(sub_per_fam):
            sb = _mutate(rng, base, rng.binomial(length, sub_rate))
            for _ in range(strains_per_sub):
                out.append(_mutate(rng, sb, rng.binomial(length, strain_rate)))
    out += [_dna(rng, length) for _ in range(singles)]
    return [out[i] for i in rng.permutation(len(out))]


def w_reads(rng, genomes, n, length):
    out = []
    for i in range(n):
        g = genomes[int(rng.integers(0, len(genomes)))]
        o = int(rng.integers(0, len(g) - length + 1))
        r = g[o:o + length]
        if i % 3 == 0:
            r = _mutate(rng, r, 1 + i % 3)
        out.append(orc.revcomp(r) if rng.random() < 0.5 else r)
    out += [_dna(rng, length) for _ in range(n // 4)]
    return out + [b"", b"ACGT", _dna(rng, 20)]


class W:
    def __init__(self, device=True):
        rng = np.random.default_rng(7)
        self.genomes = nested_families(rng, 6, 3, 4, 3000, 0.03, 0.004, 8)
        self.ids = [f"G{i:04d}" for i in range(len(self.genomes))]
        self.ot = orc.build_greedy_tree(self.genomes, self.ids, K, 0.001, 3000, *SEEDS)
        self.gt = BloomTree.new(K, 0.001, 3000, *SEEDS) if device else None   # (None: the oracle's side only)
        for g, i in zip(self.genomes, self.ids):
            if device:
                self.gt.insert(g, i)
        self.cm = Clades(self.ot)
        self.reads = w_reads(rng, self.genomes, 3000, 150)
        self.seq, self.off = pack_reads(self.reads)
        self.rng = rng
        self._sets, self._pairs, self._pair_sets, self._scores = {}, None, {}, {}
        self.contains = Contains(self.ot)

    def sets(self, thr):
        if thr not in self._sets:
            self._sets[thr] = oracle_sets(self.ot, self.reads, thr)
        return self._sets[thr]

    def best(self, thr):
        """The reads' sets reduced to their best-scoring entries; the scores are the oracle's."""
        if thr not in self._scores:
            sets = self.sets(thr)
            offs, leaves = csr_of(sets)
            self._scores[thr] = expected_scores(self.ot, self.reads, offs, leaves, self.contains)
        return best_sets(self.sets(thr), self._scores[thr])

    def pairs(self):
        """Mates 150 bp apart on one genome (R2 reverse-complemented), cross-genome fragments, fragments with one short
        mate, foreign fragments."""
        if self._pairs is None:
            rng, g, pairs = self.rng, self.genomes, []
            for i in range(500):
                a = g[int(rng.integers(0, len(g)))]
                o = int(rng.integers(0, len(a) - 450))
                m1, m2 = a[o:o + 150], orc.revcomp(a[o + 300:o + 450])
                if i % 3 == 0:
                    m1 = _mutate(rng, m1, 1 + i % 2)
                pairs.append((m1, m2))
            for i in range(120):
                a, b = g[int(rng.integers(0, len(g)))], g[int(rng.integers(0, len(g)))]
                oa, ob = int(rng.integers(0, len(a) - 150)), int(rng.integers(0, len(b) - 150))
                pairs.append((a[oa:oa + 150], b[ob:ob + 150]))
            for i in range(60):
                a = g[int(rng.integers(0, len(g)))]
                o = int(rng.integers(0, len(a) - 150))
                short = [b"", b"ACGT", _dna(rng, K - 1)][i % 3]
                pairs.append((short, a[o:o + 150]) if i % 2 else (a[o:o + 150], short))
            pairs += [(_dna(rng, 150), _dna(rng, 150)) for _ in range(60)]
            pairs += [(b"", b""), (b"A", _dna(rng, K - 1))]
            self._pairs = [pairs[i] for i in rng.permutation(len(pairs))]
        return self._pairs

    def pair_reads(self):
        return [m for p in self.pairs() for m in p]

    def pair_sets(self, thr):
        if thr not in self._pair_sets:
            self._pair_sets[thr] = mate_sets(self.ot, self.pair_reads(), thr)
            for v in range(self.ot.n_nodes):
                self.ot.mapped_reads[v] = 0
        return self._pair_sets[thr]


@pytest.fixture(scope="module")
def w(gpu):
    x = W()
    yield x
    x.gt.close()


def knobs(gt, path, block):
    gt.set_path(path)
    gt.set_option("PFQ_BLOCK", block)


def test_w_clade_table_equals_the_oracles_preorder(w):
    assert w.gt.clades() == w.cm.table
    assert w.cm.top == 0 and len(w.cm.table) == 2 * len(w.genomes) - 1
    here, below = w.gt.clade_counts()
    assert not here.any() and not below.any() and len(here) == len(w.cm.table)


def test_w_coverage_conditions_on_the_expected_values(w):
    """What makes W a test of the LCA rather than of single hits: asserted on the oracle's values alone."""
    cm = w.cm
    exp = cm.expected(w.sets(1.0))
    hit = exp[exp != NO]
    internal = [int(c) for c in hit if int(c) not in cm.is_leaf]
    n_hit, n_int = len(hit), len(internal)
    print(f"theta 1.0: hit {n_hit} internal {n_int} leaf {n_hit - n_int} clades {len(set(internal))} root {internal.count(0)}")
    assert n_int >= 0.25 * n_hit and n_hit - n_int >= 0.25 * n_hit
    assert len(set(internal)) >= 20 and internal.count(0) >= 1
    exp = cm.expected(w.sets(0.7))
    hit = exp[exp != NO]
    n_int = sum(1 for c in hit if int(c) not in cm.is_leaf)
    print(f"theta 0.7: hit {len(hit)} internal {n_int} leaf {len(hit) - n_int}")
    assert n_int >= 0.5 * len(hit) and len(hit) - n_int >= 0.1 * len(hit)


@pytest.mark.parametrize("block", ["0", "1"])
@pytest.mark.parametrize("path", [0, 1])
def test_w_thresholds_paths_sources_entries(w, path, block):
    """θ 1.0, 0.7, 0.3, 0.0, 1.5 x forced path x PFQ_BLOCK x with / without PFQ_WANT_HITS x host / device-resident entry."""
    gt, cm = w.gt, w.cm
    knobs(gt, path, block)
    dev = Device(w.seq, w.off)
    try:
        for thr in (1.0, 0.7, 0.3, 0.0, 1.5):
            sets = w.sets(thr)
            if thr <= 0.0:
                assert all(len(s) == len(w.genomes) for s in sets)      # every read hits every leaf: the top clade
            if thr > 1.0:
                assert sum(1 for s in sets if s) == 3                   # only the three reads without k-mers pass (need 0)
            for hits in (False, True):
                for d in (None, dev):
                    check(gt, cm, w.seq, w.off, thr, sets, hits=hits, dev=d, tag=(path, block, thr, hits, d is not None))
    finally:
        dev.close()
        knobs(gt, -1, None)


@pytest.mark.parametrize("path", [0, 1])
def test_w_best(w, path):
    """PFQ_LCA_BEST at θ 0.7 and 0.3, unpaired and paired: the LCA over the hits with the unit's highest score."""
    gt, cm, ot = w.gt, w.cm, w.ot
    all7, best7 = cm.expected(w.sets(0.7)), cm.expected(w.best(0.7))
    n_hit = int((all7 != NO).sum())
    differ = int((all7 != best7).sum())
    ties = sum(1 for s in w.best(0.7) if len(s) > 1)
    print(f"theta 0.7: hit {n_hit} best differs from all {differ} best keeps a tie {ties}")
    assert differ >= 0.2 * n_hit and ties >= 0.25 * n_hit
    knobs(gt, path, None)
    dev = Device(w.seq, w.off)
    try:
        for thr in (0.7, 0.3):
            for d in (None, dev):
                check(gt, cm, w.seq, w.off, thr, w.best(thr), hits=True, scores=True, lca="best", dev=d, tag=(path, thr, d is not None))
    finally:
        dev.close()
    preads = w.pair_reads()
    seq, off = pack_reads(preads)
    for thr in (0.7, 0.3):
        for mode in ("either", "both"):
            frag = combine(w.pair_sets(thr), mode)
            best = best_sets(frag, pair_scores(ot, preads, frag, w.contains))
            check(gt, cm, seq, off, thr, best, hits=True, scores=True, lca="best", paired=True, mode=mode, tag=(path, thr, mode))
    knobs(gt, -1, None)


@pytest.mark.parametrize("path", [0, 1])
def test_w_paired(w, path):
    """Fragments: either / both, with and without PFQ_WANT_HITS, host and device entry; all-leaf fragments (a mate shorter
    than k with `either`, both mates short with `both`, every fragment at θ 0) land on the top clade."""
    gt, cm = w.gt, w.cm
    knobs(gt, path, None)
    preads = w.pair_reads()
    seq, off = pack_reads(preads)
    dev = Device(seq, off)
    n_leaves = len(w.genomes)
    try:
        for thr in (1.0, 0.7, 0.0):
            for mode in ("either", "both"):
                frag = combine(w.pair_sets(thr), mode)
                n_all = sum(1 for s in frag if len(s) == n_leaves)
                assert n_all >= (60 if mode == "either" else 2), (thr, mode, n_all)
                for hits in (False, True):
                    for d in (None, dev):
                        got = check(gt, cm, seq, off, thr, frag, hits=hits, paired=True, mode=mode, dev=d,
                                    tag=(path, thr, mode, hits, d is not None))
                        assert all(int(got[f]) == cm.top == 0 for f, s in enumerate(frag) if len(s) == n_leaves)
        if path == 0:
            rows = gt.query_pairs([p[0] for p in w.pairs()], [p[1] for p in w.pairs()], 1.0, mode="both", lca="all")
            assert [set(r) for r in rows] == combine(w.pair_sets(1.0), "both")
            assert np.array_equal(gt.last_lca(), cm.expected(combine(w.pair_sets(1.0), "both")))
    finally:
        dev.close()
        knobs(gt, -1, None)


# ---------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------
def test_balanced_tree_of_several_leaf_groups(gpu):
    """2600 leaves, 8191-bit filters: two-level frontier, three leaf groups, 5199 clades counted in LDS; twins, shared prefixes
    and (below θ 1) false positives of the small filters give the multi-hit reads."""
    genomes = _genomes(2600, 150, 260, n_long=6)
    for i in range(300):                                              # twins in different leaf groups (an LCA near the root)
        genomes[1300 + 4 * i] = genomes[i]                            # and neighbours that share a prefix (an LCA near the leaves)
        genomes[2 * i + 601] = genomes[2 * i + 600][:100] + genomes[2 * i + 601][100:]
    ot, ids = oracle_tree(genomes, K, 8191, 4)
    gt = gpu_tree(genomes, ids, K, 8191, 4)
    cm = Clades(ot)
    assert gt.clades() == cm.table
    reads = make_reads(genomes, 700, 200, 150, K)
    seq, off = pack_reads(reads)
    for thr in (1.0, 0.5, 0.0):
        sets = oracle_sets(ot, reads, thr)
        if thr == 1.0:
            assert sum(1 for s in sets if len(s) > 1) >= 20
        for path in (0, 1):
            gt.set_path(path)
            for hits in (False, True):
                check(gt, cm, seq, off, thr, sets, hits=hits, tag=(thr, path, hits))
            st = gt.last_stats()
            assert st.leaf_groups == 3 and (st.coarse_cols > 0 or thr <= 0), (thr, path)    # the two-level frontier ran
    gt.close()


def test_more_clades_than_the_lds_histogram_holds(gpu):
    """5000 leaves: 9999 clades, counted with global atomics."""
    genomes = _genomes(5000, 150, 200)
    genomes[4000] = genomes[5]
    ot, ids = oracle_tree(genomes, K, 8191, 4)
    gt = gpu_tree(genomes, ids, K, 8191, 4)
    cm = Clades(ot)
    assert len(cm.table) == 9999 and gt.clades() == cm.table
    reads = make_reads(genomes, 500, 100, 150, K)
    seq, off = pack_reads(reads)
    for thr in (1.0, 0.0):
        sets = oracle_sets(ot, reads, thr)
        for hits in (False, True):
            check(gt, cm, seq, off, thr, sets, hits=hits, tag=(thr, hits))
    gt.close()


def test_caterpillar_from_disk_then_pruned(gpu, tmp_path):
    """An unbalanced tree with a 300-leaf caterpillar (depth > 300: one unit still costs two loads), loaded from disk, then
    pruned at two depths: the clade table and the counters are derived again after each prune."""
    genomes = _genomes(2500, 150, 230, n_long=4)
    ot, ids = _random_shape_tree(genomes, K, 32749, 5)
    d = str(tmp_path / "db")
    fmt.write_db(ot, d)
    gt = BloomTree.load(d)
    shutil.rmtree(d)
    reads = make_reads(genomes, 600, 150, 150, K) + [genomes[i][:150] for i in range(0, 300, 7)]
    seq, off = pack_reads(reads)
    for depth in (None, 40, 9):
        if depth is not None:
            gt.query_packed(seq, off, 1.0, lca="all")                 # counters that the prune must zero
            assert gt.clade_counts()[0].any()
            ot.prune(depth)
            gt.prune_tree(depth)
            assert not gt.clade_counts()[0].any()
        cm = Clades(ot)
        assert max(cm.dep) == (depth if depth is not None else max(cm.dep)) and (depth is not None or max(cm.dep) >= 300)
        assert gt.clades() == cm.table, depth
        for thr in (1.0, 0.5, 0.0):
            sets = oracle_sets(ot, reads, thr)
            for path in (0, 1):
                gt.set_path(path)
                for hits in (False, True):
                    check(gt, cm, seq, off, thr, sets, hits=hits, tag=(depth, thr, path, hits))
    gt.close()


def test_colliding_internal_names_guard_columns(gpu, tmp_path):
    """Reference-built trees alias internal filters: guard columns, and clade names that collide (the index is the identity)."""
    genomes, ot, ids = _h4_tree(320, 32)
    d = str(tmp_path / "db")
    fmt.write_db(ot, d)
    gt = BloomTree.load(d)
    assert gt.info().superset_verified == 0
    cm = Clades(ot)
    assert gt.clades() == cm.table
    reads = make_reads(genomes, 1200, 200, 150, K)
    seq, off = pack_reads(reads)
    for thr in (1.0, 0.6, 0.0):
        sets = oracle_sets(ot, reads, thr)
        for path in (0, 1):
            gt.set_path(path)
            for hits in (False, True):
                check(gt, cm, seq, off, thr, sets, hits=hits, tag=(thr, path, hits))
    gt.close()


def test_one_leaf_tree(gpu):
    genomes = [rand_dna(3000)]
    ot, ids = oracle_tree(genomes, K, 30011, 5)
    gt = gpu_tree(genomes, ids, K, 30011, 5)
    cm = Clades(ot)
    assert gt.clades() == cm.table == [(-1, 0, 0, 1, ids[0])]
    reads = make_reads(genomes, 60, 30, 150, K)
    seq, off = pack_reads(reads)
    for thr in (1.0, 0.5, 0.0):
        sets = oracle_sets(ot, reads, thr)
        for hits in (False, True):
            got = check(gt, cm, seq, off, thr, sets, hits=hits, tag=(thr, hits))
            assert set(got.tolist()) <= {0, NO}
    pairs = [(reads[i], reads[i + 1]) for i in range(0, len(reads) - 1, 2)]
    preads = [m for p in pairs for m in p]
    seq, off = pack_reads(preads)
    for mode in ("either", "both"):
        frag = combine(mate_sets(ot, preads, 1.0), mode)
        for hits in (False, True):
            check(gt, cm, seq, off, 1.0, frag, hits=hits, paired=True, mode=mode, tag=(mode, hits))
    gt.close()


@pytest.mark.parametrize("deep", [False, True])
def test_one_child_nodes(gpu, tmp_path, deep):
    """A database with a node of one child, opened from disk (the loader accepts it).  deep: root = (P, X), P = (Q, Y),
    Q = (A, -): a single hit on A gives A's clade, the deepest of the chain Q - A.  Not deep: root = (A, -): the top clade,
    what a read that hits every leaf gets, is A's clade 1, not the root."""
    db = tmp_path / "db"
    genome = _one_child_db(db, deep)
    ot = fmt.read_db(str(db))
    gt = BloomTree.load(str(db))
    cm = Clades(ot)
    assert gt.clades() == cm.table
    assert cm.top == (0 if deep else 1)
    rng = np.random.default_rng(11)
    reads = [genome[o:o + 150] for o in range(0, 1300, 50)] + [_dna(rng, 150) for _ in range(40)] + [b"", b"ACG", genome[:14]]
    seq, off = pack_reads(reads)
    for thr in (1.0, 0.3, 0.0):
        sets = oracle_sets(ot, reads, thr)
        for path in (0, 1):
            gt.set_path(path)
            for hits in (False, True):
                got = check(gt, cm, seq, off, thr, sets, hits=hits, tag=(deep, thr, path, hits))
                assert int(got[len(reads) - 3]) == cm.top               # the empty read: every leaf
                if thr == 1.0:
                    assert int(got[0]) == cm.idx[ot.leaves_dfs()[0]]    # a read of A alone: the leaf, not its one-child parent
    preads = reads[:40]
    seq, off = pack_reads(preads)
    for mode in ("either", "both"):
        frag = combine(mate_sets(ot, preads, 1.0), mode)
        for hits in (False, True):
            check(gt, cm, seq, off, 1.0, frag, hits=hits, paired=True, mode=mode, tag=(deep, mode, hits))
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# state
# ---------------------------------------------------------------------------------------------------------------
def small_families():
    rng = np.random.default_rng(99)
    genomes = nested_families(rng, 3, 2, 3, 2000, 0.03, 0.005, 4)
    ids = [f"S{i:02d}" for i in range(len(genomes))]
    return rng, genomes, ids


def test_counters_accumulate_and_are_zeroed(gpu, tmp_path):
    rng, genomes, ids = small_families()
    n0 = len(genomes) - 3
    ot = orc.build_greedy_tree(genomes[:n0], ids[:n0], K, 0.001, 2000, *SEEDS)
    gt = BloomTree.new(K, 0.001, 2000, *SEEDS)
    for g, i in zip(genomes[:n0], ids[:n0]):
        gt.insert(g, i)
    cm = Clades(ot)
    assert gt.clades() == cm.table
    blocks = [w_reads(rng, genomes, 300, 120) for _ in range(3)]
    total_here = np.zeros(len(cm.table), dtype=np.uint64)
    gt.reset_counts()
    for i, (reads, thr, hits) in enumerate(zip(blocks, (1.0, 0.6, 1.0), (False, True, False))):
        seq, off = pack_reads(reads)
        gt.query_packed(seq, off, thr, want_hits=hits, lca="all")
        exp = cm.expected(oracle_sets(ot, reads, thr))
        assert np.array_equal(gt.last_lca(), exp), i
        total_here += cm.here_below(exp)[0]
        here, below = gt.clade_counts()
        assert np.array_equal(here, total_here), i                     # accumulated over the calls
        assert int(below[0]) == int(total_here.sum())
    # a call without the flag leaves the counters alone
    seq, off = pack_reads(blocks[0])
    gt.query_packed(seq, off, 1.0)
    assert np.array_equal(gt.clade_counts()[0], total_here)
    # the counters are not stored
    d = str(tmp_path / "db")
    gt.save(d)
    t2 = BloomTree.load(d)
    assert t2.clades() == cm.table and not t2.clade_counts()[0].any()
    assert [n for _, n in t2.get_leaf_counts()] == [n for _, n in gt.get_leaf_counts()]
    t2.close()
    gt.reset_counts()
    assert not gt.clade_counts()[0].any() and not gt.clade_counts()[1].any()
    # insert: the clade numbering changes, the counters start again, the table is the oracle's new pre-order
    gt.query_packed(seq, off, 1.0, lca="all")
    assert gt.clade_counts()[0].any()
    for g, i in zip(genomes[n0:], ids[n0:]):
        gt.insert(g, i)
        orc.greedy_insert(ot, g, i)
    orc.renumber_preorder(ot)
    cm = Clades(ot)
    assert not gt.clade_counts()[0].any()
    assert gt.clades() == cm.table and len(cm.table) == 2 * len(genomes) - 1
    for thr in (1.0, 0.6):
        sets = oracle_sets(ot, blocks[1], thr)
        s1, o1 = pack_reads(blocks[1])
        for hits in (False, True):
            check(gt, cm, s1, o1, thr, sets, hits=hits, tag=("after insert", thr, hits))
    # prune
    gt.query_packed(seq, off, 1.0, lca="all")
    assert gt.clade_counts()[0].any()
    gt.prune_tree(3)
    ot.prune(3)
    cm = Clades(ot)
    assert not gt.clade_counts()[0].any() and gt.clades() == cm.table
    sets = oracle_sets(ot, blocks[2], 1.0)
    s2, o2 = pack_reads(blocks[2])
    check(gt, cm, s2, o2, 1.0, sets, hits=False, tag="after prune")
    gt.close()


@pytest.mark.parametrize("path,block", [(0, None), (1, "0"), (1, "1")])
def test_hit_buffer_retry_counts_once(w, path, block):
    """PFQ_HIT_SLOTS 0 and 100: the block's hit buffer overflows and the block runs again; `here` equals a run without."""
    gt, cm = w.gt, w.cm
    knobs(gt, path, block)
    preads = w.pair_reads()
    pseq, poff = pack_reads(preads)
    try:
        for thr in (1.0, 0.3):
            sets = w.sets(thr)
            want_here = cm.here_below(cm.expected(sets))[0]
            frag = combine(w.pair_sets(thr), "either")
            for slots in ("0", "100"):
                gt.set_option("PFQ_HIT_SLOTS", slots)
                try:
                    for hits in (False, True):
                        check(gt, cm, w.seq, w.off, thr, sets, hits=hits, tag=(path, block, thr, slots, hits))
                        c = gt.last_capacity()
                        assert c["attempts"] == 2 and c["hit_cap"] == int(slots) < c["hit_cursor"], (path, block, thr, slots, c)
                        assert np.array_equal(gt.clade_counts()[0], want_here)
                    check(gt, cm, pseq, poff, thr, frag, hits=False, paired=True, tag=(path, block, thr, slots, "paired"))
                    assert gt.last_capacity()["attempts"] == 2
                finally:
                    gt.set_option("PFQ_HIT_SLOTS", None)
    finally:
        knobs(gt, -1, None)


def test_documented_error_codes(w, tmp_path):
    gt = w.gt
    seq, off = pack_reads(w.reads[:50])
    gt.query_packed(seq, off, 1.0, lca="all")
    assert len(gt.last_lca()) == 50
    gt.query_packed(seq, off, 1.0, want_hits=True)                    # a call without the flag ends the validity
    with pytest.raises(PfqError) as e:
        gt.last_lca()
    assert e.value.code == PFQ_ERR_ARG and "PFQ_WANT_LCA" in str(e.value)
    L, hits = _ffi.lib(), _ffi.Hits()
    import ctypes as C
    for flags in (_ffi.LCA_BEST, _ffi.LCA_BEST | _ffi.WANT_LCA, _ffi.LCA_BEST | _ffi.WANT_LCA | _ffi.WANT_HITS,
                  _ffi.LCA_BEST | _ffi.WANT_HITS | _ffi.WANT_SCORES):
        rc = L.pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, 50, 1.0, flags, C.byref(hits))
        assert rc == PFQ_ERR_ARG and b"PFQ_LCA_BEST" in L.pfq_last_error(), flags
        with pytest.raises(PfqError):
            gt.last_lca()
    # a subtree shard does not hold the other shards' topology
    d = str(tmp_path / "db")
    gt.save(d)
    shard = BloomTree.load_subtree(d, 2, 1)
    try:
        with pytest.raises(PfqError) as e:
            shard.query_packed(seq, off, 1.0, lca="all")
        assert e.value.code == PFQ_ERR_UNSUPPORTED and "shard" in str(e.value) and "topology" in str(e.value)
        with pytest.raises(PfqError) as e:
            shard.clades()
        assert e.value.code == PFQ_ERR_UNSUPPORTED
        assert shard.query_packed(seq, off, 1.0) is None               # the shard still answers without the flag
    finally:
        shard.close()
