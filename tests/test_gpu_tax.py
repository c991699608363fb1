"""PFQ_WANT_TAXA: every unit (a read; with PFQ_PAIRED a fragment) is counted on the nodes of a taxonomy the user lays over the
leaves: `here` at the deepest node above all its hits, `any` on every node above at least one of them, `below` = the subtree
sums of `here`.

Nothing expected here comes from the library.  The hit sets are the oracle's (orc.query_batch; fragments combined from the
mates' sets as tests/test_gpu_paired.py does), the node table and the counts come from tests/tax_ref.py, the model in plain
Python.  Every case asserts last_taxa() == expected per unit, here / below / any == the reference's, any of the genome nodes
== the call's leaf counts, and that leaf counts, hit CSR, scores and statistics equal those of the same call without the
flag.  Workload W and its helpers are those of tests/test_gpu_lca.py."""
import ctypes as C

import numpy as np
import pytest

import tax_ref
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_build import SEEDS, _dna, _mutate
from test_gpu_lca import K, NO, Device, W, knobs, oracle_sets, small_families, w_reads
from test_gpu_paired import combine
from test_gpu_parity import gpu_tree, make_reads, oracle_tree, rand_dna

pytestmark = pytest.mark.gpu

PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -4, -6


@pytest.fixture(scope="module")
def w(gpu):
    x = W()
    yield x
    x.gt.close()


# ---------------------------------------------------------------------------------------------------------------
# taxonomies
# ---------------------------------------------------------------------------------------------------------------
def random_taxonomy(seed, n_leaves, depth=6):
    """Mixed arity, genomes at the root and at inner taxa, one-child chains, no relation between a leaf's index and where it
    sits: (taxon_parent, taxon_names, leaf_taxon)."""
    rng = np.random.default_rng(seed)
    parent, dep = [-1], [0]
    for _ in range(3 + int(rng.integers(0, 3))):                  # some chains of one-child taxa first, from anywhere
        p = int(rng.integers(0, len(parent)))
        while dep[p] < depth and rng.random() < 0.8:
            parent.append(p)
            dep.append(dep[p] + 1)
            p = len(parent) - 1
    while len(parent) < 40:
        p = int(rng.integers(0, len(parent)))
        if dep[p] < depth:
            parent.append(p)
            dep.append(dep[p] + 1)
    heavy = int(rng.integers(1, len(parent)))                     # top-heavy, as phage taxonomies are
    leaf_taxon = [heavy if rng.random() < 0.4 else 0 if rng.random() < 0.1 else int(rng.integers(0, len(parent))) for _ in range(n_leaves)]
    return parent, [f"t{i}" for i in range(len(parent))], leaf_taxon


def self_taxonomy(cm):
    """The SBT's own topology as a taxonomy: its internal clades are the taxa (pre-order, so a parent comes first)."""
    internal = [c for c in range(len(cm.table)) if c not in cm.is_leaf]
    taxon_of = {c: i for i, c in enumerate(internal)}
    parent = [-1 if cm.par[c] < 0 else taxon_of[cm.par[c]] for c in internal]
    return parent, [cm.table[c][4] for c in internal], [taxon_of[cm.par[c]] for c in cm.leaf_clade]


def stats_of(gt):
    s = gt.last_stats()
    return tuple(int(getattr(s, f)) for f in ("n_reads", "n_hits", "n_allhit_reads", "algorithmic_bytes"))


def call(gt, seq, off, thr, *, taxa, dev=None, scores=False, paired=False, mode="either", **kw):
    if dev is None:
        return gt.query_packed(seq, off, thr, want_hits=True, want_scores=scores, paired=paired, pair_mode=mode, taxa=taxa, **kw)
    res = gt.query_device_hits(dev.seq.ptr, dev.off.ptr, dev.n, dev.total, thr, stream=dev.stream, want_scores=scores, paired=paired,
                               pair_mode=mode, taxa=taxa, **kw)
    return tuple(np.array(a) for a in res)


def plain_call(gt, seq, off, thr, **kw):
    """The call without the flag, counters from zero: (CSR and scores, leaf counts, statistics)."""
    gt.reset_counts()
    res = call(gt, seq, off, thr, taxa=False, **kw)
    return res, gt.get_leaf_counts(), stats_of(gt)


def check(gt, ref, want, seq, off, thr, plain, tag, **kw):
    """The flagged call, counters from zero, against the reference's (last, here, below, any) and against the plain call."""
    gt.reset_counts()
    res = call(gt, seq, off, thr, taxa=True, **kw)
    last = gt.last_taxa()
    stats = stats_of(gt)
    counts = gt.get_leaf_counts()
    here, below, any_ = gt.taxon_counts()
    p_res, p_counts, p_stats = plain
    assert counts == p_counts and stats == p_stats, tag
    assert len(res) == len(p_res) and all(np.array_equal(a, b) for a, b in zip(res, p_res)), tag
    w_last, w_here, w_below, w_any = want
    assert last.dtype == np.uint32 and last.shape == w_last.shape, (tag, last.shape, w_last.shape)
    bad = np.flatnonzero(last != w_last)
    assert bad.size == 0, (tag, bad[:10], last[bad[:10]], w_last[bad[:10]])
    for name, got, exp in (("here", here, w_here), ("below", below, w_below), ("any", any_, w_any)):
        bad = np.flatnonzero(got != exp)
        assert got.shape == exp.shape and bad.size == 0, (tag, name, bad[:10], got[bad[:10]], exp[bad[:10]])
    assert [int(any_[ref.leaf_node[l]]) for l in range(len(counts))] == [n for _, n in counts], tag
    assert int(any_[0]) == int(below[0]) == int((w_last != NO).sum()) and bool((any_ >= below).all()), tag
    return last


def set_tax(gt, ids, tax):
    """Lays `tax` over the tree; the reference's node table must be the library's."""
    gt.set_taxonomy(*tax)
    ref = tax_ref.Nodes(ids, *tax)
    assert gt.taxa() == ref.table
    return ref


REF_CACHE = {}


def ref_counts(key, ref, sets):
    if key not in REF_CACHE:
        REF_CACHE[key] = ref.counts(sets)
    return REF_CACHE[key]


# ---------------------------------------------------------------------------------------------------------------
# 1. the tree's own topology as the taxonomy: the new path against the merged --lca
# ---------------------------------------------------------------------------------------------------------------
def test_self_taxonomy_equals_the_clades(w):
    gt, cm = w.gt, w.cm
    ids = [t for t, _ in gt.get_leaf_counts()]
    ref = set_tax(gt, ids, self_taxonomy(cm))
    leafset = {}
    for c, (_, _, first, count, _) in enumerate(cm.table):
        leafset[frozenset(range(first, first + count))] = c
    by_rank = sorted(range(len(ids)), key=lambda l: ref.rank[l])
    clade_of = [leafset[frozenset(by_rank[r[2]:r[2] + r[3]])] for r in ref.table]
    assert sorted(clade_of) == list(range(len(cm.table)))             # node <-> clade, one to one
    for thr in (1.0, 0.7):
        sets = w.sets(thr)
        exp = cm.expected(sets)
        c_here, c_below = cm.here_below(exp)
        gt.reset_counts()
        gt.query_packed(w.seq, w.off, thr, want_hits=True, taxa=True)
        last = gt.last_taxa()
        assert np.array_equal(np.array([NO if v == NO else clade_of[v] for v in last.tolist()], dtype=np.uint32), exp), thr
        here, below, any_ = gt.taxon_counts()
        assert [int(x) for x in here] == [int(c_here[c]) for c in clade_of], thr
        assert [int(x) for x in below] == [int(c_below[c]) for c in clade_of], thr
        assert np.array_equal(any_, ref.counts(sets)[3]), thr


# ---------------------------------------------------------------------------------------------------------------
# 2. random taxonomies x thresholds x paths x entries
# ---------------------------------------------------------------------------------------------------------------
TAX_SEEDS = (101, 202, 303)


def test_random_taxonomies_are_what_they_should_be(w):
    """Asserted on the reference alone."""
    ids = w.ids
    for seed in TAX_SEEDS:
        tax = random_taxonomy(seed, len(ids))
        ref = tax_ref.Nodes(ids, *tax)
        taxa = [r for r in ref.table if r[4] < 0]
        assert sum(1 for l in range(len(ids)) if ref.rank[l] != l) >= len(ids) // 2
        assert 4 <= max(r[1] for r in taxa) <= 6
        assert any(r[0] == 0 for r in ref.table if r[4] >= 0)                               # genomes at the root
        inner = {r[0] for r in taxa if r[0] > 0}                                              # taxa below the root with a child taxon
        assert any(r[4] >= 0 and r[0] in inner for r in ref.table)                           # ... that hold genomes too
        kids = {}
        for v, r in enumerate(ref.table):
            kids.setdefault(r[0], []).append(v)
        assert any(len(k) == 1 and ref.table[k[0]][4] < 0 for p, k in kids.items() if p >= 0)  # a one-child chain
        assert len({len(k) for k in kids.values()}) >= 3                                    # mixed arity


@pytest.mark.parametrize("block", ["0", "1"])
@pytest.mark.parametrize("path", [0, 1])
def test_random_taxonomies_thresholds_paths_entries(w, path, block):
    """θ 1.0, 0.7, 0.3, 0.0, 1.5 x forced path x PFQ_BLOCK x host / device-resident entry, three taxonomies."""
    gt = w.gt
    ids = [t for t, _ in gt.get_leaf_counts()]
    knobs(gt, path, block)
    dev = Device(w.seq, w.off)
    try:
        plain = {}
        for seed in TAX_SEEDS:
            ref = set_tax(gt, ids, random_taxonomy(seed, len(ids)))
            for thr in (1.0, 0.7, 0.3, 0.0, 1.5):
                sets = w.sets(thr)
                if thr <= 0.0:
                    assert all(len(s) == len(ids) for s in sets)        # every row lists all 80 leaves: the all-leaf shortcut
                if thr > 1.0:
                    assert sum(1 for s in sets if s) == 3               # only the three reads without k-mers
                want = ref_counts((seed, thr), ref, sets)
                for d in (None, dev):
                    if (thr, d is None) not in plain:
                        plain[(thr, d is None)] = plain_call(gt, w.seq, w.off, thr, dev=d)
                    check(gt, ref, want, w.seq, w.off, thr, plain[(thr, d is None)], (seed, path, block, thr, d is not None), dev=d)
    finally:
        dev.close()
        knobs(gt, -1, None)


def test_scores_and_text_entry(w):
    """The flag beside PFQ_WANT_SCORES, and through pfq_text_query."""
    gt = w.gt
    ids = [t for t, _ in gt.get_leaf_counts()]
    ref = set_tax(gt, ids, random_taxonomy(TAX_SEEDS[0], len(ids)))
    want = ref_counts((TAX_SEEDS[0], 0.7), ref, w.sets(0.7))
    check(gt, ref, want, w.seq, w.off, 0.7, plain_call(gt, w.seq, w.off, 0.7, scores=True), "scores", scores=True)
    n = 400
    text = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(w.reads[:n]))
    assert gt.parse_text(text, "fasta")["n_records"] == n
    gt.reset_counts()
    offs, leaves = gt.query_text(0.7, want_hits=True, taxa=True)
    sets = w.sets(0.7)[:n]
    assert [set(leaves[int(offs[i]):int(offs[i + 1])].tolist()) for i in range(n)] == sets
    last, here, below, any_ = ref.counts(sets)
    assert np.array_equal(gt.last_taxa(), last)
    got = gt.taxon_counts()
    assert np.array_equal(got[0], here) and np.array_equal(got[1], below) and np.array_equal(got[2], any_)


# ---------------------------------------------------------------------------------------------------------------
# 3. fragments
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 1])
def test_paired(w, path):
    """either / both on W.pairs(): all-leaf fragments, fragments with one short mate, cross-genome fragments."""
    gt = w.gt
    ids = [t for t, _ in gt.get_leaf_counts()]
    ref = set_tax(gt, ids, random_taxonomy(TAX_SEEDS[1], len(ids)))
    knobs(gt, path, None)
    preads = w.pair_reads()
    seq, off = pack_reads(preads)
    dev = Device(seq, off)
    try:
        for thr in (1.0, 0.7):
            for mode in ("either", "both"):
                frag = combine(w.pair_sets(thr), mode)
                assert sum(1 for s in frag if len(s) == len(ids)) >= (60 if mode == "either" else 2)
                want = ref.counts(frag)
                for d in (None, dev):
                    kw = dict(paired=True, mode=mode, dev=d)
                    last = check(gt, ref, want, seq, off, thr, plain_call(gt, seq, off, thr, **kw), (path, thr, mode, d is not None), **kw)
                    assert all(int(last[f]) == 0 for f, s in enumerate(frag) if len(s) == len(ids))
        if path == 0:
            gt.reset_counts()
            rows = gt.query_pairs([p[0] for p in w.pairs()], [p[1] for p in w.pairs()], 1.0, mode="both", taxa=True)
            frag = combine(w.pair_sets(1.0), "both")
            assert [set(r) for r in rows] == frag and np.array_equal(gt.last_taxa(), ref.counts(frag)[0])
    finally:
        dev.close()
        knobs(gt, -1, None)


# ---------------------------------------------------------------------------------------------------------------
# 4. long rows that are not all-leaf
# ---------------------------------------------------------------------------------------------------------------
def long_row_workload():
    """One family of 72 genomes, each binomial(3000, 0.002) substitutions away from a 3000-base ancestor, plus 24 unrelated
    genomes, shuffled; 600 error-free 150-base reads."""
    rng = np.random.default_rng(11)
    base = _dna(rng, 3000)
    genomes = [_mutate(rng, base, rng.binomial(3000, 0.002)) for _ in range(72)] + [_dna(rng, 3000) for _ in range(24)]
    genomes = [genomes[i] for i in rng.permutation(len(genomes))]
    reads = []
    for _ in range(600):
        g = genomes[int(rng.integers(0, len(genomes)))]
        o = int(rng.integers(0, len(g) - 150 + 1))
        reads.append(g[o:o + 150])
    return genomes, [f"F{i:03d}" for i in range(len(genomes))], reads


def test_long_rows(gpu):
    """Rows of 65 .. 95 of the 96 leaves take the wave-per-row kernel and are not all-leaf.  On the oracle's sets, checked on
    the CPU for this workload (default_rng(11)): 369 of 600 rows at θ 0.7, the longest row at θ 1.0 has 61 entries."""
    genomes, ids, reads = long_row_workload()
    ot = orc.build_greedy_tree(genomes, ids, K, 0.001, 3000, *SEEDS)
    gt = BloomTree.new(K, 0.001, 3000, *SEEDS)
    for g, i in zip(genomes, ids):
        gt.insert(g, i)
    try:
        leaf_ids = [t for t, _ in gt.get_leaf_counts()]
        assert leaf_ids == [ot.tax_id[v] for v in ot.leaves_dfs()]
        ref = set_tax(gt, leaf_ids, random_taxonomy(404, len(ids)))
        seq, off = pack_reads(reads)
        sets7, sets1 = oracle_sets(ot, reads, 0.7), oracle_sets(ot, reads, 1.0)
        n_long = sum(1 for s in sets7 if 65 <= len(s) <= 95)
        print(f"theta 0.7: rows of 65 .. 95 leaves: {n_long} of {len(reads)}; theta 1.0: longest row {max(len(s) for s in sets1)}")
        assert n_long >= 100
        assert max(len(s) for s in sets1) <= 64
        for thr, sets in ((0.7, sets7), (1.0, sets1)):
            for path in (0, 1):
                gt.set_path(path)
                check(gt, ref, ref.counts(sets), seq, off, thr, plain_call(gt, seq, off, thr), (thr, path))
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. more nodes than any LDS histogram holds
# ---------------------------------------------------------------------------------------------------------------
def test_more_nodes_than_the_lds_histograms_hold(w):
    """Every genome under its own chain of 400 one-child taxa: 32 081 nodes, the global-atomic build."""
    gt = w.gt
    ids = [t for t, _ in gt.get_leaf_counts()]
    parent, names, leaf_taxon = [-1], ["root"], []
    for l in range(len(ids)):
        for j in range(400):
            parent.append(0 if j == 0 else len(parent) - 1)
            names.append(f"c{l}_{j}")
        leaf_taxon.append(len(parent) - 1)
    ref = set_tax(gt, ids, (parent, names, leaf_taxon))
    assert ref.n == 32081
    for thr in (1.0, 0.0):
        check(gt, ref, ref.counts(w.sets(thr)), w.seq, w.off, thr, plain_call(gt, w.seq, w.off, thr), thr)


# ---------------------------------------------------------------------------------------------------------------
# 6. degenerate shapes
# ---------------------------------------------------------------------------------------------------------------
def test_flat_and_one_chain_above_everything(w):
    gt = w.gt
    ids = [t for t, _ in gt.get_leaf_counts()]
    n = len(ids)
    flat = ([-1], ["root"], [0] * n)
    chain = ([-1, 0, 1, 2], ["root", "a", "b", "c"], [3] * n)
    chain_split = ([-1, 0, 1, 2, 2], ["root", "a", "b", "c", "d"], [3 + (l % 2) for l in range(n)])
    for name, tax, top in (("flat", flat, 0), ("chain", chain, 3), ("chain_split", chain_split, 2)):
        ref = set_tax(gt, ids, tax)
        assert max(v for v, r in enumerate(ref.table) if r[3] == n) == top
        for thr in (1.0, 0.3, 0.0):
            sets = w.sets(thr)
            last = check(gt, ref, ref.counts(sets), w.seq, w.off, thr, plain_call(gt, w.seq, w.off, thr), (name, thr))
            assert all(int(last[u]) == top for u, s in enumerate(sets) if len(s) == n)   # the top node is not always the root


def test_one_leaf_tree(gpu):
    genomes = [rand_dna(3000)]
    ot, ids = oracle_tree(genomes, K, 30011, 5)
    gt = gpu_tree(genomes, ids, K, 30011, 5)
    try:
        reads = make_reads(genomes, 60, 30, 150, K)
        seq, off = pack_reads(reads)
        for tax in (([-1], ["root"], [0]), ([-1, 0, 1, 0], ["root", "a", "b", "empty"], [2])):
            ref = set_tax(gt, ids, tax)
            assert ref.n == len(tax[0]) - (1 if len(tax[0]) > 1 else 0) + 1
            for thr in (1.0, 0.5, 0.0):
                sets = oracle_sets(ot, reads, thr)
                last = check(gt, ref, ref.counts(sets), seq, off, thr, plain_call(gt, seq, off, thr), (len(tax[0]), thr))
                assert set(last.tolist()) <= {ref.n - 1, NO}                 # the genome's own node, the deepest of the chain
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. state
# ---------------------------------------------------------------------------------------------------------------
def test_counters_accumulate_are_zeroed_and_the_taxonomy_is_dropped(gpu):
    rng, genomes, ids = small_families()
    n0 = len(genomes) - 1
    ot = orc.build_greedy_tree(genomes[:n0], ids[:n0], K, 0.001, 2000, *SEEDS)
    gt = BloomTree.new(K, 0.001, 2000, *SEEDS)
    for g, i in zip(genomes[:n0], ids[:n0]):
        gt.insert(g, i)
    try:
        assert gt.taxa() == [] and all(len(x) == 0 for x in gt.taxon_counts())
        leaf_ids = [t for t, _ in gt.get_leaf_counts()]
        tax_a, tax_b = random_taxonomy(1, n0), random_taxonomy(2, n0)
        bytes_before = int(gt.info().device_bytes)
        ref = set_tax(gt, leaf_ids, tax_a)
        assert int(gt.info().device_bytes) >= bytes_before + 2 * 8 * ref.n + 2 * 4 * n0   # the tables count in device_bytes
        reads = w_reads(rng, genomes, 900, 120)
        sets = oracle_sets(ot, reads, 0.6)
        want = ref.counts(sets)
        # three unequal calls equal one call
        gt.reset_counts()
        for a, b in ((0, 100), (100, 101), (101, len(reads))):
            seq, off = pack_reads(reads[a:b])
            gt.query_packed(seq, off, 0.6, want_hits=True, taxa=True)
            assert np.array_equal(gt.last_taxa(), want[0][a:b])
        seq, off = pack_reads(reads)
        for got, exp in zip(gt.taxon_counts(), want[1:]):
            assert np.array_equal(got, exp)
        # a call without the flag leaves the counters alone and ends last_taxa's validity
        gt.query_packed(seq, off, 0.6, want_hits=True)
        assert np.array_equal(gt.taxon_counts()[2], want[3])
        with pytest.raises(PfqError) as e:
            gt.last_taxa()
        assert e.value.code == PFQ_ERR_ARG and "PFQ_WANT_TAXA" in str(e.value)
        gt.reset_counts()
        assert not any(x.any() for x in gt.taxon_counts()) and gt.taxa() == ref.table
        # set_taxonomy twice replaces and zeroes
        gt.query_packed(seq, off, 0.6, want_hits=True, taxa=True)
        assert gt.taxon_counts()[0].any()
        ref_b = set_tax(gt, leaf_ids, tax_b)
        assert not any(x.any() for x in gt.taxon_counts())
        check(gt, ref_b, ref_b.counts(sets), seq, off, 0.6, plain_call(gt, seq, off, 0.6), "second taxonomy")
        # together with lca, abundance and coverage: each of their results equals the run without the flag
        other = {}
        for taxa in (False, True):
            gt.reset_counts()
            res = gt.query_packed(seq, off, 0.6, want_hits=True, want_scores=True, lca="all", abundance=True, coverage=True, taxa=taxa)
            ab, cv = gt.abundance(), gt.coverage()
            other[taxa] = (res, gt.last_lca(), gt.clade_counts(), ab["mass"], ab["unique"], [ab[k] for k in ("n_units", "n_unhit", "n_unique", "n_ambiguous", "n_all_leaves", "n_entries")],
                           cv["registers"], cv["units"], cv["matched"], gt.get_leaf_counts())
        for x, y in zip(other[False], other[True]):
            if isinstance(x, tuple):
                assert all(np.array_equal(a, b) for a, b in zip(x, y))
            elif isinstance(x, np.ndarray):
                assert np.array_equal(x, y)
            else:
                assert x == y
        for got, exp in zip(gt.taxon_counts(), ref_b.counts(sets)[1:]):
            assert np.array_equal(got, exp)
        # prune and insert drop the taxonomy
        for change in ("insert", "prune"):
            set_tax(gt, [t for t, _ in gt.get_leaf_counts()], random_taxonomy(3, len(gt.get_leaf_counts())))
            if change == "insert":
                gt.insert(genomes[n0], ids[n0])
            else:
                gt.prune_tree(2)
            assert gt.taxa() == [] and all(len(x) == 0 for x in gt.taxon_counts())
            with pytest.raises(PfqError) as e:
                gt.query_packed(seq, off, 0.6, want_hits=True, taxa=True)
            assert e.value.code == PFQ_ERR_STATE and "pfq_tree_set_taxonomy" in str(e.value), change
            assert gt.query_packed(seq, off, 0.6, want_hits=True) is not None
    finally:
        gt.close()


@pytest.mark.parametrize("path,block", [(0, None), (1, "0"), (1, "1")])
def test_hit_buffer_retry_counts_once(w, path, block):
    """PFQ_HIT_SLOTS 0 and 100: the block's hit buffer overflows and the block runs again; the counts equal a run without."""
    gt = w.gt
    ids = [t for t, _ in gt.get_leaf_counts()]
    ref = set_tax(gt, ids, random_taxonomy(TAX_SEEDS[2], len(ids)))
    knobs(gt, path, block)
    try:
        for thr in (1.0, 0.3):
            want = ref_counts((TAX_SEEDS[2], thr), ref, w.sets(thr))
            plain = plain_call(gt, w.seq, w.off, thr)
            for slots in ("0", "100"):
                gt.set_option("PFQ_HIT_SLOTS", slots)
                try:
                    gt.reset_counts()
                    gt.query_packed(w.seq, w.off, thr, want_hits=True, taxa=True)
                    c = gt.last_capacity()
                    assert c["attempts"] == 2 and c["hit_cap"] == int(slots) < c["hit_cursor"], (path, block, thr, slots, c)
                    assert np.array_equal(gt.last_taxa(), want[0])
                    for got, exp in zip(gt.taxon_counts(), want[1:]):
                        assert np.array_equal(got, exp), (path, block, thr, slots)
                    assert gt.get_leaf_counts() == plain[1]
                finally:
                    gt.set_option("PFQ_HIT_SLOTS", None)
    finally:
        knobs(gt, -1, None)


# ---------------------------------------------------------------------------------------------------------------
# 8. documented error codes
# ---------------------------------------------------------------------------------------------------------------
def test_documented_error_codes(w, tmp_path):
    gt = w.gt
    ids = [t for t, _ in gt.get_leaf_counts()]
    n = len(ids)
    set_tax(gt, ids, random_taxonomy(TAX_SEEDS[0], n))
    seq, off = pack_reads(w.reads[:50])
    L, hits = _ffi.lib(), _ffi.Hits()
    # the flag without the hits
    rc = L.pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, 50, 1.0, _ffi.WANT_TAXA, C.byref(hits))
    assert rc == PFQ_ERR_ARG and b"PFQ_WANT_TAXA needs PFQ_WANT_HITS" in L.pfq_last_error()
    with pytest.raises(ValueError):
        gt.query_packed(seq, off, 1.0, taxa=True)
    # argument violations leave the taxonomy that was set
    before = gt.taxa()
    for tax in (([-1, 1], ["root", "a"], [0] * n), ([-1, 0, 2], ["root", "a", "b"], [0] * n), ([0], ["root"], [0] * n),
                ([-1, 0], ["root", "a"], [2] + [0] * (n - 1)), ([-1, 0], ["root", "a"], [-1] + [0] * (n - 1))):
        with pytest.raises(PfqError) as e:
            gt.set_taxonomy(*tax)
        assert e.value.code == PFQ_ERR_ARG, tax[0]
    rc = L.pfq_tree_set_taxonomy(gt._h, 0, None, None, None)
    assert rc == PFQ_ERR_ARG
    assert gt.taxa() == before
    # no taxonomy set
    d = str(tmp_path / "db")
    gt.save(d)
    fresh = BloomTree.load(d)
    try:
        assert fresh.taxa() == []
        with pytest.raises(PfqError) as e:
            fresh.query_packed(seq, off, 1.0, want_hits=True, taxa=True)
        assert e.value.code == PFQ_ERR_STATE
        with pytest.raises(PfqError) as e:
            fresh.last_taxa()
        assert e.value.code == PFQ_ERR_ARG
    finally:
        fresh.close()
    # a subtree shard's rows are partial
    shard = BloomTree.load_subtree(d, 2, 1)
    try:
        m = len(shard.get_leaf_counts())
        with pytest.raises(PfqError) as e:
            shard.set_taxonomy([-1], ["root"], [0] * m)
        assert e.value.code == PFQ_ERR_UNSUPPORTED and "shard" in str(e.value)
        with pytest.raises(PfqError) as e:
            shard.query_packed(seq, off, 1.0, want_hits=True, taxa=True)
        assert e.value.code == PFQ_ERR_UNSUPPORTED
        assert shard.query_packed(seq, off, 1.0, want_hits=True) is not None
    finally:
        shard.close()
    # an empty tree
    empty = BloomTree.new(K, 0.001, 3000, *SEEDS)
    try:
        with pytest.raises(PfqError) as e:
            empty.set_taxonomy([-1], ["root"], [])
        assert e.value.code == PFQ_ERR_STATE
    finally:
        empty.close()
