"""pfq_tree_recluster on the device against tests/cluster_ref.py over the oracle's filters: the merge log (every integer of it)
and the clade table must be equal, whatever the knobs of the shared-bits stage; the new tree holds the same leaf words under
internal filters that are the OR of their children; a query gives every read the same genomes as on the source tree and exactly
what the oracle's query gives on the reference's new tree; reads that hit one strain family get that family's clade as LCA."""
import ctypes as C
import math

import numpy as np
import pytest

import cluster_ref as cr
from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_parity import check_query
from test_sim_cpu import SEEDS, dna, mutate, strain_families

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 4, 200003
PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -4, -6


def ids_of(n, prefix="S"):
    return [f"{prefix}{i:04d}" for i in range(n)]


def balanced(genomes, ids, k=K, nbits=NBITS, h=H, seeds=SEEDS):
    return orc.build_balanced_tree(genomes, ids, k, nbits, h, *seeds), BloomTree.build_balanced(genomes, ids, k, nbits, h, *seeds)


def check_recluster(gt, ot, tag=None, ref=None):
    """gt.recluster() against the reference over `ot`: log, rounds, clades, node count.  Returns (new tree, reference)."""
    ref = ref or cr.recluster(ot)
    nt, log, rounds, _ = ref
    rt = gt.recluster()
    try:
        cr.same_log(rt.merges(), log, rounds, rt.merge_rounds(), tag)
        assert rt.clades() == cr.clade_table(nt), tag
        i = rt.info()
        n = len(ot.leaves_dfs())
        assert (i.n_nodes, i.n_leaves, i.n_filters, i.superset_verified) == (2 * n - 1, n, 2 * n - 1, 1), tag
        assert [t for t, _ in rt.get_leaf_counts()] == [t for t, _ in nt.leaf_counts()], tag
        assert (i.kmer_size, i.nbits, i.num_hashes, i.seed1, i.seed2) == (ot.kmer_size, ot.nbits, ot.num_hashes, ot.seed1, ot.seed2)
    except BaseException:
        rt.close()
        raise
    return rt, ref


def children(table):
    """clade -> [left, right] from a clade table (pre-order: the left child comes first)."""
    ch = {}
    for c, row in enumerate(table):
        if row[0] >= 0:
            ch.setdefault(row[0], []).append(c)
    return ch


# ---------------------------------------------------------------------------------------------------------------
# small filters, few leaves, empty filters, ties
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,length", [(64, 27), (127, 30), (4099, 200)])
def test_small_filters_and_the_knobs_of_the_shared_bits(gpu, nbits, length):
    rng = np.random.default_rng(nbits)
    base = dna(rng, length)
    genomes = [base, base[:-3] + dna(rng, 3), dna(rng, length), dna(rng, length), base]
    ot, gt = balanced(genomes, ids_of(5), nbits=nbits)
    try:
        ref = cr.recluster(ot)
        assert ref[1][0][:3] == (5, 0, 4) and ref[1][0][5] == 1 << 20       # the duplicates first, at similarity 1
        for naive in (None, "1"):
            for slices in (None, "1", "7", "1000"):
                gt.set_option("PFQ_SIM_NAIVE", naive)
                gt.set_option("PFQ_SIM_SLICES", slices)
                rt, _ = check_recluster(gt, ot, (nbits, naive, slices), ref)
                rt.close()
    finally:
        gt.close()


@pytest.mark.parametrize("case", ["1", "2", "3", "short", "two short", "only short"])
def test_few_leaves_and_empty_filters(gpu, case):
    rng = np.random.default_rng(len(case))
    g = [dna(rng, 300) for _ in range(3)]
    short = [b"ACGTACGTAC", b"GATTACA"]                                       # shorter than k: all-zero filters
    genomes = {"1": g[:1], "2": g[:2], "3": g, "short": [g[0], short[0], g[1]], "two short": [short[0], g[0], short[1], g[1]],
               "only short": short}[case]
    ot, gt = balanced(genomes, ids_of(len(genomes)), nbits=4099)
    try:
        rt, (nt, log, rounds, _) = check_recluster(gt, ot, case)
        try:
            assert len(log) == len(genomes) - 1 and (rounds == 0) == (len(genomes) == 1)
            reads = [g[0][:100], g[1][50:150], dna(rng, 80), b"ACG", b""]
            for thr in (1.0, 0.5):
                check_query(rt, nt, reads, thr)
        finally:
            rt.close()
        assert len(gt.merges()) == 0 and gt.merge_rounds() == 0              # the source tree has no log
    finally:
        gt.close()


def test_ties(gpu):
    rng = np.random.default_rng(77)
    a, b = dna(rng, 400), dna(rng, 400)
    genomes = [a, dna(rng, 400), b, a, b, a, dna(rng, 400), b, a]             # 4 x a, 3 x b, 2 singles
    ot, gt = balanced(genomes, ids_of(9), nbits=30011)
    try:
        rt, (nt, log, rounds, _) = check_recluster(gt, ot, "ties")
        rt.close()
        # among equals the smaller index wins: every copy of a prefers 0, and 0 prefers 3; 5 and 8 find each other a round later
        assert [e[1:4] for e in log[:4]] == [(0, 3, 0), (1, 6, 0), (2, 4, 0), (5, 8, 1)] and all(log[i][5] == log[i][6] << 20 for i in (0, 2, 3))
        sets = cr.leaf_sets(log, 9)
        assert frozenset([0, 3, 5, 8]) in sets and frozenset([2, 4, 7]) in sets
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# 130 leaves, 200 003 bits: balanced, and greedy in shuffled insertion order
# ---------------------------------------------------------------------------------------------------------------
class Big:
    def __init__(self, greedy):
        self.rng = np.random.default_rng(2718)
        self.genomes = strain_families(self.rng, 10, 3, 2000, 0.006, 100)
        self.ids = ids_of(130)
        if greedy:
            order = np.random.default_rng(5).permutation(130)
            g, i = [self.genomes[j] for j in order], [self.ids[j] for j in order]
            self.ot = orc.build_greedy_tree(g, i, K, 0.001, 14000, *SEEDS)
            self.gt = BloomTree.new(K, 0.001, 14000, *SEEDS)
            for x, y in zip(g, i):
                self.gt.insert(x, y)
        else:
            self.ot, self.gt = balanced(self.genomes, self.ids)
        self.rt, self.ref = check_recluster(self.gt, self.ot, ("big", greedy))
        self.nt = self.ref[0]
        self.family = {self.ids[3 * f + s]: f for f in range(10) for s in range(3)}

    def close(self):
        self.rt.close()
        self.gt.close()


@pytest.fixture(scope="module", params=[False, True], ids=["balanced", "greedy"])
def big(gpu, request):
    x = Big(request.param)
    yield x
    x.close()


def test_big_tree_filters(big):
    src_table, table = big.gt.clades(), big.rt.clades()
    assert len(table) == 259 and big.rt.info().superset_verified == 1
    src_words = {row[4]: big.gt.node_filter(c) for c, row in enumerate(src_table) if row[3] == 1}
    assert len(src_words) == 130
    words = [big.rt.node_filter(c) for c in range(len(table))]
    ch = children(table)
    n_internal = 0
    for c, row in enumerate(table):
        if row[3] == 1:
            assert c not in ch and np.array_equal(words[c], src_words[row[4]]), row
        else:
            left, right = ch[c]
            assert np.array_equal(words[c], words[left] | words[right]), row
            n_internal += 1
    assert n_internal == 129
    # every family is a clade of exactly its three strains; the height stays logarithmic
    names = [t for t, _ in big.rt.get_leaf_counts()]
    fams = set()
    for row in table:
        below = names[row[2]:row[2] + row[3]]
        if row[3] == 3 and all(n in big.family for n in below) and len({big.family[n] for n in below}) == 1:
            fams.add(big.family[below[0]])
    assert fams == set(range(10))
    assert max(row[1] for row in table) < 2 * math.ceil(math.log2(130)) + 8


def make_reads(big, n_pos=1400, n_neg=400, n_short=200):
    rng = np.random.default_rng(31)
    reads = []
    for _ in range(n_pos):
        g = big.genomes[int(rng.integers(0, 130))]
        o = int(rng.integers(0, 1900))
        reads.append(mutate(rng, g[o:o + 100], 1))                            # 1 % errors
    reads += [dna(rng, 100) for _ in range(n_neg)]
    reads += [dna(rng, int(rng.integers(0, K))) for _ in range(n_short)]
    return [reads[i] for i in rng.permutation(len(reads))]


def tax_sets(tree, seq, off, thr):
    names = [t for t, _ in tree.get_leaf_counts()]
    offs, leaves = tree.query_packed(seq, off, thr, want_hits=True)
    return [frozenset(names[int(j)] for j in leaves[int(offs[r]):int(offs[r + 1])]) for r in range(len(off) - 1)]


def test_query_invariance(big, tmp_path):
    reads = make_reads(big)
    assert len(reads) == 2000
    seq, off = pack_reads(reads)
    for thr in (1.0, 0.5, 0.0):
        for path in (0, 1):
            for t in (big.gt, big.rt):
                t.reset_counts()
                t.set_path(path)
            want, got = tax_sets(big.gt, seq, off, thr), tax_sets(big.rt, seq, off, thr)
            assert got == want, (thr, path)
            assert sorted(big.rt.get_leaf_counts()) == sorted(big.gt.get_leaf_counts()), (thr, path)
            assert thr == 0.0 or 0 < sum(len(s) for s in want) < 130 * len(reads)
            # leaf order, hit lists and counts against the oracle's query on the reference's new tree
            check_query(big.rt, big.nt, reads, thr, path=path)
            csv = str(tmp_path / "c.csv")
            big.rt.save_leaf_counts(csv)
            assert open(csv).read() == big.nt.classification_csv(), (thr, path)
    for t in (big.gt, big.rt):
        t.set_path(-1)
        t.reset_counts()


def test_lca_of_a_family_is_its_clade(big):
    rng = np.random.default_rng(9)
    reads = []
    for _ in range(300):
        g = big.genomes[int(rng.integers(0, 30))]
        o = int(rng.integers(0, 1900))
        reads.append(g[o:o + 100])
    for v in range(big.nt.n_nodes):
        big.nt.mapped_reads[v] = 0
    hits, _, _ = orc.query_batch(big.nt, reads, 0.5)
    per_read = {}
    for r, v in hits:
        per_read.setdefault(r, set()).add(big.nt.tax_id[v])
    fam_reads = {r: s for r, s in per_read.items() if len(s) == 3 and all(n in big.family for n in s) and len({big.family[n] for n in s}) == 1}
    assert len(fam_reads) >= 20, len(fam_reads)
    seq, off = pack_reads(reads)
    big.rt.reset_counts()
    big.rt.query_packed(seq, off, 0.5, want_hits=True, lca="all")
    lca, table = big.rt.last_lca(), big.rt.clades()
    names = [t for t, _ in big.rt.get_leaf_counts()]
    for r, s in fam_reads.items():
        row = table[int(lca[r])]
        assert row[3] == 3 and set(names[row[2]:row[2] + 3]) == s, (r, row, s)
    big.rt.reset_counts()


def test_source_tree_is_untouched(big):
    gt = big.gt
    reads = make_reads(big, 150, 40, 10)
    seq, off = pack_reads(reads)
    gt.reset_counts()
    off1, leaves1, scores1 = gt.query_packed(seq, off, 0.8, want_hits=True, want_scores=True)
    counts, st1, nodes = gt.get_leaf_counts(), gt.last_stats(), gt.info().n_nodes
    rt = gt.recluster()
    try:
        cr.same_log(rt.merges(), big.ref[1], big.ref[2], rt.merge_rounds(), "again")
        assert [c for _, c in rt.get_leaf_counts()] == [0] * 130             # the new tree's counters start at zero
    finally:
        rt.close()
    st = gt.last_stats()
    assert (st.n_reads, st.n_hits, st.n_candidates, st.path) == (st1.n_reads, st1.n_hits, st1.n_candidates, st1.path)
    assert gt.get_leaf_counts() == counts and gt.info().n_nodes == nodes and np.array_equal(gt.last_hit_scores(), scores1)
    off2, leaves2, _ = gt.query_packed(seq, off, 0.8, want_hits=True, want_scores=True)
    assert np.array_equal(off2, off1) and np.array_equal(leaves2, leaves1)
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# more than 2048 leaves: the new tree is served by the two-level frontier
# ---------------------------------------------------------------------------------------------------------------
def test_2100_leaves(gpu):
    rng = np.random.default_rng(2100)
    k, nbits, h = 21, 8191, 3
    genomes = strain_families(rng, 150, 3, 220, 0.01, 2100 - 450)
    order = rng.permutation(2100)
    genomes = [genomes[i] for i in order]
    ot, gt = balanced(genomes, ids_of(2100), k=k, nbits=nbits, h=h)
    try:
        rt, (nt, log, rounds, _) = check_recluster(gt, ot, "2100")
        try:
            reads = []
            for _ in range(500):
                g = genomes[int(rng.integers(0, 2100))]
                o = int(rng.integers(0, len(g) - 100))
                reads.append(g[o:o + 100])
            reads += [dna(rng, 100) for _ in range(100)] + [b"", dna(rng, k - 1)]
            for thr in (1.0, 0.5):
                st = check_query(rt, nt, reads, thr)
                assert st.leaf_groups > 1, (thr, st.leaf_groups)
        finally:
            rt.close()
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# save and load; padding bits; the log goes when the topology changes
# ---------------------------------------------------------------------------------------------------------------
def test_save_load_and_padding(gpu, tmp_path):
    rng = np.random.default_rng(12)
    genomes = strain_families(rng, 3, 3, 400, 0.01, 4)
    ot = orc.build_balanced_tree(genomes, ids_of(13), K, 4099, H, *SEEDS)     # 65 words: 61 padding bits
    ref = cr.recluster(ot)
    dirty = orc.build_balanced_tree(genomes, ids_of(13), K, 4099, H, *SEEDS)
    for v in range(dirty.n_nodes):
        dirty.bits[v, -1] |= np.uint64(((1 << 61) - 1) << 3) if v % 3 else np.uint64(1 << 63)
    d = str(tmp_path / "dirty")
    fmt.write_db(dirty, d)
    gt = BloomTree.load(d)
    try:
        rt = gt.recluster()
        try:
            cr.same_log(rt.merges(), ref[1], ref[2], rt.merge_rounds(), "padding")
            table = rt.clades()
            assert [row[:4] for row in table] == [row[:4] for row in cr.clade_table(ref[0])]
            # the leaves keep their words, padding included
            src = {row[4]: gt.node_filter(c) for c, row in enumerate(gt.clades()) if row[3] == 1}
            for c, row in enumerate(table):
                if row[3] == 1:
                    assert np.array_equal(rt.node_filter(c), src[row[4]]) and int(rt.node_filter(c)[-1]) >> 3
            out = str(tmp_path / "new")
            rt.save(out)
            back = BloomTree.load(out)
            try:
                assert back.clades() == table and back.info().superset_verified == 1 and len(back.merges()) == 0
            finally:
                back.close()
            rd = fmt.read_db(out)
            assert rd.n_nodes == 25 and [t for t, _ in rd.leaf_counts()] == [t for t, _ in rt.get_leaf_counts()]
            assert all(c == 0 for _, c in rd.leaf_counts())
            # the log describes the shape the tree was given: it goes when the shape changes
            assert len(rt.merges()) == 12
            rt.prune_tree(2)
            assert len(rt.merges()) == 0 and rt.merge_rounds() == 0
        finally:
            rt.close()
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------
def test_errors(gpu, tmp_path):
    L = _ffi.lib()
    h = C.c_void_p()
    rng = np.random.default_rng(3)
    genomes = [dna(rng, 300) for _ in range(6)]
    ot, gt = balanced(genomes, ids_of(6), nbits=4099)
    try:
        assert L.pfq_tree_recluster(None, C.byref(h)) == PFQ_ERR_ARG and L.pfq_tree_recluster(gt._h, None) == PFQ_ERR_ARG
        empty = BloomTree.new(K, 0.001, 2000, *SEEDS)
        try:
            with pytest.raises(PfqError) as e:
                empty.recluster()
            assert e.value.code == PFQ_ERR_STATE, str(e.value)
        finally:
            empty.close()
        d = str(tmp_path / "db")
        fmt.write_db(ot, d)
        sh = BloomTree.load_subtree(d, 1, 0)
        try:
            with pytest.raises(PfqError) as e:
                sh.recluster()
            assert e.value.code == PFQ_ERR_UNSUPPORTED and "shard" in str(e.value), str(e.value)
        finally:
            sh.close()
        leaves = ot.leaves_dfs()
        ot.bf_path[leaves[4]] = ot.bf_path[leaves[1]]                          # two leaves alias one .bf
        ot.filter_of[leaves[4]] = ot.filter_of[leaves[1]]
        d2 = str(tmp_path / "db2")
        fmt.write_db(ot, d2)
        al = BloomTree.load(d2)
        try:
            with pytest.raises(PfqError) as e:
                al.recluster()
            assert e.value.code == PFQ_ERR_UNSUPPORTED and ot.bf_path[leaves[1]] in str(e.value), str(e.value)
        finally:
            al.close()
        rt = gt.recluster()                                                   # the tree still works after the refusals
        rt.close()
    finally:
        gt.close()


def test_size_limit(gpu):
    n = 16385
    tiny = [b"ACGTTGCAAC"] * n
    gt = BloomTree.build_balanced(tiny, [f"T{i}" for i in range(n)], 5, 64, 2, *SEEDS)
    try:
        with pytest.raises(PfqError) as e:
            gt.recluster()
        assert e.value.code == PFQ_ERR_UNSUPPORTED and "16385 leaves" in str(e.value) and "16384" in str(e.value), str(e.value)
    finally:
        gt.close()
