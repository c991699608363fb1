"""pfq_tree_similarity on the device against tests/sim_ref.py over the oracle's filters: shared_bits, bits_a and bits_b exactly;
kmers, shared_kmers and jaccard — one formula applied to identical integers on both sides, so only libm's rounding differs — at
relative 1e-9.  Tiles of the kernel are 128 x 128 leaves and its chunks 16 words: the 130-leaf tree has ragged tiles on both
sides, 200 003 bits are 3126 words (195 chunks and 6 words)."""
import numpy as np
import pytest

import sim_ref
from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, pack_reads
from test_sim_cpu import SEEDS, dna, strain_families

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 4, 200003
PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -4, -6
KEYS = sim_ref.INT_KEYS + sim_ref.FLOAT_KEYS


def ids_of(n, prefix="S"):
    return [f"{prefix}{i:03d}" for i in range(n)]


def balanced(genomes, ids, k=K, nbits=NBITS, h=H, seeds=SEEDS):
    return orc.build_balanced_tree(genomes, ids, k, nbits, h, *seeds), BloomTree.build_balanced(genomes, ids, k, nbits, h, *seeds)


def equal(a, b, tag=None):
    """Two similarity() dicts of the library."""
    for k in KEYS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (tag, k)


class Big:
    """130 leaves: 10 families of 3 strains and 100 unrelated genomes of 2 000 bp, balanced.  `ref`: all x all, computed once."""

    def __init__(self):
        self.rng = np.random.default_rng(2718)
        self.genomes = strain_families(self.rng, 10, 3, 2000, 0.006, 100)
        self.ids = ids_of(130)
        self.ot, self.gt = balanced(self.genomes, self.ids)
        self.ref = sim_ref.similarity(self.ot)


@pytest.fixture(scope="module")
def big(gpu):
    x = Big()
    assert x.ref["shared_bits"].shape == (130, 130) and x.ref["jaccard"][0, 1] > 0.5 > x.ref["jaccard"][0, 3]
    yield x
    x.gt.close()


# ---------------------------------------------------------------------------------------------------------------
# 1. ragged tiles, sublists in any order, repeats
# ---------------------------------------------------------------------------------------------------------------
def test_all_against_all(big):
    got = big.gt.similarity()
    sim_ref.same(got, big.ref, "all x all")
    assert np.array_equal(np.diag(got["shared_bits"]).astype(np.uint64), got["bits_a"]) and (np.diag(got["jaccard"]) == 1.0).all()
    fam = got["jaccard"][:30, :30]
    assert all(fam[i, j] > 0.5 for i in range(30) for j in range(30) if i // 3 == j // 3)


@pytest.mark.parametrize("n_a,n_b", [(1, 1), (1, 130), (3, 65), (63, 64), (64, 64), (65, 127), (127, 128), (128, 128), (129, 1), (300, 7)])
def test_rectangular_sublists(big, n_a, n_b):
    rng = np.random.default_rng(n_a * 1000 + n_b)
    la = rng.permutation(130)[:n_a] if n_a <= 130 else rng.integers(0, 130, n_a)
    lb = rng.permutation(130)[:n_b]
    if n_b >= 3:
        lb[-1] = lb[1]                                                       # a repeated leaf
    want = sim_ref.sub(big.ref, la, lb)
    sim_ref.same(big.gt.similarity(leaves_a=la, leaves_b=lb), want, (n_a, n_b))
    sim_ref.same(big.gt.similarity(other=big.gt, leaves_a=la.tolist(), leaves_b=None), sim_ref.sub(big.ref, la, np.arange(130)), (n_a, "all"))


# ---------------------------------------------------------------------------------------------------------------
# 2. one word, a ragged last word, few words
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,length", [(64, 27), (127, 30), (4099, 200)])
def test_word_count(gpu, nbits, length):
    rng = np.random.default_rng(nbits)
    base = dna(rng, length)
    genomes = [base, base[:-3] + dna(rng, 3), dna(rng, length), dna(rng, length), base]
    ot, gt = balanced(genomes, ids_of(5), nbits=nbits)
    try:
        want = sim_ref.similarity(ot)
        assert 0 < want["bits_a"].min() and want["bits_a"].max() < nbits and want["shared_bits"][0, 4] == want["bits_a"][0]
        for naive in (None, "1"):
            gt.set_option("PFQ_SIM_NAIVE", naive)
            sim_ref.same(gt.similarity(), want, (nbits, naive))
            sim_ref.same(gt.similarity(leaves_a=[4, 1], leaves_b=[2, 0, 0]), sim_ref.sub(want, [4, 1], [2, 0, 0]), (nbits, naive, "lists"))
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. knobs never change the result; 4. the output is cleared by every call
# ---------------------------------------------------------------------------------------------------------------
def test_knobs(big):
    gt = big.gt
    la, lb = np.arange(129, -1, -1), np.arange(3, 130)
    want = sim_ref.sub(big.ref, la, lb)
    try:
        for slices in ("1", "2", "7", "1000", "0", None):
            gt.set_option("PFQ_SIM_SLICES", slices)
            sim_ref.same(gt.similarity(), big.ref, ("slices", slices))
            sim_ref.same(gt.similarity(leaves_a=la, leaves_b=lb), want, ("slices", slices, "lists"))
        gt.set_option("PFQ_SIM_SLICES", "7")
        gt.set_option("PFQ_SIM_NAIVE", "1")
        sim_ref.same(gt.similarity(), big.ref, "naive")
        sim_ref.same(gt.similarity(leaves_a=la, leaves_b=lb), want, ("naive", "lists"))
    finally:
        gt.set_option("PFQ_SIM_SLICES", None)
        gt.set_option("PFQ_SIM_NAIVE", None)
    with pytest.raises(PfqError) as e:
        gt.set_option("PFQ_SIM_TILE", "64")
    assert e.value.code == PFQ_ERR_ARG


def test_zeroing(big):
    gt = big.gt
    for slices in (None, "5"):
        gt.set_option("PFQ_SIM_SLICES", slices)
        try:
            sim_ref.same(gt.similarity(), big.ref, "first")
            sim_ref.same(gt.similarity(), big.ref, "the same call again")
            sim_ref.same(gt.similarity(leaves_a=[7, 0], leaves_b=[1, 2, 8]), sim_ref.sub(big.ref, [7, 0], [1, 2, 8]), "a small call after a large one")
            sim_ref.same(gt.similarity(leaves_a=[7, 0], leaves_b=[1, 2, 8]), sim_ref.sub(big.ref, [7, 0], [1, 2, 8]), "and again")
        finally:
            gt.set_option("PFQ_SIM_SLICES", None)


# ---------------------------------------------------------------------------------------------------------------
# 5. leaf index -> filter row
# ---------------------------------------------------------------------------------------------------------------
def test_greedy_tree_and_pruned(gpu):
    rng = np.random.default_rng(99)
    genomes = strain_families(rng, 3, 3, 2000, 0.01, 5)
    genomes = [genomes[i] for i in rng.permutation(len(genomes))]
    ids = ids_of(len(genomes), "Q")
    ot = orc.build_greedy_tree(genomes, ids, K, 0.001, 2000, *SEEDS)
    gt = BloomTree.new(K, 0.001, 2000, *SEEDS)
    try:
        for g, i in zip(genomes, ids):
            gt.insert(g, i)
        names = [t for t, _ in ot.leaf_counts()]
        assert [t for t, _ in gt.get_leaf_counts()] == names and names != ids           # (filter rows are not in leaf order)
        want = sim_ref.similarity(ot)
        sim_ref.same(gt.similarity(), want, "greedy")
        # inserted genome x against leaf column names.index(x): itself
        col = [names.index(i) for i in ids]
        assert all(want["jaccard"][c, c] == 1.0 for c in col)
        ot.prune(2)
        gt.prune_tree(2)
        n = len(ot.leaves_dfs())
        assert 2 <= n <= 4 and len(gt.get_leaf_counts()) == n
        sim_ref.same(gt.similarity(), sim_ref.similarity(ot), "pruned: the leaves are unions")
        sim_ref.same(gt.similarity(leaves_a=[n - 1], leaves_b=[0, n - 1]), sim_ref.similarity(ot, None, [n - 1], [0, n - 1]), "pruned, lists")
    finally:
        gt.close()


def test_two_leaves_share_one_file(gpu, tmp_path):
    rng = np.random.default_rng(5)
    genomes = [dna(rng, 2000) for _ in range(6)]
    ot = orc.build_balanced_tree(genomes, ids_of(6), K, NBITS, H, *SEEDS)
    leaves = ot.leaves_dfs()
    ot.bf_path[leaves[4]] = ot.bf_path[leaves[1]]                             # both leaves alias ONE .bf afterwards
    ot.filter_of[leaves[4]] = ot.filter_of[leaves[1]]
    d = str(tmp_path / "db")
    fmt.write_db(ot, d)
    gt = BloomTree.load(d)
    try:
        assert gt.info().n_filters == gt.info().n_nodes - 1
        got = gt.similarity()
        sim_ref.same(got, sim_ref.similarity(ot), "shared .bf")
        assert got["shared_bits"][1, 4] == got["bits_a"][1] == got["bits_b"][4] and got["jaccard"][4, 1] == 1.0
    finally:
        gt.close()


def test_subtree_shard(big, tmp_path):
    d = str(tmp_path / "db")
    fmt.write_db(big.ot, d)
    for index in (1, 3):
        sh, first = orc.subtree_shard(big.ot, 2, index)
        n = len(sh.leaves_dfs())
        gs = BloomTree.load_subtree(d, 2, index)
        try:
            assert 30 <= n <= 35 and int(gs.info().shard_first_leaf) == first
            rows = np.arange(first, first + n)
            sim_ref.same(gs.similarity(), sim_ref.sub(big.ref, rows, rows), ("shard", index))
            # leaf indices are local to the shard; and a shard against the whole tree
            sim_ref.same(gs.similarity(leaves_a=[n - 1, 0]), sim_ref.sub(big.ref, [first + n - 1, first], rows), ("shard", index, "lists"))
            sim_ref.same(gs.similarity(other=big.gt, leaves_b=[0, 129]), sim_ref.sub(big.ref, rows, [0, 129]), ("shard x tree", index))
        finally:
            gs.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. two trees
# ---------------------------------------------------------------------------------------------------------------
def test_two_trees(big):
    rng = np.random.default_rng(31)
    genomes = [dna(rng, 2000) for _ in range(7)] + [big.genomes[0], big.genomes[129], big.genomes[4][:1000] + dna(rng, 1000)]
    ot2, gt2 = balanced(genomes, ids_of(10, "T"))
    try:
        want = sim_ref.similarity(big.ot, ot2)
        assert want["shared_bits"].shape == (130, 10) and want["jaccard"][0, 7] == 1.0 and want["jaccard"][129, 8] == 1.0 and 0.25 < want["jaccard"][4, 9] < 0.4
        sim_ref.same(big.gt.similarity(gt2), want, "a x b")
        sim_ref.same(gt2.similarity(big.gt), sim_ref.similarity(ot2, big.ot), "b x a")
        la, lb = [129, 4, 4, 0], [9, 8, 7]
        sim_ref.same(big.gt.similarity(gt2, la, lb), sim_ref.similarity(big.ot, ot2, la, lb), "lists")
        equal(gt2.similarity(None), gt2.similarity(gt2), "b = None is b = a")
        equal(gt2.similarity(None, [3, 1], None), gt2.similarity(gt2, [3, 1], None), "b = None is b = a, lists")
    finally:
        gt2.close()


@pytest.mark.parametrize("field,kw", [("seed2", dict(seeds=(SEEDS[0], SEEDS[1] ^ 1))), ("seed1", dict(seeds=(SEEDS[0] + 1, SEEDS[1]))),
                                      ("nbits", dict(nbits=NBITS + 1)), ("kmer_size", dict(k=K - 2)), ("num_hashes", dict(h=H + 1))])
def test_trees_that_cannot_be_compared(big, field, kw):
    _, other = balanced(big.genomes[:2], ids_of(2, "X"), **kw)
    try:
        for a, b in ((big.gt, other), (other, big.gt)):
            with pytest.raises(PfqError) as e:
                a.similarity(b, [0], [0])
            assert e.value.code == PFQ_ERR_ARG and field in str(e.value), str(e.value)
        sim_ref.same(big.gt.similarity(leaves_a=[5], leaves_b=[5, 6]), sim_ref.sub(big.ref, [5], [5, 6]), "the trees still work")
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the diagonal; 8. a query's results stay; 9. errors
# ---------------------------------------------------------------------------------------------------------------
def test_diagonal_is_coverage_filter_bits(big):
    got = big.gt.similarity()
    bits = big.gt.coverage()["filter_bits"]
    assert np.array_equal(np.diag(got["shared_bits"]).astype(np.uint64), bits) and np.array_equal(got["bits_a"], bits)
    assert np.allclose(got["kmers_a"], big.gt.coverage()["genome_kmers"], rtol=1e-12, atol=0)


def test_query_state_is_untouched(big):
    gt, rng = big.gt, np.random.default_rng(8)
    reads = []
    for _ in range(200):
        g = big.genomes[int(rng.integers(0, 130))]
        o = int(rng.integers(0, 1900))
        reads.append(g[o:o + 100])
    seq, off = pack_reads(reads)
    gt.reset_counts()
    c0 = np.array([c for _, c in gt.get_leaf_counts()])
    off1, leaves1, scores1 = gt.query_packed(seq, off, 0.8, want_hits=True, want_scores=True)
    assert len(leaves1) >= 200 and scores1.max() == 80
    c1 = np.array([c for _, c in gt.get_leaf_counts()])
    st1 = gt.last_stats()
    sim_ref.same(gt.similarity(), big.ref, "between two queries")
    assert np.array_equal(gt.last_hit_scores(), scores1), "pfq_last_hit_scores still describes the last query"
    st = gt.last_stats()
    assert (st.n_reads, st.n_hits, st.n_candidates, st.path) == (st1.n_reads, st1.n_hits, st1.n_candidates, st1.path)
    assert np.array_equal(np.array([c for _, c in gt.get_leaf_counts()]), c1)
    off2, leaves2, scores2 = gt.query_packed(seq, off, 0.8, want_hits=True, want_scores=True)
    c2 = np.array([c for _, c in gt.get_leaf_counts()])
    assert np.array_equal(off2, off1) and np.array_equal(leaves2, leaves1) and np.array_equal(scores2, scores1)
    assert np.array_equal(c2 - c1, c1 - c0) and (c1 - c0).sum() == len(leaves1)
    assert np.array_equal(gt.last_hit_scores(), scores1)
    gt.reset_counts()


def test_errors(big):
    gt = big.gt
    for la, lb in (([130], None), (None, [0, 130]), ([0, 1, 2 ** 32 - 1], [0])):
        with pytest.raises(PfqError) as e:
            gt.similarity(leaves_a=la, leaves_b=lb)
        assert e.value.code == PFQ_ERR_ARG and "130 leaves" in str(e.value), str(e.value)
    with pytest.raises(PfqError) as e:                                       # 8193 x 8192 > 2^26 pairs
        gt.similarity(leaves_a=np.zeros(8193, dtype=np.uint32), leaves_b=np.full(8192, 129, dtype=np.uint32))
    assert e.value.code == PFQ_ERR_UNSUPPORTED and "panels" in str(e.value), str(e.value)
    with pytest.raises(PfqError) as e:                                       # and far beyond it: refused before the lists are looked at
        gt.similarity(leaves_a=np.zeros(1 << 20, dtype=np.uint32), leaves_b=np.zeros(1 << 20, dtype=np.uint32))
    assert e.value.code == PFQ_ERR_UNSUPPORTED
    for la, lb, shape in (([], None, (0, 130)), (None, [], (130, 0)), ([], [], (0, 0)), (np.zeros(0, dtype=np.uint32), [4], (0, 1))):
        got = gt.similarity(leaves_a=la, leaves_b=lb)
        assert got["shared_bits"].shape == shape and got["shared_bits"].dtype == np.uint32 and got["jaccard"].shape == shape
        assert got["bits_a"].shape == (shape[0],) and got["kmers_b"].shape == (shape[1],) and got["bits_b"].dtype == np.uint64
    sim_ref.same(gt.similarity(leaves_a=[129], leaves_b=[129, 0]), sim_ref.sub(big.ref, [129], [129, 0]), "after the refusals")
    empty = BloomTree.new(K, 0.001, 2000, *SEEDS)
    try:
        for a, b in ((empty, None), (empty, gt), (gt, empty)):
            with pytest.raises(PfqError) as e:
                a.similarity(b)
            assert e.value.code == PFQ_ERR_STATE, str(e.value)
    finally:
        empty.close()
