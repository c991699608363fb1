"""Position slots of sparse leaf-filter tiles (pfq_tilelist.hip) and k_tile_test<0> rebuilding tiles from them.

One tree serves every test: 8 leaves, k = 21, 10 hashes, 2^21 + 12345 bits = 3 tiles, the last one partial.  Genomes of
~600 and ~30 k-mers give ~3000 and ~150 set bits per full tile (columns with slots); genomes of ~4000 k-mers give ~20 000
(more than a slot's 8192: dense columns).  Every test counts the tiles' set bits itself from the device's filters and asserts
that both kinds of column are there."""
import numpy as np
import pytest

import tile_lists_ref as ref
from oracle import pfq_oracle as orc
from phagefilter_amd import PfqError, pack_reads
from test_gpu_parity import gpu_tree, oracle_tree
from test_gpu_regimes import mutate, with_knobs

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 10, (1 << 21) + 12345
RNG = np.random.default_rng(20261019)
# leaf order: sparse, dense, tiny, sparse, dense, sparse, tiny, sparse (a block that walks the tasks in order goes
# sparse -> dense -> sparse and sparse -> sparse)
KMERS = [600, 4000, 30, 620, 4100, 580, 34, 610]
ONE_LEAF = 3          # the sparse leaf the 60 bp reads come from


def dna(n):
    return RNG.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(n)).astype(np.uint8).tobytes()


def leaf_popcounts(gt, ot):
    """Per leaf column: (filter words, set bits of every tile), from the device's own filters."""
    out = []
    for v in ot.leaves_dfs():
        w = gt.node_filter(v)
        out.append((w, ref.tile_popcounts(w)))
    return out


def assert_preconditions(pops):
    sparse = [bool((p <= ref.TILE_LIST_CAP).all()) for _, p in pops]
    assert any(sparse), "no leaf with every tile within the cap"
    assert any((p > ref.TILE_LIST_CAP).any() for _, p in pops), "no leaf with a tile above the cap"
    assert all(len(p) == 3 for _, p in pops)
    return sparse


def make_reads(genomes):
    exact, subst = [], []
    for g in genomes:
        for _ in range(40):
            L = int(min(len(g), RNG.integers(60, 151)))
            o = int(RNG.integers(0, len(g) - L + 1))
            r = g[o:o + L]
            exact.append(orc.revcomp(r) if len(exact) % 2 else r)
            subst.append(mutate(r, 1))
    rand = [dna(int(RNG.integers(40, 200))) for _ in range(300)]
    g = genomes[ONE_LEAF]
    one = [g[o:o + 60] for o in RNG.integers(0, len(g) - 60 + 1, 33400)]
    return exact, subst, rand, one


class Shared:
    pass


@pytest.fixture(scope="module")
def shared(gpu):
    s = Shared()
    s.genomes = [dna(n + K - 1) for n in KMERS]
    s.ot, s.ids = oracle_tree(s.genomes, K, NBITS, H)
    s.gt = gpu_tree(s.genomes, s.ids, K, NBITS, H)
    s.exact, s.subst, s.rand, s.one = make_reads(s.genomes)
    s.reads = s.exact + s.subst + s.rand + s.one
    s.seq, s.off = pack_reads(s.reads)
    s.oracle = {}
    yield s
    s.gt.close()


def oracle_result(s, thr):
    """(per-leaf counts, CSR offsets, CSR leaf columns) of the shared reads, computed once per threshold."""
    if thr not in s.oracle:
        for v in range(s.ot.n_nodes):
            s.ot.mapped_reads[v] = 0
        hits, _, _ = orc.query_batch(s.ot, s.reads, thr, threads=4)
        col = {v: i for i, v in enumerate(s.ot.leaves_dfs())}
        h = np.array([(r, col[v]) for r, v in hits], dtype=np.int64).reshape(-1, 2)
        h = h[np.lexsort((h[:, 1], h[:, 0]))]
        offs = np.zeros(len(s.reads) + 1, dtype=np.int64)
        np.add.at(offs, h[:, 0] + 1, 1)
        s.oracle[thr] = (s.ot.leaf_counts(), np.cumsum(offs), h[:, 1].copy())
    return s.oracle[thr]


def run_query(s, thr):
    """Counts and per-read hit lists (sorted within a read) of the shared reads on the bucketed path, and the slots' info."""
    gt = s.gt
    gt.reset_counts()
    gt.set_path(1)
    offs, leaves = gt.query_packed(s.seq, s.off, thr, want_hits=True)
    st = gt.last_stats()
    assert (st.path, st.tile_mode) == (1, 1), (st.path, st.tile_mode)
    offs = np.asarray(offs).astype(np.int64)
    leaves = np.asarray(leaves).astype(np.int64)
    read_of = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    leaves = leaves[np.lexsort((leaves, read_of))]
    return gt.get_leaf_counts(), offs, leaves, dict(gt.tile_lists_info(), passes=int(st.tile_passes_launched))


def assert_same(got, want, what):
    assert got[0] == want[0], what
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what


def check_results(s, knobs):
    """Lists on, PFQ_TILE_LISTS=0 and the oracle agree at theta = 1; the counters say which path the tiles took."""
    want = oracle_result(s, 1.0)
    n_exact, n_subst = len(s.exact), len(s.subst)
    per_read = np.diff(want[1])
    assert (per_read[:n_exact] >= 1).all(), "an exact substring of a leaf must hit it"
    assert (per_read[n_exact:n_exact + n_subst] == 0).all(), "a read with one substitution must fail at theta = 1"
    assert (per_read[-len(s.one):] >= 1).all() and len(s.one) > 32 * 1024

    def both():
        on = run_query(s, 1.0)
        off = with_knobs(s.gt, {"PFQ_TILE_LISTS": "0"}, lambda: run_query(s, 1.0))
        return on, off
    on, off = with_knobs(s.gt, {"PFQ_BLOCK": "0", **knobs}, both)
    assert_same(on, want, "lists on vs oracle")
    assert_same(off, want, "PFQ_TILE_LISTS=0 vs oracle")
    assert on[3]["list_tiles"] > 0 and on[3]["dense_tiles"] > 0, on[3]
    assert off[3]["list_tiles"] == 0 and off[3]["columns"] == 0 and off[3]["dense_tiles"] > 0, off[3]
    return on[3]


def test_builder_slots_equal_numpy(shared):
    s = shared
    pops = leaf_popcounts(s.gt, s.ot)
    sparse = assert_preconditions(pops)
    info = s.gt.tile_lists_info()
    assert info["columns"] == sum(sparse)
    assert info["bytes"] == sum(sparse) * 3 * ref.TILE_LIST_CAP * 4
    empty_tiles = 0
    for col, ((w, p), sp) in enumerate(zip(pops, sparse)):
        if not sp:
            with pytest.raises(PfqError):
                s.gt.tile_list(col, 0)
            continue
        for t in range(3):                                      # (tile 2 is the partial one)
            slot = s.gt.tile_list(col, t)
            ref.check_slot(slot, w, t)
            assert set(slot.tolist()) - {ref.TILE_LIST_NONE} == set(ref.tile_positions(w, t).tolist()), (col, t)
            if p[t] == 0:
                empty_tiles += 1
                assert (slot == ref.TILE_LIST_NONE).all(), (col, t)
    print("set bits per tile:", [p.tolist() for _, p in pops], "empty tiles:", empty_tiles)


def test_results_lists_on_off_oracle(shared):
    assert_preconditions(leaf_popcounts(shared.gt, shared.ot))
    info = check_results(shared, {})
    print(info)


def test_one_block_walks_every_task(shared):
    """PFQ_TEST_BLOCKS=1: one block meets sparse -> dense -> sparse and un-sets a slot's bits before every next slot."""
    s = shared
    sparse = assert_preconditions(leaf_popcounts(s.gt, s.ot))
    info = check_results(s, {"PFQ_TEST_BLOCKS": "1"})
    # the one block takes every (column with pairs, tile) once per pass: all 8 leaves have reads
    n = 3 * info["passes"]
    assert info["list_tiles"] == n * sum(sparse) and info["dense_tiles"] == n * (len(sparse) - sum(sparse)), info


def test_other_modes_untouched(shared):
    s = shared
    assert_preconditions(leaf_popcounts(s.gt, s.ot))
    want = oracle_result(s, 0.5)
    got = with_knobs(s.gt, {"PFQ_BLOCK": "0"}, lambda: run_query(s, 0.5))
    assert_same(got, want, "theta = 0.5 vs oracle")
    assert got[3]["list_tiles"] == 0, got[3]


def test_layout_rebuilt_after_insert(gpu):
    """Query, insert one more genome, query again: the slots are those of the new tree."""
    genomes = [dna(n + K - 1) for n in KMERS[:4]]
    ot, ids = oracle_tree(genomes, K, NBITS, H)
    gt = gpu_tree(genomes, ids, K, NBITS, H)
    try:
        new = dna(590 + K - 1)
        reads = [g[o:o + 100] for g in genomes + [new] for o in range(0, 400, 7) if o + 100 <= len(g)] + [dna(100) for _ in range(50)]
        new_first = sum(1 for g in genomes for o in range(0, 400, 7) if o + 100 <= len(g))
        seq, off = pack_reads(reads)

        def query():
            gt.reset_counts()
            for v in range(ot.n_nodes):
                ot.mapped_reads[v] = 0
            gt.set_path(1)
            gt.query_packed(seq, off, 1.0)
            assert gt.last_stats().tile_mode == 1
            orc.query_batch(ot, reads, 1.0)
            assert gt.get_leaf_counts() == ot.leaf_counts()
            return gt.tile_lists_info()

        gt.set_option("PFQ_BLOCK", "0")
        sparse = assert_preconditions(leaf_popcounts(gt, ot))
        info = query()
        assert info["columns"] == sum(sparse) and info["list_tiles"] > 0 and info["dense_tiles"] > 0, info
        gt.insert(new, "NEW")
        orc.greedy_insert(ot, new, "NEW")
        orc.renumber_preorder(ot)
        pops = leaf_popcounts(gt, ot)
        sparse2 = assert_preconditions(pops)
        assert len(sparse2) == 5 and sum(sparse2) == sum(sparse) + 1
        info = query()
        assert info["columns"] == sum(sparse2) and info["list_tiles"] > 0, info
        counts = dict(gt.get_leaf_counts())
        n_new = len(reads) - 50 - new_first
        assert n_new > 0 and counts["NEW"] >= n_new, (counts, n_new)
        col = [ot.tax_id[v] for v in ot.leaves_dfs()].index("NEW")
        for t in range(3):
            ref.check_slot(gt.tile_list(col, t), pops[col][0], t)
    finally:
        gt.close()
