"""The slots-only build of k_tile_test<0>: every column of the tree has position slots, the entry stream is a
rotating pipeline of steps that stays filled across the switch from one unit to the next.

The all-sparse tree: 8 leaves, k = 21, 10 hashes, 2^21 + 12345 bits = 3 tiles, the last one partial.  A read of 60 bp has 40
k-mers = 400 probes, ~199 in each full tile and a handful in the partial one; a step of the stream is 16 384 entries.  The
columns (leaf order) and what their buckets of a full tile hold:

  0  40 exact + 40 substituted reads + 33 400 reads of 60 bp: more than TEST_GROUP x 1024 pairs, a task has a second group
  1  (a genome of 30 k-mers) 40 exact + 40 substituted: 40 .. 80 pairs of 30 k-mers, under one step
  2  no read at all: a block skips the column, also when it looks two units ahead
  3  one read: a single pair, the pipeline has nothing to rotate
  4  (34 k-mers) as 1
  5  200 reads of 60 bp: ~40 k entries, between two and three steps
  6  40 exact + 40 substituted + 700 reads of 60 bp: ~140 k entries, more steps than the pipeline is deep
  7  120 reads of 60 bp: ~24 k entries, between one and two steps

(The 40 + 40 reads go to the columns whose regime they do not disturb.)  The entry counts are computed here from the
oracle's probe indices, and every regime is asserted before anything is compared."""
import collections

import numpy as np
import pytest

import tile_lists_ref as ref
from oracle import pfq_oracle as orc
from phagefilter_amd import pack_reads
from test_gpu_parity import gpu_tree, oracle_tree
from test_gpu_regimes import mutate, with_knobs

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 10, (1 << 21) + 12345
SEEDS = (5, 10)
RNG = np.random.default_rng(20261020)
KMERS = [600, 30, 620, 580, 34, 610, 590, 605]
MIXED_KMERS = [600, 4000, 30, 620, 4100, 580, 34, 610]   # the tree of test_gpu_tile_lists: sparse and dense columns
WITH_SETS = (0, 1, 4, 6)                                  # 40 exact + 40 substituted reads
SHORT = {0: 33400, 3: 1, 5: 200, 6: 700, 7: 120}          # reads of 60 bp
NO_READS = 2
STEP, TEST_GROUP, CHUNK_PAIRS, DEPTH_MAX = 16384, 32, 1024, 3
STREAM_BIT = 0x80
KMER_TILES = {}   # k-mer -> [tile] number of its probes


def dna(n):
    return RNG.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(n)).astype(np.uint8).tobytes()


def make_reads(genomes):
    """(reads, leaf each exact or substituted read was cut from or -1, is-substituted flags)"""
    reads, leaf, subst = [], [], []
    for li in WITH_SETS:
        g = genomes[li]
        for i in range(40):
            L = int(min(len(g), RNG.integers(60, 151)))
            o = int(RNG.integers(0, len(g) - L + 1))
            r = g[o:o + L]
            reads += [orc.revcomp(r) if i % 2 else r, mutate(r, 1)]
            leaf += [li, li]
            subst += [False, True]
    for _ in range(300):
        reads.append(dna(int(RNG.integers(40, 200))))
        leaf.append(-1)
        subst.append(False)
    for li, n in SHORT.items():
        g = genomes[li]
        for o in RNG.integers(0, len(g) - 60 + 1, n):
            reads.append(g[int(o):int(o) + 60])
            leaf.append(li)
            subst.append(False)
    return reads, np.array(leaf), np.array(subst)


def tile_entries(reads, which):
    """[tile] probes of the reads `which` (indices), from the oracle's probe indices (cached per canonical k-mer)."""
    out = np.zeros(3, dtype=np.int64)
    for r, n in collections.Counter(reads[i] for i in which).items():   # (the 60 bp reads repeat: ~540 offsets a genome)
        for km in orc.get_kmers(r, K):
            if km not in KMER_TILES:
                idx = orc.probe_indices(SEEDS[0], SEEDS[1], H, NBITS, orc.get_lex_less(km))
                KMER_TILES[km] = np.bincount(np.array(idx, dtype=np.int64) >> 20, minlength=3)
            out += n * KMER_TILES[km]
    return out


class Shared:
    pass


@pytest.fixture(scope="module")
def shared(gpu):
    s = Shared()
    s.genomes = [dna(n + K - 1) for n in KMERS]
    s.ot, s.ids = oracle_tree(s.genomes, K, NBITS, H, SEEDS)
    s.gt = gpu_tree(s.genomes, s.ids, K, NBITS, H, SEEDS)
    s.reads, s.leaf, s.subst = make_reads(s.genomes)
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


def run_query(s, thr, tile_mode=1):
    """Counts and per-read hit lists (sorted within a read) on the bucketed path; the slots' info, the passes and pair_stage."""
    gt = s.gt
    gt.reset_counts()
    gt.set_path(1)
    offs, leaves = gt.query_packed(s.seq, s.off, thr, want_hits=True)
    st = gt.last_stats()
    assert st.path == 1 and (tile_mode is None or st.tile_mode == tile_mode), (st.path, st.tile_mode)
    offs = np.asarray(offs).astype(np.int64)
    leaves = np.asarray(leaves).astype(np.int64)
    read_of = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    leaves = leaves[np.lexsort((leaves, read_of))]
    return gt.get_leaf_counts(), offs, leaves, dict(gt.tile_lists_info(), passes=int(st.tile_passes_launched), stage=int(st.pair_stage))


def assert_same(got, want, what):
    assert got[0] == want[0], what
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what


def assert_preconditions(s):
    """Every column sparse and with slots; every pipeline regime among the columns' buckets; what the oracle says of the reads."""
    for v in s.ot.leaves_dfs():
        p = ref.tile_popcounts(s.gt.node_filter(v))
        assert len(p) == 3 and (p <= ref.TILE_LIST_CAP).all(), p
    assert s.gt.tile_lists_info()["columns"] == 8
    assert not (s.leaf == NO_READS).any()
    lo, hi = {}, {}          # entries of a column's buckets: of its exact reads (they are pairs), and with its substituted ones
    for li in range(8):
        exact = np.flatnonzero((s.leaf == li) & ~s.subst)
        lo[li] = tile_entries(s.reads, exact)
        hi[li] = lo[li] + tile_entries(s.reads, np.flatnonzero((s.leaf == li) & s.subst))
    print("entries per column and tile, exact reads .. with substituted:", {li: (lo[li].tolist(), hi[li].tolist()) for li in range(8)})
    assert (s.leaf == 3).sum() == 1 and 0 < lo[3][0] < STEP
    for li in (1, 4):
        assert 0 < lo[li][0] and hi[li][0] < STEP, (li, lo[li], hi[li])
    assert STEP < lo[7][0] and hi[7][0] < 2 * STEP, (lo[7], hi[7])
    assert 2 * STEP < lo[5][0] and hi[5][0] < 3 * STEP, (lo[5], hi[5])
    assert lo[6][0] > DEPTH_MAX * STEP and lo[6][1] > DEPTH_MAX * STEP, lo[6]
    assert ((s.leaf == 0) & ~s.subst).sum() > TEST_GROUP * CHUNK_PAIRS
    assert all(0 < lo[li][2] < STEP for li in (3, 5, 7)), "the partial tile: a short unit after a long one"
    want = oracle_result(s, 1.0)
    per_read = np.diff(want[1])
    assert (per_read[(s.leaf >= 0) & ~s.subst] >= 1).all(), "an exact substring of a leaf must hit it"
    assert (per_read[s.subst] == 0).all(), "a read with one substitution must fail at theta = 1"
    assert dict(want[0])[s.ids[NO_READS]] == 0
    return want


def check_three_builds(s, knobs, calls=1):
    """The slots-only build, PFQ_TILE_STREAM=0 and PFQ_TILE_LISTS=0 agree with the oracle (the last of `calls` calls each)."""
    want = assert_preconditions(s)

    def last(fn):
        for _ in range(calls - 1):
            fn()
        return fn()

    def three():
        on = last(lambda: run_query(s, 1.0))
        generic = with_knobs(s.gt, {"PFQ_TILE_STREAM": "0"}, lambda: last(lambda: run_query(s, 1.0)))
        dense = with_knobs(s.gt, {"PFQ_TILE_LISTS": "0"}, lambda: last(lambda: run_query(s, 1.0)))
        return on, generic, dense
    on, generic, dense = with_knobs(s.gt, {"PFQ_BLOCK": "0", **knobs}, three)
    print(on[3], generic[3], dense[3])
    assert_same(on, want, "slots-only build vs oracle")
    assert_same(generic, want, "PFQ_TILE_STREAM=0 vs oracle")
    assert_same(dense, want, "PFQ_TILE_LISTS=0 vs oracle")
    assert on[3]["stage"] & STREAM_BIT and not generic[3]["stage"] & STREAM_BIT and not dense[3]["stage"] & STREAM_BIT
    for r in (on, generic):
        assert r[3]["list_tiles"] > 0 and r[3]["dense_tiles"] == 0, r[3]
    assert dense[3]["list_tiles"] == 0 and dense[3]["dense_tiles"] > 0, dense[3]
    return on[3], generic[3]


def test_three_builds_equal_oracle(shared):
    check_three_builds(shared, {})


def test_one_block_walks_every_task(shared):
    """PFQ_TEST_BLOCKS=1: one block meets every task and every switch, and skips the column without pairs."""
    on, generic = check_three_builds(shared, {"PFQ_TEST_BLOCKS": "1"})
    for info in (on, generic):
        assert info["list_tiles"] == 3 * info["passes"] * 7, info


def test_several_passes(shared):
    """A small entry budget: the second call launches as many passes as the first one needed."""
    on, generic = check_three_builds(shared, {"PFQ_TILE_ENTRIES": "4000000", "PFQ_TEST_BLOCKS": "1"}, calls=2)
    assert on["passes"] > 1 and generic["passes"] > 1, (on, generic)
    assert on["list_tiles"] == 3 * on["passes"] * 7, on


def test_other_builds_untouched(shared):
    """theta = 0.5 and block mode on the all-sparse tree, theta = 1 on a tree with dense columns: not the slots-only build."""
    s = shared
    assert_preconditions(s)
    got = with_knobs(s.gt, {"PFQ_BLOCK": "0"}, lambda: run_query(s, 0.5))
    assert_same(got, oracle_result(s, 0.5), "theta = 0.5 vs oracle")
    assert not got[3]["stage"] & STREAM_BIT and got[3]["list_tiles"] == 0, got[3]
    got = with_knobs(s.gt, {"PFQ_BLOCK": "1"}, lambda: run_query(s, 1.0, tile_mode=None))
    assert_same(got, oracle_result(s, 1.0), "block mode vs oracle")
    assert not got[3]["stage"] & STREAM_BIT, got[3]

    m = Shared()
    m.genomes = [dna(n + K - 1) for n in MIXED_KMERS]
    m.ot, m.ids = oracle_tree(m.genomes, K, NBITS, H, SEEDS)
    m.gt = gpu_tree(m.genomes, m.ids, K, NBITS, H, SEEDS)
    try:
        pops = [ref.tile_popcounts(m.gt.node_filter(v)) for v in m.ot.leaves_dfs()]
        sparse = [bool((p <= ref.TILE_LIST_CAP).all()) for p in pops]
        assert any(sparse) and not all(sparse)
        m.reads = [g[o:o + 100] for g in m.genomes for o in range(0, max(1, len(g) - 100), 9)] + [dna(100) for _ in range(50)]
        m.reads += [mutate(r, 1) for r in m.reads[::5]]
        m.seq, m.off = pack_reads(m.reads)
        m.oracle = {}
        got = with_knobs(m.gt, {"PFQ_BLOCK": "0"}, lambda: run_query(m, 1.0))
        assert_same(got, oracle_result(m, 1.0), "mixed tree vs oracle")
        assert not got[3]["stage"] & STREAM_BIT, got[3]
        assert got[3]["columns"] == sum(sparse) and got[3]["list_tiles"] > 0 and got[3]["dense_tiles"] > 0, got[3]
    finally:
        m.gt.close()


def test_dense_insert_ends_slots_only(gpu):
    """Two calls on an all-sparse tree, then a dense genome is inserted: the next call runs the generic build."""
    genomes = [dna(n + K - 1) for n in (600, 30, 620, 580)]
    ot, ids = oracle_tree(genomes, K, NBITS, H, SEEDS)
    gt = gpu_tree(genomes, ids, K, NBITS, H, SEEDS)
    try:
        new = dna(4000 + K - 1)
        reads = [g[o:o + 100] for g in genomes + [new] for o in range(0, max(1, min(len(g) - 100, 400)), 7)] + [dna(100) for _ in range(50)]
        reads += [mutate(r, 1) for r in reads[::4]]
        seq, off = pack_reads(reads)

        def query():
            gt.reset_counts()
            for v in range(ot.n_nodes):
                ot.mapped_reads[v] = 0
            gt.set_path(1)
            gt.query_packed(seq, off, 1.0)
            st = gt.last_stats()
            assert (st.path, st.tile_mode) == (1, 1)
            orc.query_batch(ot, reads, 1.0)
            assert gt.get_leaf_counts() == ot.leaf_counts()
            return dict(gt.tile_lists_info(), stage=int(st.pair_stage))

        gt.set_option("PFQ_BLOCK", "0")
        for _ in range(2):
            info = query()
            assert info["columns"] == 4 and info["stage"] & STREAM_BIT and info["list_tiles"] > 0 and info["dense_tiles"] == 0, info
        gt.insert(new, "NEW")
        orc.greedy_insert(ot, new, "NEW")
        orc.renumber_preorder(ot)
        info = query()
        assert info["columns"] == 4 and not info["stage"] & STREAM_BIT and info["dense_tiles"] > 0, info
        assert dict(gt.get_leaf_counts())["NEW"] > 0
    finally:
        gt.close()
