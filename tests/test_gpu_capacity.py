"""Full scratch buffers of the bucketed path: every "no room -> certify inline" branch against the oracle, and the hit-buffer
retry.  The test knobs PFQ_PAIR_SLOTS, PFQ_GUARD_SLOTS, PFQ_MISS_WORDS, PFQ_KMISS_BYTES and PFQ_HIT_SLOTS shrink one capacity
each; pfq_debug_last_capacity (BloomTree.last_capacity) shows that the intended buffer did overflow, so a
knob that stops working fails here instead of passing quietly.  Every cap runs at 0 (everything inline), at a few
reservations (one launch mixes deferred and inline pairs) and just below what the block needs."""
import numpy as np
import pytest

from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, pack_reads
from test_gpu_paired import check_pairs, make_pairs, mate_sets
from test_gpu_parity import RNG, gpu_tree, hits_of, make_reads, oracle_hits, oracle_tree, rand_dna
from test_gpu_regimes import family_genomes, mutate, with_knobs
from test_gpu_scores import expected_scores, long_reads

pytestmark = pytest.mark.gpu

K = 21
# buffer -> (knob, cursor, cap, unit of a reservation)
BUFFERS = {
    "pair": ("PFQ_PAIR_SLOTS", "pair_cursor", "pair_cap", 32),
    "guard": ("PFQ_GUARD_SLOTS", "guard_cursor", "guard_cap", 32),
    "miss": ("PFQ_MISS_WORDS", "miss_cursor", "miss_cap", 256),
    "kmiss": ("PFQ_KMISS_BYTES", "kmiss_used", "kmiss_cap", 16),
}


def oracle_result(ot, reads, thr):
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    ohits, _, _ = orc.query_batch(ot, reads, thr)
    return oracle_hits(ot, ohits), ot.leaf_counts()


def mode_of(gt):
    """(path, tile_mode): tile_mode 2 is block mode."""
    st = gt.last_stats()
    return st.path, st.tile_mode


def check_overflow(gt, ot, reads, thr, buf, *, block=False, scores=False, knobs=None, want=None):
    """One block with `buf`'s cap at 0, a few reservations and just below the demand of the same block: hits, counts and
    scores == the oracle's, the buffer overflowed, partial caps also took pairs, and the regime is the default cap's."""
    knob, cur, cap_key, unit = BUFFERS[buf]
    base = dict(knobs or {})
    base["PFQ_BLOCK"] = "1" if block else "0"
    gt.set_path(1)
    seq, off = pack_reads(reads)
    want_hits, want_counts = want or oracle_result(ot, reads, thr)

    def run():
        gt.reset_counts()
        res = gt.query_packed(seq, off, thr, want_hits=True, want_scores=scores)
        return res, gt.get_leaf_counts(), mode_of(gt), gt.last_capacity()

    res0, counts0, mode0, cap0 = with_knobs(gt, base, run)
    assert counts0 == want_counts and hits_of(res0[0], res0[1]) == want_hits, (buf, thr)
    assert mode0[0] == 1 and (mode0[1] == 2) == block, (buf, thr, mode0)
    if scores:
        assert np.array_equal(res0[2].astype(np.int64), expected_scores(ot, reads, res0[0], res0[1])), (buf, thr)
    demand = cap0[cur]
    assert demand <= cap0[cap_key], ("the default cap already overflows", buf, cap0)
    assert demand >= 4 * unit, ("the block does not fill a few reservations", buf, cap0)
    # (reservations are taken in whatever order the waves run: "just below" leaves a margin of 5 %)
    for cap in (0, 2 * unit, demand - max(unit, demand // 20 // unit * unit)):
        res, counts, mode, c = with_knobs(gt, {**base, knob: str(cap)}, run)
        assert mode == mode0, (buf, thr, cap, mode, mode0)
        assert counts == want_counts, (buf, thr, cap)
        assert all(np.array_equal(x, y) for x, y in zip(res, res0)), (buf, thr, cap)
        assert c[cap_key] == cap, (buf, cap, c)
        if buf == "kmiss":      # (the bytes handed out saturate at the cap: the default cap's figure is the demand)
            assert c[cur] == cap < demand, (buf, cap, demand, c)
        else:
            assert c[cur] > c[cap_key], ("no overflow", buf, cap, c)
        if cap:
            assert c["pairs_sorted"] > 0, ("a partial cap took no pairs", buf, cap, c)
    return demand


# ---------------------------------------------------------------------------------------------------------------
# trees and reads
# ---------------------------------------------------------------------------------------------------------------
def close_families(n_families, length=3000, subs=2):
    """Families of 8 strains 2 substitutions apart: a read of one passes about 8 leaves."""
    genomes = []
    for _ in range(n_families):
        base = rand_dna(length)
        genomes += [base] + [mutate(base, subs) for _ in range(7)]
    return genomes + [rand_dna(length) for _ in range(4)]


def family_reads(genomes, n=1500):
    reads = make_reads(genomes, n, n // 10, 150, K) + long_reads(genomes, 6)
    RNG.shuffle(reads)
    return reads


@pytest.fixture(scope="module")
def families(gpu):
    genomes = close_families(4) + family_genomes(2)
    ot, ids = oracle_tree(genomes, K, 131071, 7)
    gt = gpu_tree(genomes, ids, K, 131071, 7)
    yield genomes, ot, gt, family_reads(genomes)
    gt.close()


@pytest.fixture(scope="module")
def guarded(gpu, tmp_path_factory):
    """Internal filters that are not unions and two internal nodes sharing one .bf: guard columns."""
    genomes = close_families(2) + [rand_dna(3000) for _ in range(6)]
    ot, ids = oracle_tree(genomes, K, 131071, 7)
    internal = [v for v in range(ot.n_nodes) if not ot.is_leaf(v)]
    ot.bits[ot.filter_of[internal[1]]][::2] = 0
    a, b = internal[2], internal[3]
    ot.bf_path[b] = ot.bf_path[a]
    ot.filter_of[b] = ot.filter_of[a]
    d = str(tmp_path_factory.mktemp("guarded") / "db")
    fmt.write_db(ot, d)
    gt = BloomTree.load(d)
    assert gt.info().superset_verified == 0
    yield genomes, ot, gt, family_reads(genomes)
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# every buffer's overflow branch
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1.0, 0.7, 0.3])
def test_pair_buffer_overflow_pair_pipeline(families, thr):
    genomes, ot, gt, reads = families
    check_overflow(gt, ot, reads, thr, "pair")


@pytest.mark.parametrize("thr", [1.0, 0.3])
def test_pair_buffer_overflow_block_mode(families, thr):
    genomes, ot, gt, reads = families
    check_overflow(gt, ot, reads, thr, "pair", block=True)


@pytest.mark.parametrize("thr", [0.7, 0.3])
def test_miss_words_overflow(families, thr):
    genomes, ot, gt, reads = families
    check_overflow(gt, ot, reads, thr, "miss")


@pytest.mark.parametrize("thr,block", [(0.3, False), (0.7, False), (0.3, True)])
def test_tile_miss_bytes_overflow(families, thr, block):
    genomes, ot, gt, reads = families
    check_overflow(gt, ot, reads, thr, "kmiss", block=block)


@pytest.mark.parametrize("buf,thr", [("pair", 1.0), ("pair", 0.3), ("miss", 0.3), ("kmiss", 0.3)])
def test_overflow_with_scores(families, buf, thr):
    genomes, ot, gt, reads = families
    check_overflow(gt, ot, reads[:600] + reads[-40:], thr, buf, scores=True)


@pytest.mark.parametrize("buf,thr", [("guard", 1.0), ("guard", 0.7), ("guard", 0.3), ("pair", 1.0), ("miss", 0.7)])
def test_guard_columns_overflow(guarded, buf, thr):
    genomes, ot, gt, reads = guarded
    check_overflow(gt, ot, reads, thr, buf)


def test_two_level_tree_overflow(gpu):
    """PFQ_COARSE_MIN_LEAVES=1024 on an 1100-leaf tree: two leaf groups under a coarse level."""
    genomes = [rand_dna(int(RNG.integers(200, 400))) for _ in range(1100)]
    genomes[1050] = genomes[3]
    ot, ids = oracle_tree(genomes, K, 60013, 4)
    gt = gpu_tree(genomes, ids, K, 60013, 4)
    reads = make_reads(genomes, 1500, 150, 150, K)
    try:
        gt.set_option("PFQ_COARSE_MIN_LEAVES", "1024")
        for buf, thr in (("pair", 1.0), ("pair", 0.7), ("miss", 0.7)):
            check_overflow(gt, ot, reads, thr, buf)
            st = gt.last_stats()
            assert st.coarse_cols > 0 and st.leaf_groups == 2, (buf, thr)
    finally:
        gt.close()


@pytest.mark.parametrize("buf,thr,block", [("pair", 1.0, False), ("pair", 0.3, False), ("pair", 1.0, True), ("miss", 0.3, False),
                                           ("kmiss", 0.3, False)])
def test_paired_overflow(families, buf, thr, block):
    """PFQ_PAIRED, both modes, with one buffer at 0, a few reservations and just below the demand."""
    genomes, ot, gt, _ = families
    pairs = make_pairs(genomes, K, 60)
    sets = mate_sets(ot, [m for p in pairs for m in p], thr)
    knob, cur, cap_key, unit = BUFFERS[buf]
    gt.set_path(1)
    base = {"PFQ_BLOCK": "1" if block else "0"}
    for mode in ("either", "both"):
        with_knobs(gt, base, lambda: check_pairs(gt, ot, pairs, thr, mode, oracle=sets))
        mode0, demand = mode_of(gt), gt.last_capacity()[cur]
        assert demand >= 2 * unit, (buf, thr, mode, demand)
        for cap in (0, unit, demand - max(unit, demand // 20 // unit * unit)):
            with_knobs(gt, {**base, knob: str(cap)}, lambda: check_pairs(gt, ot, pairs, thr, mode, oracle=sets))
            c = gt.last_capacity()
            assert mode_of(gt) == mode0 and c[cap_key] == cap, (buf, thr, mode, cap, c)
            assert (c[cur] == cap < demand) if buf == "kmiss" else c[cur] > cap, (buf, thr, mode, cap, c)
            if cap:
                assert c["pairs_sorted"] > 0, (buf, thr, mode, cap, c)


# ---------------------------------------------------------------------------------------------------------------
# the hit-buffer retry: counters restored from the snapshot, the block run again
# ---------------------------------------------------------------------------------------------------------------
HIT_MODES = [(0, None), (1, "0"), (1, "1")]   # (path, PFQ_BLOCK): direct, pair pipeline, block mode


def doubled(counts):
    return [(t, 2 * n) for t, n in counts]


@pytest.mark.parametrize("path,block", HIT_MODES)
@pytest.mark.parametrize("thr", [1.0, 0.3])
def test_hit_retry_on_counted_tree(families, path, block, thr):
    """A counts-only call, then PFQ_HIT_SLOTS (0, then 100) on the same block with hits and scores: the counters hold twice
    the oracle's counts only if the retry restored them before running the block again."""
    genomes, ot, gt, reads = families
    reads = reads[:800]
    seq, off = pack_reads(reads)
    want_hits, want_counts = oracle_result(ot, reads, thr)
    gt.set_path(path)
    knobs = {} if block is None else {"PFQ_BLOCK": block}
    for slots in ("0", "100"):
        def run():
            gt.reset_counts()
            gt.query_packed(seq, off, thr)
            assert gt.get_leaf_counts() == want_counts
            offs, leaves, scores = gt.query_packed(seq, off, thr, want_hits=True, want_scores=True)
            return offs, leaves, scores.copy(), gt.last_capacity(), gt.get_leaf_counts()
        offs, leaves, scores, c, counts = with_knobs(gt, {**knobs, "PFQ_HIT_SLOTS": slots}, run)
        assert c["attempts"] == 2 and c["hit_cap"] == int(slots) < c["hit_cursor"], (path, block, thr, c)
        assert counts == doubled(want_counts), (path, block, thr, slots)
        assert hits_of(offs, leaves) == want_hits, (path, block, thr, slots)
        assert np.array_equal(scores.astype(np.int64), expected_scores(ot, reads, offs, leaves)), (path, block, thr)
        path_now, tile_mode = mode_of(gt)
        assert path_now == path and (tile_mode == 2) == (block == "1"), (path, block, thr, path_now, tile_mode)


@pytest.mark.parametrize("path,block", HIT_MODES)
def test_hit_retry_paired(families, path, block):
    """PFQ_PAIRED (the pair_hits branch) with PFQ_HIT_SLOTS=0 after a counts-only paired call: fragments counted once more."""
    genomes, ot, gt, _ = families
    pairs = make_pairs(genomes, K, 40)
    reads = [m for p in pairs for m in p]
    seq, off = pack_reads(reads)
    gt.set_path(path)
    knobs = {} if block is None else {"PFQ_BLOCK": block}
    for thr in (1.0, 0.3):
        sets = mate_sets(ot, reads, thr)
        for mode in ("either", "both"):
            with_knobs(gt, knobs, lambda: check_pairs(gt, ot, pairs, thr, mode, oracle=sets))
            once = gt.get_leaf_counts()

            def run():
                gt.reset_counts()
                gt.query_packed(seq, off, thr, paired=True, pair_mode=mode)
                res = gt.query_packed(seq, off, thr, want_hits=True, want_scores=True, paired=True, pair_mode=mode)
                return res, gt.last_capacity(), gt.get_leaf_counts()
            (offs, leaves, _), c, counts = with_knobs(gt, {**knobs, "PFQ_HIT_SLOTS": "0"}, run)
            assert c["attempts"] == 2 and c["hit_cursor"] > 0, (path, block, thr, mode, c)
            assert counts == doubled(once), (path, block, thr, mode)
            want = [sorted(s) for s in
                    [sets[2 * f] | sets[2 * f + 1] if mode == "either" else sets[2 * f] & sets[2 * f + 1] for f in range(len(pairs))]]
            assert [leaves[int(offs[f]):int(offs[f + 1])].tolist() for f in range(len(pairs))] == want


@pytest.mark.parametrize("path,block", HIT_MODES)
def test_hit_retry_natural_on_stored_counts(families, tmp_path, path, block):
    """A database saved with stored counts, reopened: its first PFQ_WANT_HITS call sizes the hit buffer for 2 hits per read,
    the family reads have about 8, so the block runs twice; the counters end at stored + this block's counts."""
    genomes, ot, gt, _ = families
    reads = make_reads(genomes[:32], 700, 0, 150, K, errors=False)[:700]     # (the close families: about 8 leaves per read)
    seq, off = pack_reads(reads)
    want_hits, want_counts = oracle_result(ot, reads, 1.0)
    assert len(want_hits) > 2 * len(reads) + 1024
    gt.set_path(-1)
    gt.reset_counts()
    gt.query_packed(seq, off, 1.0)
    d = str(tmp_path / "db")
    gt.save(d)
    t2 = BloomTree.load(d)
    try:
        assert t2.get_leaf_counts() == want_counts
        t2.set_path(path)
        if block is not None:
            t2.set_option("PFQ_BLOCK", block)
        offs, leaves = t2.query_packed(seq, off, 1.0, want_hits=True)
        c = t2.last_capacity()
        assert c["attempts"] == 2 and c["hit_cap"] < c["hit_cursor"], (path, block, c)
        assert hits_of(offs, leaves) == want_hits
        assert t2.get_leaf_counts() == doubled(want_counts), (path, block)
        offs, leaves = t2.query_packed(seq, off, 1.0, want_hits=True)   # sized from the first call: one attempt
        assert t2.last_capacity()["attempts"] == 1
        assert t2.get_leaf_counts() == [(t, 3 * n) for t, n in want_counts]
    finally:
        t2.close()


def test_hit_slots_apply_to_the_first_attempt_only(families):
    """PFQ_HIT_SLOTS far below the hits: the retry sizes itself from the cursor (a second overflow would be an error)."""
    genomes, ot, gt, reads = families
    gt.set_path(1)
    seq, off = pack_reads(reads)
    want_hits, want_counts = oracle_result(ot, reads, 0.3)

    def run():
        gt.reset_counts()
        offs, leaves = gt.query_packed(seq, off, 0.3, want_hits=True)
        return hits_of(offs, leaves), gt.get_leaf_counts(), gt.last_capacity()
    hits, counts, c = with_knobs(gt, {"PFQ_HIT_SLOTS": "1"}, run)
    assert (hits, counts) == (want_hits, want_counts)
    assert c["attempts"] == 2 and c["hit_cap"] == 1 < c["hit_cursor"], c
