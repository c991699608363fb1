"""The stage between k_classify and the certificates on the bucketed path, against the CPU oracle: the records of the reads'
last windows (k_tail_records: passes of 16 reads x 4 k-mers, 4 x 16 and 2 x 32, chosen per pair) and the sort of the deferred
pairs by leaf (k_bucket_scatter: an LDS histogram per slice of 8192 slots while the buckets fit one, one global atomic per
pair beyond).  Each case compares per-leaf counts and every read's hit set with the oracle (check_query / check_overflow) and
asserts through pfq_stats.pair_stage that the intended tail shapes and sort kernel ran."""
import pytest

from oracle import pfq_oracle as orc
from test_gpu_capacity import check_overflow, close_families, family_reads, guarded  # noqa: F401  (guarded: a fixture)
from test_gpu_parity import RNG, check_query, gpu_tree, make_reads, oracle_tree, rand_dna
from test_gpu_regimes import with_knobs

pytestmark = pytest.mark.gpu

K, H, NBITS = 21, 7, 1 << 21
SORT_SLICED, SORT_PER_PAIR = 1, 2               # pfq_stats.pair_stage, bits 0-1
SHAPE_4, SHAPE_16, SHAPE_32 = 0x10, 0x20, 0x40  # bits 4-6
SLICE = 8192                                     # slots of a block's slice (pfq_kernels.hip: SORT_SLICE)
MAX_LDS_BUCKETS = 4096                           # (SORT_LDS_BUCKETS)


def exact_reads(g, n, length):
    out = []
    for i in range(n):
        o = int(RNG.integers(0, len(g) - length + 1))
        r = g[o:o + length]
        out.append(orc.revcomp(r) if i % 2 else r)
    return out


def shuffled(reads):
    order = RNG.permutation(len(reads))
    return [reads[i] for i in order]


def tail_of(length, k):
    return (length - k + 1) & 63


def host_batch_tails(reads, k):
    """setup_pairs(): tails of up to 32 k-mers are batched when the call's average read length makes such a tail, else up to 16."""
    avg = sum(len(r) for r in reads) // len(reads)
    tl = tail_of(avg, k) if avg >= k else 0
    return 32 if 16 < tl <= 32 else 16


def expected_shapes(reads, k):
    """Shapes that serve at least one read of `reads`, all of which are deferred (exact substrings of a genome)."""
    bt, bits = host_batch_tails(reads, k), 0
    for r in reads:
        n = len(r) - k + 1
        tl = n & 63
        if n > 64 and 0 < tl <= bt:
            bits |= SHAPE_4 if tl <= 4 else (SHAPE_16 if tl <= 16 else SHAPE_32)
    return bits


def run_pairs(gt, ot, reads, thr=1.0, knobs=None):
    knobs = {"PFQ_BLOCK": "0", **(knobs or {})}
    st = with_knobs(gt, knobs, lambda: check_query(gt, ot, reads, thr, path=1))
    assert st.path == 1, st.path
    return st


@pytest.fixture(scope="module")
def small(gpu):
    genomes = [rand_dna(4000) for _ in range(6)]
    genomes[4] = genomes[1]  # two identical genomes: their reads are deferred for two leaves
    ot, ids = oracle_tree(genomes, K, NBITS, H)
    gt = gpu_tree(genomes, ids, K, NBITS, H)
    yield genomes, ot, gt
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# last windows
# ---------------------------------------------------------------------------------------------------------------
# read length at k = 21 -> k-mers in the last window, and the shape that serves it when the call holds this length alone
TAILS = [(149, 1, SHAPE_4), (150, 2, SHAPE_4), (152, 4, SHAPE_4), (153, 5, SHAPE_16), (164, 16, SHAPE_16), (165, 17, SHAPE_32),
         (180, 32, SHAPE_32), (181, 33, 0)]


@pytest.mark.parametrize("length,tail,shape", TAILS)
def test_one_tail_length(small, length, tail, shape):
    genomes, ot, gt = small
    assert tail_of(length, K) == tail
    reads = []
    for g in genomes[:4]:
        reads += exact_reads(g, 150, length)
    reads += [rand_dna(length) for _ in range(50)]
    reads = shuffled(reads)
    assert expected_shapes(reads[:1], K) in (shape, 0) and expected_shapes(reads, K) == shape
    st = run_pairs(gt, ot, reads)
    assert st.pair_stage >> 4 == shape >> 4, (length, hex(st.pair_stage))
    assert st.pair_stage & 3 == SORT_SLICED, hex(st.pair_stage)


def test_reads_of_one_window_have_no_tail(small):
    genomes, ot, gt = small
    reads = []
    for length in (K, K + 1, 40, 83, 84):  # at most 64 k-mers
        reads += exact_reads(genomes[2], 60, length)
    st = run_pairs(gt, ot, shuffled(reads))
    assert st.pair_stage >> 4 == 0, hex(st.pair_stage)


def test_every_tail_length_in_one_call(small):
    """Trimmed reads: every shape in one launch, chosen per pair; the 181 bp reads outweigh the rest so that the host asks for
    tails of up to 32."""
    genomes, ot, gt = small
    reads = []
    for length, _, _ in TAILS:
        for g in genomes[:3]:
            reads += exact_reads(g, 40, length)
    reads += exact_reads(genomes[3], 700, 181) + exact_reads(genomes[0], 40, 84) + make_reads(genomes, 0, 30, 150, K)
    reads = shuffled(reads)
    assert host_batch_tails(reads, K) == 32
    st = run_pairs(gt, ot, reads)
    assert st.pair_stage >> 4 == (SHAPE_4 | SHAPE_16 | SHAPE_32) >> 4, hex(st.pair_stage)
    # ... and with tails of up to 16 only (uniformly many of each length): the 17 .. 32 k-mer tails stay with k_classify
    reads = []
    for length, _, _ in TAILS:
        reads += exact_reads(genomes[0], 60, length)
    reads = shuffled(reads)
    assert host_batch_tails(reads, K) == 16
    st = run_pairs(gt, ot, reads)
    assert st.pair_stage >> 4 == (SHAPE_4 | SHAPE_16) >> 4, hex(st.pair_stage)
    # lengths drawn from 100 .. 150
    reads = []
    for g in genomes[:4]:
        for _ in range(200):
            reads += exact_reads(g, 1, int(RNG.integers(100, 151)))
    st = run_pairs(gt, ot, shuffled(reads))
    assert st.pair_stage >> 4 == expected_shapes(reads, K) >> 4, hex(st.pair_stage)


def test_tail_batching_off(small):
    genomes, ot, gt = small
    reads = shuffled(exact_reads(genomes[0], 200, 150))
    st = run_pairs(gt, ot, reads, knobs={"PFQ_NO_TAIL_BATCH": "1"})
    assert st.pair_stage >> 4 == 0, hex(st.pair_stage)


@pytest.mark.parametrize("k,length", [(20, 150), (64, 129), (64, 194)])
def test_short_tail_other_k(gpu, k, length):
    assert 1 <= tail_of(length, k) <= 4 and length - k + 1 > 64
    genomes = [rand_dna(3000) for _ in range(5)]
    ot, ids = oracle_tree(genomes, k, NBITS, H)
    gt = gpu_tree(genomes, ids, k, NBITS, H)
    try:
        reads = []
        for g in genomes:
            reads += exact_reads(g, 120, length)
        reads += [rand_dna(length) for _ in range(40)]
        st = run_pairs(gt, ot, shuffled(reads))
        assert st.pair_stage >> 4 == SHAPE_4 >> 4, hex(st.pair_stage)
    finally:
        gt.close()


def test_read_deferred_for_two_leaves(small):
    """genomes[1] == genomes[4]: both pairs of a read name the same last window; it is written twice, same values."""
    genomes, ot, gt = small
    reads = shuffled(exact_reads(genomes[1], 300, 150) + exact_reads(genomes[1], 100, 160) + exact_reads(genomes[0], 50, 150))
    st = run_pairs(gt, ot, reads)
    assert st.n_hits >= 2 * 400
    assert st.pair_stage >> 4 == (SHAPE_4 | SHAPE_16) >> 4, hex(st.pair_stage)


# ---------------------------------------------------------------------------------------------------------------
# the sort by leaf
# ---------------------------------------------------------------------------------------------------------------
def small_genomes(n):
    return [rand_dna(int(RNG.integers(200, 400))) for _ in range(n)]


@pytest.mark.parametrize("n_leaves,n_pos", [(1, 300), (1, 2 * SLICE + 77), (2, 9000), (64, SLICE - 100), (64, 3 * SLICE + 1), (1024, 3000),
                                            (2048, 3000)])
def test_leaf_counts_and_pair_counts(gpu, n_leaves, n_pos):
    """Sub-buckets on (1, 2, 64 leaves: 64, 128, 1024 buckets) and off; fewer pairs than a slice, several slices with a partial
    last one."""
    genomes = small_genomes(n_leaves)
    ot, ids = oracle_tree(genomes, K, 60013, 4)
    gt = gpu_tree(genomes, ids, K, 60013, 4)
    try:
        reads = make_reads(genomes, n_pos, n_pos // 10 + 5, 150, K, errors=False)
        st = run_pairs(gt, ot, reads)
        assert st.pair_stage & 3 == SORT_SLICED, hex(st.pair_stage)
        assert gt.last_capacity()["pairs_sorted"] >= min(n_pos, n_pos * 150 // 400), gt.last_capacity()
    finally:
        gt.close()


@pytest.mark.parametrize("thr", [1.0, 0.7])
def test_every_positive_read_from_one_leaf(gpu, thr):
    """One bucket of 1024 takes every block's whole slice (and, at 0.7, every miss word)."""
    genomes = small_genomes(1024)
    ot, ids = oracle_tree(genomes, K, 60013, 4)
    gt = gpu_tree(genomes, ids, K, 60013, 4)
    try:
        reads = shuffled(exact_reads(genomes[700], 2 * SLICE + 500, 150) + [rand_dna(150) for _ in range(500)])
        st = run_pairs(gt, ot, reads, thr)
        assert st.pair_stage & 3 == SORT_SLICED, hex(st.pair_stage)
        assert gt.last_capacity()["pairs_sorted"] >= 2 * SLICE + 500
    finally:
        gt.close()


@pytest.mark.parametrize("thr", [0.7, 0.3])
def test_miss_words_reserved_per_slice(gpu, thr):
    genomes = small_genomes(64)
    ot, ids = oracle_tree(genomes, K, 60013, 4)
    gt = gpu_tree(genomes, ids, K, 60013, 4)
    try:
        reads = make_reads(genomes, SLICE + 3000, 400, 150, K)
        st = run_pairs(gt, ot, reads, thr)
        assert st.pair_stage & 3 == SORT_SLICED, hex(st.pair_stage)
    finally:
        gt.close()


@pytest.mark.parametrize("thr", [1.0, 0.7])
def test_voided_reservations_and_overflow(gpu, thr):
    """PFQ_PAIR_SLOTS at 0, a few reservations and just below the demand: voided slots inside the slices, the rest inline."""
    genomes = close_families(4)
    ot, ids = oracle_tree(genomes, K, 131071, 7)
    gt = gpu_tree(genomes, ids, K, 131071, 7)
    try:
        check_overflow(gt, ot, family_reads(genomes), thr, "pair")
        assert gt.last_stats().pair_stage & 3 == SORT_SLICED
    finally:
        gt.close()


@pytest.mark.parametrize("thr", [1.0, 0.7])
def test_guard_columns_second_launch(guarded, thr):
    """Guard pairs are sorted by a second launch on the same cursors; owner_sorted carries their leaf pair."""
    genomes, ot, gt, reads = guarded
    st = run_pairs(gt, ot, reads, thr)
    assert st.pair_stage & 3 == SORT_SLICED, hex(st.pair_stage)
    assert gt.last_capacity()["guard_cursor"] > 0, gt.last_capacity()


@pytest.mark.parametrize("n_families,thr,sort", [(4, 1.0, SORT_SLICED), (4, 0.3, SORT_SLICED), (40, 1.0, SORT_PER_PAIR)])
def test_block_mode_keys(gpu, n_families, thr, sort):
    """PFQ_BLOCK=1: buckets by (block of 8 leaves, candidate mask), 256 per block — an LDS histogram up to 16 blocks, the
    per-pair kernel beyond."""
    genomes = close_families(n_families, length=1200)
    n_blocks = (len(genomes) + 7) // 8
    assert (n_blocks * 256 <= MAX_LDS_BUCKETS) == (sort == SORT_SLICED)
    ot, ids = oracle_tree(genomes, K, 131071, 7)
    gt = gpu_tree(genomes, ids, K, 131071, 7)
    try:
        reads = make_reads(genomes, 1500, 150, 150, K)
        st = run_pairs(gt, ot, reads, thr, knobs={"PFQ_BLOCK": "1"})
        assert st.tile_mode == 2, st.tile_mode
        assert st.pair_stage & 3 == sort, hex(st.pair_stage)
    finally:
        gt.close()
