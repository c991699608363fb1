"""Batched emission at threshold 1 (k_classify<DEFER> turns the frontier words of a pass's surviving reads into pairs with one
prefix sum and one reservation) against the CPU oracle, with PFQ_BATCH_EMIT at 1 and at 0 (the per-read loop).  Every case
compares per-leaf counts and every read's hit set with the oracle (check_query / check_overflow) and asserts through bit 3 of
pfq_stats.pair_stage whether a pair was emitted by the batched path."""
import pytest

from oracle import pfq_oracle as orc
from phagefilter_amd import pack_reads
from test_gpu_capacity import check_overflow, close_families, family_reads, guarded, oracle_result  # noqa: F401  (guarded: a fixture)
from test_gpu_parity import RNG, check_query, gpu_tree, make_reads, oracle_tree, rand_dna
from test_gpu_record_kernel import exact_reads, shuffled
from test_gpu_regimes import with_knobs

pytestmark = pytest.mark.gpu

K = 21
BATCH_BIT = 0x8  # pfq_stats.pair_stage: at least one pair of the call was written by the batched path
EMIT = ["1", "0"]
PASS = 16        # reads of a pass of the dense screen


def run(gt, ot, reads, emit, *, block=False, knobs=None, batched=None):
    """One call on the bucketed path; bit 3 must say what PFQ_BATCH_EMIT asked for (`batched`: whether a read survives the
    screen at all; never in block mode, which keeps the per-read loop)."""
    knobs = {"PFQ_BLOCK": "1" if block else "0", "PFQ_BATCH_EMIT": emit, **(knobs or {})}
    st = with_knobs(gt, knobs, lambda: check_query(gt, ot, reads, 1.0, path=1))
    assert st.path == 1 and (st.tile_mode == 2) == block, (st.path, st.tile_mode)
    expect = (emit == "1" and not block) if batched is None else (batched and emit == "1" and not block)
    assert bool(st.pair_stage & BATCH_BIT) == expect, (emit, block, hex(st.pair_stage))
    return st


# leaves -> (row words, leaf of the second copy of genome 3): the two copies' columns lie in different quarters of the row
# (a quarter is rw / 4 words = 8 rw columns).  The 6-leaf tree fits one word: its copies share a quarter.
WIDTHS = {6: (4, 5), 100: (4, 90), 200: (8, 150), 300: (16, 250), 600: (32, 500), 1100: (64, 1000)}


@pytest.fixture(scope="module", params=sorted(WIDTHS))
def wide(gpu, request):
    n = request.param
    rw, twin = WIDTHS[n]
    genomes = [rand_dna(int(RNG.integers(300, 500))) for _ in range(n)]
    genomes[twin] = genomes[3]
    ot, ids = oracle_tree(genomes, K, 60013, 4)
    gt = gpu_tree(genomes, ids, K, 60013, 4)
    yield n, rw, genomes, ot, gt
    gt.close()


@pytest.mark.parametrize("emit", EMIT)
def test_row_widths(wide, emit):
    """rw = 4, 8, 16, 32 and 64: a read of the doubled genome has pairs in two quarters of its row, so the prefix sum runs
    across the read's four lanes; reads of the other genomes land in every quarter."""
    n, rw, genomes, ot, gt = wide
    reads = exact_reads(genomes[3], 40, 150)
    for g in (genomes[0], genomes[n // 3], genomes[n // 2], genomes[n - 1]):
        reads += exact_reads(g, 12, 150)
    reads = shuffled(reads + [rand_dna(150) for _ in range(37)])
    st = run(gt, ot, reads, emit)
    assert st.n_hits >= 40 * 2 + 4 * 12
    if n > 6:  # the two copies' columns: different quarters
        cols = sorted({c for r, c in oracle_result(ot, exact_reads(genomes[3], 1, 150), 1.0)[0]})
        assert len(cols) == 2 and cols[0] // (8 * rw) != cols[1] // (8 * rw), (cols, rw)


@pytest.fixture(scope="module")
def small(gpu):
    genomes = [rand_dna(4000) for _ in range(6)]
    genomes[4] = genomes[1]
    ot, ids = oracle_tree(genomes, K, 1 << 21, 7)
    gt = gpu_tree(genomes, ids, K, 1 << 21, 7)
    yield genomes, ot, gt
    gt.close()


def pos(genomes, n):
    return [exact_reads(genomes[i % 4], 1, 150)[0] for i in range(n)]


def neg(n):
    return [rand_dna(150) for _ in range(n)]


@pytest.mark.parametrize("emit", EMIT)
@pytest.mark.parametrize("survivors", [0, 1, 15, 16])
def test_survivors_per_pass(small, survivors, emit):
    """Groups of 16 consecutive reads of which 0, 1, 15 and 16 survive the screen, the survivors at changing places."""
    genomes, ot, gt = small
    reads = []
    for g in range(9):
        odd = (g * 5) % PASS  # the one survivor, or the one read that does not survive
        for j in range(PASS):
            alive = {0: False, 1: j == odd, 15: j != odd, 16: True}[survivors]
            reads += pos(genomes, 1) if alive else neg(1)
    st = run(gt, ot, reads, emit, batched=survivors > 0)
    assert st.n_hits >= 9 * survivors


@pytest.mark.parametrize("emit", EMIT)
@pytest.mark.parametrize("n_reads", [1, 15, 16, 17, 16 * 7 + 5])
def test_read_counts(small, n_reads, emit):
    """The last (or only) group of a call is short; every read of it survives."""
    genomes, ot, gt = small
    st = run(gt, ot, pos(genomes, n_reads), emit)
    assert st.n_hits >= n_reads


@pytest.mark.parametrize("emit", EMIT)
def test_positives_and_negatives_alternate(small, emit):
    genomes, ot, gt = small
    reads = [x for p, q in zip(pos(genomes, 200), neg(200)) for x in (p, q)] + pos(genomes, 3)
    run(gt, ot, reads, emit)


@pytest.mark.parametrize("emit", EMIT)
def test_irregular_reads_inside_a_pass(small, emit):
    """Reads without k-mers (they count at every leaf), of fewer than four k-mers and of many windows among exact reads:
    the irregular ones take the per-read path, the others of their pass the batched one."""
    genomes, ot, gt = small
    reads = pos(genomes, 150) + neg(30) + [b"", b"", b"ACGT", rand_dna(K - 1), rand_dna(K - 1), rand_dna(K), rand_dna(K + 2)]
    for g in genomes[:3]:
        reads += exact_reads(g, 6, 1000) + exact_reads(g, 6, 1500) + exact_reads(g, 6, K) + exact_reads(g, 6, K + 1)
    st = run(gt, ot, shuffled(reads), emit)
    assert st.n_allhit_reads == 5


@pytest.mark.parametrize("emit", EMIT)
def test_no_record_buffer(small, emit):
    """PFQ_RECORD_GB=0: no records, nothing for k_tail_records to make; the pairs are emitted all the same."""
    genomes, ot, gt = small
    st = run(gt, ot, shuffled(pos(genomes, 300) + neg(50)), emit, knobs={"PFQ_RECORD_GB": "0"})
    assert st.pair_stage >> 4 == 0, hex(st.pair_stage)


def test_records_made_by_k_classify(small):
    """PFQ_SPLIT_RECORDS=0: k_classify hashes the deferred reads itself, read by read — no batched emission."""
    genomes, ot, gt = small
    run(gt, ot, shuffled(pos(genomes, 300) + neg(50)), "1", knobs={"PFQ_SPLIT_RECORDS": "0"}, batched=False)


def test_statistics_equal(small):
    """One mixed call with the knob at 1 and at 0: the same candidates, hits, all-hit reads, bytes and pair slots."""
    genomes, ot, gt = small
    reads = shuffled(pos(genomes, 700) + neg(300) + [b"", b"ACGT"] + exact_reads(genomes[2], 10, 1000))
    seen = []
    for emit in EMIT:
        st = run(gt, ot, reads, emit)
        seen.append((st.n_candidates, st.n_hits, st.n_allhit_reads, st.algorithmic_bytes, gt.last_capacity()["pair_cursor"]))
    assert seen[0] == seen[1], seen
    assert seen[0][0] >= 700 and seen[0][4] >= 700


def test_knob_flipped_between_calls(small):
    """Counts accumulate over calls as the oracle's do, whichever path emitted the pairs."""
    genomes, ot, gt = small
    gt.reset_counts()
    gt.set_path(1)
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    try:
        for i, emit in enumerate(["1", "0", "1", "1", "0"]):
            reads = shuffled(pos(genomes, 100 + 16 * i) + neg(40))
            seq, off = pack_reads(reads)
            gt.set_option("PFQ_BATCH_EMIT", emit)
            gt.query_packed(seq, off, 1.0)
            orc.query_batch(ot, reads, 1.0)
            assert gt.get_leaf_counts() == ot.leaf_counts(), (i, emit)
            assert bool(gt.last_stats().pair_stage & BATCH_BIT) == (emit == "1"), (i, emit)
    finally:
        gt.set_option("PFQ_BATCH_EMIT", None)
        gt.set_path(-1)


@pytest.fixture(scope="module")
def families(gpu):
    genomes = close_families(4) + [rand_dna(3000) for _ in range(4)]
    ot, ids = oracle_tree(genomes, K, 131071, 7)
    gt = gpu_tree(genomes, ids, K, 131071, 7)
    yield genomes, ot, gt, family_reads(genomes)
    gt.close()


@pytest.mark.parametrize("emit", EMIT)
@pytest.mark.parametrize("block", [False, True])
def test_several_pairs_per_read(families, block, emit):
    """Families of 8 strains: a pass of 16 reads has up to 128 pairs — several chunks in one reservation, reads that straddle
    two reservations.  Block mode keeps the per-read loop (bit 3 clear) and gives the same results."""
    genomes, ot, gt, reads = families
    st = run(gt, ot, reads, emit, block=block)
    assert st.n_hits > 2 * len(reads), (st.n_hits, len(reads))
    if not block:
        assert st.n_candidates > 4 * len(reads), st.n_candidates  # passes of more than 32 pairs


def test_a_pass_of_128_pairs(families):
    """Sixteen consecutive reads that each pass the 8 strains of one family: T = 128, four chunks at once."""
    genomes, ot, gt, _ = families
    reads = []
    for f in range(4):
        reads += [genomes[8 * f][o:o + 150] for o in range(100, 100 + 40 * PASS, 40)]
    want_hits, _ = oracle_result(ot, reads, 1.0)
    per_read = [sum(1 for r, _ in want_hits if r == i) for i in range(len(reads))]
    assert sum(1 for c in per_read if c >= 7) >= len(reads) // 2, per_read
    for emit in EMIT:
        run(gt, ot, reads, emit)


@pytest.mark.parametrize("block", [False, True])
def test_pair_buffer_full(families, block):
    """PFQ_PAIR_SLOTS at 0, two reservations and just below the demand: passes whose reservation does not fit go down the
    per-read loop, which certifies inline."""
    genomes, ot, gt, reads = families
    check_overflow(gt, ot, reads, 1.0, "pair", block=block, knobs={"PFQ_BATCH_EMIT": "1"})


@pytest.mark.parametrize("emit", EMIT)
def test_more_than_2048_leaves(gpu, emit):
    """Two leaf groups (k_classify<LIST>): a read listed for both groups is emitted once per group, under its own index."""
    genomes = [rand_dna(int(RNG.integers(200, 400))) for _ in range(2100)]
    genomes[2090] = genomes[3]
    ot, ids = oracle_tree(genomes, K, 60013, 4)
    gt = gpu_tree(genomes, ids, K, 60013, 4)
    try:
        reads = make_reads(genomes, 1500, 150, 150, K) + exact_reads(genomes[3], 50, 180)
        st = run(gt, ot, reads, emit)
        assert st.leaf_groups >= 2, st.leaf_groups
    finally:
        gt.close()


@pytest.mark.parametrize("emit", EMIT)
def test_guarded_tree(guarded, emit):
    """k_expand_guards walks the batched pairs: every guard of a pair's leaf becomes a pair of its own."""
    genomes, ot, gt, reads = guarded
    run(gt, ot, reads, emit)
    check_overflow(gt, ot, reads, 1.0, "guard", knobs={"PFQ_BATCH_EMIT": emit})
