"""The probe records of the deferred reads at threshold 1 (k_tail_records: every window of a read, 64 k-mers a pass, plus the
batched last windows) against the CPU oracle, with PFQ_SPLIT_RECORDS at 1 (k_classify only defers) and at 0 (k_classify
hashes the full windows itself).  Every case compares per-leaf counts and every read's hit set with the oracle (check_query /
check_overflow) and asserts through bit 2 of pfq_stats.pair_stage which kernel made the records."""
import pytest

from oracle import pfq_oracle as orc
from test_gpu_capacity import check_overflow, close_families, family_reads, guarded  # noqa: F401  (guarded: a fixture)
from test_gpu_parity import RNG, check_query, gpu_tree, make_reads, oracle_tree, rand_dna
from test_gpu_regimes import with_knobs

pytestmark = pytest.mark.gpu

K, H, NBITS = 20, 7, 1 << 21
SPLIT_BIT = 0x4  # pfq_stats.pair_stage: k_tail_records made the records of the full windows
SPLIT = ["1", "0"]
# read length at k = 20 -> k-mers: none, one, a window less one, one window, a window and one, two windows, two and a last
# window of two, a window and a last window of 17 (100 bp), and sixteen windows less 43
LENGTHS = [(19, 0), (20, 1), (82, 63), (83, 64), (84, 65), (147, 128), (149, 130), (100, 81), (1000, 981), (1500, 1481)]


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


def run(gt, ot, reads, split, *, block=False, knobs=None, records=True):
    """One call on the bucketed path; the split bit must say what PFQ_SPLIT_RECORDS asked for (never without records)."""
    knobs = {"PFQ_BLOCK": "1" if block else "0", "PFQ_SPLIT_RECORDS": split, **(knobs or {})}
    st = with_knobs(gt, knobs, lambda: check_query(gt, ot, reads, 1.0, path=1))
    assert st.path == 1 and (st.tile_mode == 2) == block, (st.path, st.tile_mode)
    assert bool(st.pair_stage & SPLIT_BIT) == (split == "1" and records), (split, hex(st.pair_stage))
    return st


@pytest.fixture(scope="module")
def small(gpu):
    genomes = [rand_dna(4000) for _ in range(6)]
    genomes[4] = genomes[1]  # two identical genomes: their reads are deferred for two leaves
    ot, ids = oracle_tree(genomes, K, NBITS, H)
    gt = gpu_tree(genomes, ids, K, NBITS, H)
    yield genomes, ot, gt
    gt.close()


@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("length,n", LENGTHS)
def test_one_read_length(small, length, n, split):
    genomes, ot, gt = small
    assert max(length - K + 1, 0) == n
    reads = []
    for g in genomes[:4]:
        reads += exact_reads(g, 100, length)
    reads += [rand_dna(length) for _ in range(40)]
    st = run(gt, ot, shuffled(reads), split, records=n >= 1)  # (reads without k-mers defer nothing: no read is served)
    assert st.n_hits >= (500 if n >= 1 else 0)


@pytest.mark.parametrize("split", SPLIT)
def test_every_length_in_one_call(small, split):
    genomes, ot, gt = small
    reads = []
    for length, _ in LENGTHS:
        for g in genomes[:3]:
            reads += exact_reads(g, 40, length)
    for g in genomes[:4]:
        for _ in range(150):
            reads += exact_reads(g, 1, int(RNG.integers(K, 400)))
    reads += make_reads(genomes, 200, 60, 150, K) + [b"", b"ACGT"]
    run(gt, ot, shuffled(reads), split)
    # the 17 .. 32 k-mer last windows stay with the 64-k-mer pass when the host asks for tails of up to 16, and every last
    # window does with the batching off
    run(gt, ot, shuffled(reads), split, knobs={"PFQ_NO_TAIL_BATCH": "1"})


@pytest.mark.parametrize("h", [3, 4, 12, 13])
@pytest.mark.parametrize("split", SPLIT)
def test_hash_counts(gpu, h, split):
    """The carry walk of the records: straight-line builds for 4 .. 12 hashes, the rolled loop beside them."""
    genomes = [rand_dna(3000) for _ in range(5)]
    ot, ids = oracle_tree(genomes, 21, NBITS, h)
    gt = gpu_tree(genomes, ids, 21, NBITS, h)
    try:
        reads = []
        for g in genomes:
            reads += exact_reads(g, 60, 150) + exact_reads(g, 20, 233)
        run(gt, ot, shuffled(reads + [rand_dna(150) for _ in range(40)]), split)
    finally:
        gt.close()


@pytest.fixture(scope="module")
def families(gpu):
    genomes = close_families(4) + [rand_dna(3000) for _ in range(4)]
    ot, ids = oracle_tree(genomes, 21, 131071, 7)
    gt = gpu_tree(genomes, ids, 21, 131071, 7)
    yield genomes, ot, gt, family_reads(genomes)
    gt.close()


@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("block", [False, True])
def test_reads_deferred_for_several_leaves(families, block, split):
    """Families of 8 strains: the pairs of a read fill consecutive slots and only the first of them makes the records."""
    genomes, ot, gt, reads = families
    st = run(gt, ot, reads, split, block=block)
    assert st.n_hits > 2 * len(reads), (st.n_hits, len(reads))  # (most reads pass the 8 leaves of their family)


@pytest.mark.parametrize("split", SPLIT)
@pytest.mark.parametrize("block", [False, True])
def test_pairs_straddle_reservations(families, block, split):
    """PFQ_PAIR_SLOTS at 0, two reservations and just below the demand: full and voided reservations, reads whose pairs lie in
    two of them (hashed twice), and pairs certified inline beside deferred ones."""
    genomes, ot, gt, reads = families
    check_overflow(gt, ot, reads, 1.0, "pair", block=block, knobs={"PFQ_SPLIT_RECORDS": split})


@pytest.mark.parametrize("split", SPLIT)
def test_more_than_2048_leaves(gpu, split):
    """Two leaf groups (k_classify<LIST>): a read listed for both groups is deferred, and hashed, once per group."""
    genomes = [rand_dna(int(RNG.integers(200, 400))) for _ in range(2100)]
    genomes[2090] = genomes[3]
    ot, ids = oracle_tree(genomes, 21, 60013, 4)
    gt = gpu_tree(genomes, ids, 21, 60013, 4)
    try:
        reads = make_reads(genomes, 1500, 150, 150, 21) + exact_reads(genomes[3], 50, 180)
        st = run(gt, ot, reads, split)
        assert st.leaf_groups >= 2, st.leaf_groups
    finally:
        gt.close()


@pytest.mark.parametrize("split", SPLIT)
def test_guarded_tree(guarded, split):
    """Guard pairs live in the second region of the pair buffer, which the record kernel does not walk."""
    genomes, ot, gt, reads = guarded
    run(gt, ot, reads, split)
    check_overflow(gt, ot, reads, 1.0, "guard", knobs={"PFQ_SPLIT_RECORDS": split})


@pytest.mark.parametrize("split", SPLIT)
def test_no_record_buffer(small, split):
    """PFQ_RECORD_GB=0: no records at all, so no record kernel and no split; k_verify hashes the reads again."""
    genomes, ot, gt = small
    reads = []
    for length in (84, 100, 149, 1000):
        reads += exact_reads(genomes[1], 80, length)
    st = run(gt, ot, shuffled(reads), split, knobs={"PFQ_RECORD_GB": "0"}, records=False)
    assert st.pair_stage >> 4 == 0, hex(st.pair_stage)
