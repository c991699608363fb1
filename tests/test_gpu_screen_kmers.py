"""The lean dense screen of k_classify at threshold 1 (2 k-mers of 32 reads a pass instead of 4 of 16) against
the CPU oracle, on the bucketed path.  The screen is a necessary condition only, so the lean build (PFQ_SCREEN_KMERS=2) and the
dense one (=4) must give the oracle's hit lists and per-leaf counts on the same call, the same all-hit reads and bytes, and the
lean build at least as many candidates.  BloomTree.screen_info() says which build a call ran and the tree's E, the expected
false candidates of a random read after four rows; the rule (E <= 2^-10, rows of <= 32 words, one leaf group, the pair
pipeline) is restated here on the CPU."""
import numpy as np
import pytest

from oracle import pfq_oracle as orc
from test_gpu_capacity import check_overflow
from test_gpu_parity import RNG, check_query, gpu_tree, oracle_tree, rand_dna
from test_gpu_regimes import with_knobs

pytestmark = pytest.mark.gpu

K, H = 21, 10
LEAN, DENSE = 2, 4
PASS = 32          # reads of a pass of the lean screen
E_MAX = 2.0 ** -10


class Tree:
    def __init__(self, genomes, nbits, h=H):
        self.genomes, self.nbits = genomes, nbits
        self.ot, ids = oracle_tree(genomes, K, nbits, h)
        self.gt = gpu_tree(genomes, ids, K, nbits, h)

    def fills(self):
        """Set bits / nbits of every leaf's filter, from the oracle's filters."""
        ot = self.ot
        rows = (np.ascontiguousarray(ot.bits[ot.filter_of[v]], dtype=np.uint64).view(np.uint8) for v in ot.leaves_dfs())
        return [int(np.unpackbits(row).sum()) / self.nbits for row in rows]

    def E(self):
        return sum(f ** 4 for f in self.fills())


def genomes_of(n, lo, hi):
    return [rand_dna(int(RNG.integers(lo, hi))) for _ in range(n)]


@pytest.fixture(scope="module")
def t128(gpu):
    """128 leaves, rw = 4: one lane a read in the AND stage.  Filters about 2 % full."""
    t = Tree(genomes_of(128, 2000, 2600), 1 << 20)
    yield t
    t.gt.close()


@pytest.fixture(scope="module")
def t300(gpu):
    """300 leaves, rw = 16: four lanes a read, two sub-passes of 16 reads issued together."""
    t = Tree(genomes_of(300, 2000, 2400), 1 << 19)
    yield t
    t.gt.close()


@pytest.fixture(scope="module")
def t1024(gpu):
    """1024 leaves, rw = 32: eight lanes a read, four sub-passes of 8 reads, two at a time."""
    t = Tree(genomes_of(1024, 2000, 2200), 1 << 18)
    yield t
    t.gt.close()


@pytest.fixture(scope="module")
def t8(gpu):
    """Eight leaves built from one genome among 128: a read of it has eight pairs, a pass of 32 such reads 256."""
    genomes = genomes_of(128, 2000, 2600)
    for i in (9, 20, 33, 47, 64, 90, 101, 127):
        genomes[i] = genomes[3]
    t = Tree(genomes, 1 << 20)
    yield t
    t.gt.close()


def exact(g, length, strand):
    o = int(RNG.integers(0, len(g) - length + 1))
    r = g[o:o + length]
    return orc.revcomp(r) if strand else r


def other_base(b):
    return b"ACGT"[(b"ACGT".index(bytes([b])) + 1) % 4:][:1]


def prefix_read(g):
    """22 bases of a genome (its k-mers 1 and 2), then random: passes the lean screen for the genome's leaf, hits nothing."""
    o = int(RNG.integers(0, len(g) - 150))
    return g[o:o + K + 1] + rand_dna(150 - K - 1)


def third_kmer_broken(g):
    """A 150 bp read of the genome with base 23 substituted: k-mers 1 and 2 are the genome's, k-mers 3 .. 23 are not."""
    o = int(RNG.integers(0, len(g) - 150))
    return g[o:o + K + 1] + other_base(g[o + K + 1]) + g[o + K + 2:o + 150]


def with_n(g):
    r = bytearray(exact(g, 150, 0))
    r[int(RNG.integers(0, 150))] = ord("N")
    return bytes(r)


def mix(genomes, n):
    """n reads, every kind in turn (so that any prefix of the list holds them all): positives of both strands, random reads,
    reads without a k-mer, of one and of two k-mers, 100 and 150 bp, with an N, and the two lean-only kinds; returns the reads and how
    many of them pass the lean screen for a leaf without being able to hit it."""
    kinds = [
        lambda g: exact(g, 150, 0), lambda g: exact(g, 150, 1), lambda g: rand_dna(150), lambda g: rand_dna(K - 1),
        lambda g: exact(g, K, 0), lambda g: rand_dna(K), lambda g: exact(g, K + 1, 1), lambda g: rand_dna(K + 1),
        with_n, prefix_read, third_kmer_broken, lambda g: rand_dna(150), lambda g: b"", lambda g: exact(g, 100, 0),
        lambda g: rand_dna(150),
    ]
    reads, lean_only = [], 0
    for i in range(n):
        kind = kinds[i % len(kinds)]
        reads.append(kind(genomes[int(RNG.integers(0, len(genomes)))]))
        lean_only += kind in (prefix_read, third_kmer_broken)
    return reads, lean_only


def run(t, reads, kmers, knobs=None, thr=1.0, block="0"):
    """One call on the bucketed path with PFQ_SCREEN_KMERS = kmers (None: the rule), checked against the oracle per read and
    per leaf; returns the call's statistics and the k-mers a read its dense screen took."""
    knobs = {"PFQ_BLOCK": block, **(knobs or {})}
    if kmers is not None:
        knobs["PFQ_SCREEN_KMERS"] = str(kmers)

    def call():
        st = check_query(t.gt, t.ot, reads, thr, path=1)
        assert st.path == 1, st.path
        return st, t.gt.screen_info()["kmers"]
    return with_knobs(t.gt, knobs, call)


def lean_against_dense(t, reads, lean_only=0, knobs=None):
    (s2, k2), (s4, k4) = run(t, reads, LEAN, knobs), run(t, reads, DENSE, knobs)
    assert (k2, k4) == (LEAN, DENSE), (k2, k4)
    print("candidates lean / dense / hits:", s2.n_candidates, s4.n_candidates, s2.n_hits)
    assert (s2.n_hits, s2.n_allhit_reads, s2.algorithmic_bytes) == (s4.n_hits, s4.n_allhit_reads, s4.algorithmic_bytes)
    assert s2.n_candidates >= s4.n_candidates >= s4.n_hits, (s2.n_candidates, s4.n_candidates, s4.n_hits)
    # (a read whose first two k-mers are a leaf's is a candidate of the lean build whether it hits or not)
    assert s2.n_candidates >= s2.n_hits + lean_only, (s2.n_candidates, s2.n_hits, lean_only)
    return s2, s4


# ---------------------------------------------------------------------------------------------------------------
# knob 2 against knob 4 on the same call: row widths x read counts
# ---------------------------------------------------------------------------------------------------------------
COUNTS = [1, 31, 32, 33, 63, 2049]  # a partial last group; more groups than one trip of a wave (2049 reads: 65 groups)


@pytest.mark.parametrize("n_reads", COUNTS)
def test_rw4(t128, n_reads):
    assert t128.gt.screen_info()["rw"] == 4
    lean_against_dense(t128, *mix(t128.genomes, n_reads))


@pytest.mark.parametrize("n_reads", COUNTS)
def test_rw16(t300, n_reads):
    assert t300.gt.screen_info()["rw"] == 16
    lean_against_dense(t300, *mix(t300.genomes, n_reads))


@pytest.mark.parametrize("n_reads", COUNTS)
def test_rw32(t1024, n_reads):
    assert t1024.gt.screen_info()["rw"] == 32
    lean_against_dense(t1024, *mix(t1024.genomes, n_reads))


def test_lean_only_candidates_are_dropped_by_the_dense_screen(t128):
    """Prefix reads and reads with a broken third k-mer alone: candidates of the lean build, (nearly) none of the dense one's,
    hits of neither."""
    g = t128.genomes
    reads = [prefix_read(g[i % 128]) for i in range(200)] + [third_kmer_broken(g[(7 * i) % 128]) for i in range(200)]
    s2, s4 = lean_against_dense(t128, reads, 400)
    assert s2.n_hits == 0 and s4.n_candidates < 40, (s2.n_hits, s4.n_candidates)


# ---------------------------------------------------------------------------------------------------------------
# the rule left to itself
# ---------------------------------------------------------------------------------------------------------------
def test_rule_sparse_tree(t128):
    e = t128.E()
    assert e <= E_MAX / 4, e  # (well inside the rule: 128 leaves about 2.3 % full)
    info = t128.gt.screen_info()
    assert abs(info["E"] - e) <= 1e-9 * e, (info, e)
    reads, _ = mix(t128.genomes, 500)
    st, kmers = run(t128, reads, None)
    assert kmers == LEAN
    assert run(t128, reads, 0)[1] == LEAN  # (0 is the rule as well)


def test_rule_full_tree(gpu):
    """128 leaves at least 6 % full: 128 x 0.06^4 = 1.7e-3 > 2^-10, so the dense screen stays; knob 2 still forces the lean one."""
    t = Tree(genomes_of(128, 2000, 2600), 1 << 17)
    try:
        fills = t.fills()
        assert min(fills) >= 0.06 and t.E() > 1.7 * E_MAX, (min(fills), t.E())
        info = t.gt.screen_info()
        assert abs(info["E"] - t.E()) <= 1e-9 * t.E() and info["rw"] == 4, info
        reads, lean_only = mix(t.genomes, 700)
        assert run(t, reads, None)[1] == DENSE
        lean_against_dense(t, reads, lean_only)
    finally:
        t.gt.close()


def test_rule_rows_of_64_words(gpu):
    """2048 leaves: rw = 64, the frontier words of 32 reads do not fit the wave's LDS — the dense screen, whatever the knob."""
    t = Tree(genomes_of(2048, 200, 400), 120011, 4)
    try:
        info = t.gt.screen_info()
        assert info["rw"] == 64 and info["groups"] == 1 and info["E"] <= E_MAX and abs(info["E"] - t.E()) <= 1e-9 * t.E(), info
        reads, _ = mix(t.genomes, 600)
        assert run(t, reads, None)[1] == DENSE
        assert run(t, reads, LEAN)[1] == DENSE
    finally:
        t.gt.close()


# ---------------------------------------------------------------------------------------------------------------
# reservations and fallbacks
# ---------------------------------------------------------------------------------------------------------------
def eightfold_reads(t, n_pos):
    g = t.genomes[3]
    return [g[o:o + 150] for o in range(50, 50 + 11 * n_pos, 11)]


def test_a_pass_of_256_pairs(t8):
    """32 consecutive reads that each pass the 8 copies of one genome: eight chunks in one reservation; then passes that mix
    such reads with negatives and lean-only candidates."""
    reads = eightfold_reads(t8, 2 * PASS)
    more, lean_only = mix(t8.genomes, 90)
    reads += more + eightfold_reads(t8, 5)
    s2, s4 = lean_against_dense(t8, reads, lean_only)
    assert s2.n_hits >= 8 * (2 * PASS + 5)
    assert s2.pair_stage & 0x8 and s4.pair_stage & 0x8  # both builds emitted pairs a pass at a time


@pytest.mark.parametrize("knobs", [{"PFQ_BATCH_EMIT": "0"}, {"PFQ_SPLIT_RECORDS": "0"}, {"PFQ_RECORD_GB": "0"}],
                         ids=["per_read_loop", "records_by_k_classify", "no_record_buffer"])
def test_fallback_paths(t8, knobs):
    """The per-read loop takes the frontier words the lean screen left (no batched emission; k_classify hashing the reads
    itself); without a record buffer the pairs are emitted all the same and k_verify hashes again."""
    reads = eightfold_reads(t8, PASS + 3)
    more, lean_only = mix(t8.genomes, 150)
    lean_against_dense(t8, reads + more, lean_only, knobs)


def test_pair_buffer_full(t8):
    """PFQ_PAIR_SLOTS at 0, two reservations and just below the demand with the lean build: the reads of a pass whose pairs
    find no slot go down the per-read loop, which certifies inline."""
    reads = eightfold_reads(t8, 3 * PASS)
    more, _ = mix(t8.genomes, 400)
    check_overflow(t8.gt, t8.ot, reads + more, 1.0, "pair", knobs={"PFQ_SCREEN_KMERS": "2", "PFQ_BATCH_EMIT": "1"})
    assert run(t8, reads + more, LEAN, {"PFQ_PAIR_SLOTS": "64"})[1] == LEAN


# ---------------------------------------------------------------------------------------------------------------
# builds that have no lean screen
# ---------------------------------------------------------------------------------------------------------------
def test_threshold_below_one_and_block_mode(t8):
    reads, _ = mix(t8.genomes, 400)
    reads += eightfold_reads(t8, 40)
    for kmers in (None, LEAN):
        assert run(t8, reads, kmers, thr=0.7)[1] == 0       # the counting screen
        st, k = run(t8, reads, kmers, block="1")
        assert st.tile_mode == 2 and k == DENSE, (st.tile_mode, k)


def test_two_level_tree(gpu):
    """More than 2048 leaves: the leaf groups' launches (k_classify<LIST>) keep the dense screen."""
    t = Tree(genomes_of(2100, 200, 400), 60013, 4)
    try:
        reads, _ = mix(t.genomes, 600)
        for kmers in (None, LEAN):
            st, k = run(t, reads, kmers)
            assert st.leaf_groups >= 2 and k == DENSE, (st.leaf_groups, k)
    finally:
        t.gt.close()
