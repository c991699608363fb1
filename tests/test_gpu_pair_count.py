"""Pair slots reserved ahead by the batched emission of k_classify at threshold 1 (PFQ_PAIR_AHEAD) against the
CPU oracle, on the bucketed path.  A wave's range of reserved slots may now be longer than one chunk of 32 and outlive the pass
that reserved it: emit_pass, the per-read loop and the voiding at the wave's end all take their slots from it.  Results must
not depend on A, on the grid (PFQ_CLASSIFY_BLOCKS: with the built-in grid every wave of a small input screens one group of
reads and never reserves ahead), on the screen build or on the pair buffer's capacity; BloomTree.pair_info() says what A a
call used and how many reservations its classify launches made.
(The bucket histogram made from the pair buffer by a kernel of its own, the other half of the plan, was measured and not
built — DESIGN.md §9 — so nothing here sets PFQ_COUNT_LATER or PFQ_COUNT_BLOCKS.)"""
import numpy as np
import pytest

from phagefilter_amd import pack_reads
from test_gpu_capacity import check_overflow, close_families, oracle_result
from test_gpu_capacity import guarded as guarded  # noqa: F401  (the guarded tree of the capacity tests, a fixture)
from test_gpu_parity import RNG, gpu_tree, hits_of, make_reads, oracle_tree, rand_dna
from test_gpu_regimes import family_genomes, with_knobs

pytestmark = pytest.mark.gpu

K, NBITS, H = 21, 131071, 7
CHUNK = 32   # slots of a reservation's unit (PAIR_RESERVE)
WAVES = 8    # PFQ_CLASSIFY_BLOCKS=2: two blocks of four waves


def exact(g, length):
    o = int(RNG.integers(0, len(g) - length + 1))
    return g[o:o + length]


def mixed_reads(genomes, n_pos=800):
    """About 1500 reads: 150 bp positives (some with an N, a substitution, lowercase, reverse complements) and randoms, reads
    shorter than k, of k .. k + 3 bases, of 300 - 400 bases, and positives of every length in between."""
    reads = make_reads(genomes, n_pos, 250, 150, K)
    for d in range(4):
        reads += [exact(genomes[int(RNG.integers(0, len(genomes)))], K + d) for _ in range(10)] + [rand_dna(K + d) for _ in range(5)]
    for length in (300, 351, 400):
        reads += make_reads(genomes, 20, 4, length, K)
    reads += [exact(genomes[int(RNG.integers(0, len(genomes)))], int(RNG.integers(K, 260))) for _ in range(300)]
    order = RNG.permutation(len(reads))
    return [reads[i] for i in order]


class Case:
    """A tree, a block of reads and the oracle's answer to it, computed once."""

    def __init__(self, genomes, reads=None, *, nbits=NBITS, h=H, trees=None):
        self.genomes = genomes
        if trees is None:
            self.ot, ids = oracle_tree(genomes, K, nbits, h)
            self.gt = gpu_tree(genomes, ids, K, nbits, h)
            self.own = True
        else:
            self.ot, self.gt = trees
            self.own = False
        self.answers = {}
        self.reads = reads if reads is not None else mixed_reads(genomes)

    def close(self):
        if self.own:
            self.gt.close()

    def run(self, knobs, thr=1.0, reads=None):
        """One call on the bucketed path under `knobs`: hit lists and leaf counts == the oracle's; returns the CSR, the
        statistics, the capacities and pair_info()."""
        reads = self.reads if reads is None else reads
        key = (id(reads), thr)
        if key not in self.answers:
            self.answers[key] = (reads, pack_reads(reads), oracle_result(self.ot, reads, thr))
        _, (seq, off), (want_hits, want_counts) = self.answers[key]
        gt = self.gt

        def call():
            gt.reset_counts()
            gt.set_path(1)
            offs, leaves = gt.query_packed(seq, off, thr, want_hits=True)
            return (np.array(offs), np.array(leaves)), gt.get_leaf_counts(), gt.last_stats(), gt.last_capacity(), gt.pair_info()
        csr, counts, st, cap, info = with_knobs(gt, {"PFQ_BLOCK": "0", **knobs}, call)
        assert st.path == 1, st.path
        assert counts == want_counts, knobs
        first = self.answers.setdefault(("csr",) + key, csr)
        if first is csr:
            assert hits_of(*csr) == want_hits, knobs
        else:  # (the lists are ascending within a read: every later call must give the first call's arrays)
            assert np.array_equal(first[0], csr[0]) and np.array_equal(first[1], csr[1]), knobs
        assert info[0] == 0 and info[3] == 0, info
        return csr, st, cap, info


def settings():
    """PFQ_SCREEN_KMERS x PFQ_CLASSIFY_BLOCKS x PFQ_PAIR_AHEAD, then the per-read loop for every survivor and k_classify
    hashing the reads itself, both on two blocks of the lean build."""
    out = []
    for screen in ("2", "4"):
        for blocks in (None, "2"):
            for ahead in ("0", "8"):
                out.append({"PFQ_SCREEN_KMERS": screen, "PFQ_PAIR_AHEAD": ahead, **({"PFQ_CLASSIFY_BLOCKS": blocks} if blocks else {})})
    for variant in ({"PFQ_BATCH_EMIT": "0"}, {"PFQ_SPLIT_RECORDS": "0"}):
        for ahead in ("0", "8"):
            out.append({"PFQ_SCREEN_KMERS": "2", "PFQ_CLASSIFY_BLOCKS": "2", "PFQ_PAIR_AHEAD": ahead, **variant})
    return out


def every_emitter(case, *, leaf_groups=1, guards=False):
    sorted_by_screen = {}
    small = {}
    for knobs in settings():
        _, st, cap, info = case.run(knobs)
        assert st.leaf_groups == leaf_groups, st.leaf_groups
        ahead = int(knobs["PFQ_PAIR_AHEAD"])
        assert info[1] == (0 if knobs.get("PFQ_BATCH_EMIT") == "0" else ahead), (knobs, info)
        assert info[2] > 0 and cap["pair_cursor"] % CHUNK == 0 and cap["pair_cursor"] <= cap["pair_cap"], (knobs, info, cap)
        # the deferred pairs are the screen's candidates, however they were emitted and whatever was reserved for them
        screen = st.leaf_groups > 1 or knobs["PFQ_SCREEN_KMERS"]
        assert sorted_by_screen.setdefault(screen, cap["pairs_sorted"]) == cap["pairs_sorted"], (knobs, cap)
        waves = WAVES * leaf_groups
        if "PFQ_CLASSIFY_BLOCKS" in knobs and not guards:
            assert cap["pair_cursor"] - cap["pairs_sorted"] <= waves * (ahead + 1) * CHUNK, (knobs, cap)
        if "PFQ_CLASSIFY_BLOCKS" not in knobs and leaf_groups == 1:
            # the built-in grid gives every wave one group at most: nothing is reserved ahead, whatever A
            # (leaf groups: the coarse launch lists a group's reads in whatever order its waves run)
            key = knobs["PFQ_SCREEN_KMERS"]
            assert small.setdefault(key, (info[2], cap["pair_cursor"])) == (info[2], cap["pair_cursor"]), (knobs, info, cap)


# ---------------------------------------------------------------------------------------------------------------
# case 1: parity in every emitter
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def t70(gpu):
    c = Case([rand_dna(int(RNG.integers(2800, 3200))) for _ in range(70)])
    yield c
    c.close()


@pytest.fixture(scope="module")
def fam(gpu):
    """Families of 8 strains: a read of one passes about 8 leaves, a pass of 32 reads emits far more than 32 pairs."""
    c = Case(close_families(4) + family_genomes(2))
    yield c
    c.close()


def test_four_leaves_with_sub_buckets(gpu):
    c = Case([rand_dna(int(RNG.integers(2800, 3200))) for _ in range(4)])
    try:
        every_emitter(c)
    finally:
        c.close()


def test_seventy_leaves(t70):
    every_emitter(t70)


def test_families(fam):
    every_emitter(fam)
    _, st, cap, _ = fam.run({"PFQ_SCREEN_KMERS": "2", "PFQ_CLASSIFY_BLOCKS": "2", "PFQ_PAIR_AHEAD": "8"})
    assert cap["pairs_sorted"] > 4 * len(fam.reads) // 2, cap  # (several pairs a positive read)


def test_guard_columns(guarded):  # noqa: F811
    genomes, ot, gt, _ = guarded
    every_emitter(Case(genomes, trees=(ot, gt)), guards=True)
    assert gt.last_capacity()["guard_cursor"] > 0


def test_leaf_groups(gpu):
    """1100 leaves with a coarse level from 1024 on: two leaf groups, whose launches take the reads the coarse launch listed
    (k_classify<LIST>; groups hold at least 1024 columns, so this tree has short genomes and small filters)."""
    genomes = [rand_dna(int(RNG.integers(200, 400))) for _ in range(1100)]
    genomes[1050] = genomes[3]
    c = Case(genomes, make_reads(genomes, 1200, 200, 150, K) + [exact(genomes[3], 150) for _ in range(100)], nbits=60013, h=4)
    try:
        c.gt.set_option("PFQ_COARSE_MIN_LEAVES", "1024")
        every_emitter(c, leaf_groups=2)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------
# case 3: reserving ahead really happens and stays bounded
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("screen", ["2", "4"])
def test_reserving_ahead_saves_reservations(t70, screen):
    reads = make_reads(t70.genomes, 3600, 491, 150, K)
    assert len(reads) == 4096
    base = {"PFQ_SCREEN_KMERS": screen, "PFQ_CLASSIFY_BLOCKS": "2"}
    seen = {}
    for ahead in (0, 8, 16):
        _, st, cap, info = t70.run({**base, "PFQ_PAIR_AHEAD": str(ahead)}, reads=reads)
        print("A", ahead, "reservations", info[2], "cursor", cap["pair_cursor"], "sorted", cap["pairs_sorted"])
        assert info[1] == ahead, info
        assert cap["pair_cursor"] % CHUNK == 0, cap
        assert cap["pairs_sorted"] >= 3000, cap
        assert 0 <= cap["pair_cursor"] - cap["pairs_sorted"] <= WAVES * (ahead + 1) * CHUNK, (ahead, cap)
        seen[ahead] = (info[2], cap["pairs_sorted"])
    assert seen[0][1] == seen[8][1] == seen[16][1], seen
    # a wave has 4096 / 8 / (32 or 16) groups; every second or so needs a reservation at A = 0, one in four at the most at A = 8
    assert seen[8][0] * 3 <= seen[0][0] and seen[16][0] <= seen[8][0], seen
    assert seen[0][0] >= seen[0][1] // (2 * CHUNK), seen


def test_pair_ahead_is_clamped(t70):
    assert t70.run({"PFQ_PAIR_AHEAD": "1000", "PFQ_CLASSIFY_BLOCKS": "2"})[3][1] == 16
    assert t70.run({"PFQ_CLASSIFY_BLOCKS": "2"})[3][1] == 8   # unset


# ---------------------------------------------------------------------------------------------------------------
# case 4: full buffer
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("screen", ["2", "4"])
def test_pair_buffer_full(fam, screen):
    """PFQ_PAIR_SLOTS at 0, two reservations and just below the demand: a reservation that asks for slots ahead is refused
    as a whole, the reads whose pairs lie below the buffer's end are emitted, the others certified inline."""
    check_overflow(fam.gt, fam.ot, fam.reads, 1.0, "pair",
                   knobs={"PFQ_PAIR_AHEAD": "8", "PFQ_CLASSIFY_BLOCKS": "2", "PFQ_SCREEN_KMERS": screen})


# ---------------------------------------------------------------------------------------------------------------
# case 5: calls that have no batched emission
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr,block", [(1.0, "1"), (0.7, "0"), (0.3, "0")])
def test_no_reserving_ahead(fam, thr, block):
    _, st, cap, info = fam.run({"PFQ_BLOCK": block, "PFQ_PAIR_AHEAD": "8", "PFQ_CLASSIFY_BLOCKS": "2"}, thr=thr)
    assert info[1] == 0 and info[2] > 0, info
    assert (st.tile_mode == 2) == (block == "1"), st.tile_mode
    assert cap["pair_cursor"] - cap["pairs_sorted"] <= 2 * WAVES * CHUNK, cap  # (thresholds < 1: two launches)
