"""Packed tile entries at theta = 1: k_tile_bin<.., 0, PACK> writes five 24-bit entries and a round number per
16 bytes, k_tile_test<0, .., PACK> reads them.  Every comparison is of per-leaf counts and per-read hit lists against the
oracle, with PFQ_ENTRY_PACK 2 and 0, and pfq_stats.entry_pack asserted both ways; set_path(1) and PFQ_BLOCK=0 everywhere.

The tree of most cases is the 8-leaf, 3-tile one of test_gpu_tile_stream (2^21 + 12345 bits, k = 21, 10 hashes): its k_tile_bin
build is 16 x 2048, a round's budget KB = 1536 * 3 / 10 = 460 k-mers.  Its third tile is nearly empty, so the two full tiles
take half the probes each where the plan expects a third: a bin of 2048 overflows in a round of more than ~400 k-mers, and
a bucket in any chunk of more than ~170 k-mers.  The parity cases run through those fallbacks on purpose; the format
case keeps every column under both limits (asserted: no pair takes the fallback) so that a bucket holds every probe."""
import collections

import numpy as np
import pytest

import entry_pack_ref as ref
import test_gpu_tile_stream as ts
from oracle import pfq_oracle as orc
from phagefilter_amd import pack_reads
from test_gpu_parity import check_query, gpu_tree, oracle_tree
from test_gpu_regimes import build_id, mutate, with_knobs

pytestmark = pytest.mark.gpu

K, H, NBITS, SEEDS = ts.K, ts.H, ts.NBITS, ts.SEEDS
RNG = np.random.default_rng(20261019)
KB_SMALL = (2048 - 512) * 3 // H          # k-mer budget of a round on the 3-tile tree (tile_bin_kmer_budget)
FORMATS = ("2", "0")


def dna(n):
    return RNG.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(n)).astype(np.uint8).tobytes()


def cut(g, length, n):
    return [g[int(o):int(o) + length] for o in RNG.integers(0, len(g) - length + 1, n)]


class Case:
    """Reads for a tree; the oracle's answer is computed once (ts.oracle_result) and shared by both formats."""

    def __init__(self, tree, reads):
        self.gt, self.ot, self.ids = tree.gt, tree.ot, tree.ids
        self.reads = reads
        self.seq, self.off = pack_reads(reads)
        self.oracle = {}


def run_both(case, knobs=None, calls=1, tile_mode=1):
    """The case with packed and with 32-bit entries against the oracle; the stats of both runs."""
    want = ts.oracle_result(case, 1.0)
    stats = {}
    for fmt in FORMATS:
        def run():
            for _ in range(calls):
                got = ts.run_query(case, 1.0, tile_mode=tile_mode)
            return got, case.gt.last_stats()
        got, st = with_knobs(case.gt, {"PFQ_BLOCK": "0", "PFQ_ENTRY_PACK": fmt, **(knobs or {})}, run)
        ts.assert_same(got, want, f"PFQ_ENTRY_PACK={fmt} vs oracle")
        assert st.entry_pack == (fmt == "2"), (fmt, st.entry_pack)
        stats[fmt] = st
    return want, stats


@pytest.fixture(scope="module")
def small(gpu):
    """The all-sparse tree and the reads of test_gpu_tile_stream."""
    s = ts.Shared()
    s.genomes = [ts.dna(n + K - 1) for n in ts.KMERS]
    s.ot, s.ids = oracle_tree(s.genomes, K, NBITS, H, SEEDS)
    s.gt = gpu_tree(s.genomes, s.ids, K, NBITS, H, SEEDS)
    s.reads, s.leaf, s.subst = ts.make_reads(s.genomes)
    s.seq, s.off = pack_reads(s.reads)
    s.oracle = {}
    yield s
    s.gt.close()


@pytest.fixture(scope="module")
def long_tree(gpu):
    """Genomes long enough for a 20 kbp read and for 3 kbp reads (dense columns: the generic tester)."""
    s = ts.Shared()
    s.genomes = [dna(20000 + K - 1), dna(6000), dna(600 + K - 1)]
    s.ot, s.ids = oracle_tree(s.genomes, K, NBITS, H, SEEDS)
    s.gt = gpu_tree(s.genomes, s.ids, K, NBITS, H, SEEDS)
    yield s
    s.gt.close()


# ---------------------------------------------------------------------------------------------------------------
# format
# ---------------------------------------------------------------------------------------------------------------
def format_reads(genomes):
    """At most ~100 k-mers a column.  A bucket has room for as many entries as the plan gives it words: a third of the
    chunk's probes + 8 deviations + 64 + ..., 575 entries at 100 k-mers, and a full tile takes half the probes, 498 +- 16.
    Rounds end by the 16-pair cap (21 and 26 bp: 1 and 6 k-mers a read) or with the column; one column has a single pair."""
    g, rng = genomes, np.random.default_rng(7)
    cut_ = lambda s, length, n: [s[int(o):int(o) + length] for o in rng.integers(0, len(s) - length + 1, n)]
    return (cut_(g[0], 120, 1) + [g[1]] * 2 + cut_(g[2], 40, 5) + cut_(g[3], 60, 1) + [g[4]] * 2 + cut_(g[5], 21, 96) + cut_(g[6], 110, 1) +
            cut_(g[7], 26, 17) + [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 80).astype(np.uint8)) for _ in range(20)])


def read_offsets(read, cache):
    """[tile] -> sorted tile offsets of every probe of every k-mer of the read, from the oracle's probe indices."""
    if read not in cache:
        idx = []
        for km in orc.get_kmers(read, K):
            idx += orc.probe_indices(SEEDS[0], SEEDS[1], H, NBITS, orc.get_lex_less(km))
        idx = np.array(idx, dtype=np.int64)
        cache[read] = [np.sort(idx[idx >> 20 == t] & ((1 << 20) - 1)) for t in range(3)]
    return cache[read]


def test_bucket_format(small):
    case = Case(small, format_reads(small.genomes))
    want = ts.oracle_result(case, 1.0)
    got, st = with_knobs(case.gt, {"PFQ_BLOCK": "0", "PFQ_ENTRY_PACK": "2"}, lambda: (ts.run_query(case, 1.0), case.gt.last_stats()))
    ts.assert_same(got, want, "packed vs oracle")
    assert st.entry_pack == 1 and st.n_fallback_pairs == 0 and st.tile_passes_launched == 1, (st.entry_pack, st.n_fallback_pairs)
    n_chunks = case.gt.tile_bucket(0, 0, max_words=0)["n_chunks"]
    assert n_chunks >= 7
    cache, expected, buckets = {}, {}, {}
    residues, round_ends = collections.Counter(), collections.Counter()
    for c in range(n_chunks):
        for t in range(3):
            b = buckets[c, t] = case.gt.tile_bucket(c, t, max_words=1 << 16)
            assert b["packed"] and b["fill"] <= b["cap"] and b["fill"] % 4 == 0 and len(b["words"]) == b["fill"], (c, t, b["fill"], b["cap"])
            p0 = np.append(b["round_p0"], b["n"])
            assert 0 < b["n_rounds"] <= ref.PACK_ROUNDS and p0[0] == 0 and (np.diff(p0) > 0).all() and (np.diff(p0) <= ref.PACK_PAIRS).all(), p0
            for r in range(b["n_rounds"]):   # what the oracle says the run of (round r, tile t) holds: (pair of the round, offset)
                run = [ref.entry(int(p - p0[r]), int(o)) for p in range(p0[r], p0[r + 1])
                       for o in read_offsets(case.reads[int(b["reads"][p])], cache)[t]]
                expected[c, t, r] = sorted(run)
                residues[len(run) % 5] += bool(run)
                if t == 0:
                    kmers = sum(len(case.reads[int(b["reads"][p])]) - K + 1 for p in range(p0[r], p0[r + 1]))
                    nxt = len(case.reads[int(b["reads"][p0[r + 1]])]) - K + 1 if p0[r + 1] < b["n"] else None
                    round_ends["column" if nxt is None else ("cap" if p0[r + 1] - p0[r] == ref.PACK_PAIRS else "budget")] += 1
                    assert kmers <= KB_SMALL and (nxt is None or p0[r + 1] - p0[r] == ref.PACK_PAIRS or kmers + nxt > KB_SMALL), (c, r, kmers, nxt)
    print("run lengths mod 5:", dict(residues), "rounds ended by:", dict(round_ends))
    assert all(residues[m] > 0 for m in range(5)), residues
    assert round_ends["cap"] > 0 and round_ends["column"] > 0, round_ends
    assert any(b["n"] == 1 for b in buckets.values())
    for (c, t), b in buckets.items():
        e, tags = ref.unpack(b["words"])
        assert (tags < b["n_rounds"]).all() and (np.diff(tags) >= 0).all(), (c, t, tags)
        p0 = np.append(b["round_p0"], b["n"])
        ids, _ = ref.split(e)
        assert (ids < (p0[tags + 1] - p0[tags])[:, None]).all(), (c, t)
        at = 0
        for r in range(b["n_rounds"]):
            exp = expected[c, t, r]
            nv = (len(exp) + 4) // 5
            assert (tags[at:at + nv] == r).all() and (at + nv == len(tags) or tags[at + nv] > r), (c, t, r)
            flat = e[at:at + nv].reshape(-1)
            assert sorted(flat[:len(exp)].tolist()) == exp, (c, t, r)
            # (a round may bring the nearly empty third tile nothing: no vector at all)
            assert not exp or (flat[len(exp):] == flat[len(exp) - 1]).all(), (c, t, r, "padding repeats the run's last entry")
            at += nv
        assert at == len(tags), (c, t)


# ---------------------------------------------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------------------------------------------
def test_pipeline_regimes(small):
    """The reads of test_gpu_tile_stream: a column with one pair, one with more than 32 x 1024 pairs (a second group), one
    without pairs; exact and one-substitution reads interleaved in the same rounds — only the substituted pairs fail."""
    want = ts.assert_preconditions(small)
    per_read = np.diff(want[1])
    assert (small.leaf == 3).sum() == 1 and ((small.leaf == 0) & ~small.subst).sum() > 32 * 1024
    assert (per_read[small.subst] == 0).all() and (per_read[(small.leaf >= 0) & ~small.subst] >= 1).all()
    i = np.flatnonzero(small.subst)
    assert (small.leaf[i - 1] == small.leaf[i]).all() and not small.subst[i - 1].any(), "a substituted read follows its exact twin"
    run_both(small)


@pytest.mark.parametrize("fmt", FORMATS)
def test_three_tester_builds(small, fmt):
    """The slots-only build, PFQ_TILE_STREAM=0 and PFQ_TILE_LISTS=0, with one test block (it meets every task and switch)."""
    seen = []

    def three():   # (the format is chosen before the tester's build: the stats of the last of the three runs, PFQ_TILE_LISTS=0)
        out = ts.check_three_builds(small, {"PFQ_TEST_BLOCKS": "1"})
        seen.append(small.gt.last_stats().entry_pack)
        return out
    with_knobs(small.gt, {"PFQ_ENTRY_PACK": fmt}, three)
    assert seen == [int(fmt == "2")], seen


@pytest.mark.parametrize("fmt", FORMATS)
def test_several_passes_two_calls(small, fmt):
    """PFQ_TILE_ENTRIES small enough for several passes: the second call launches as many as the first one needed."""
    seen = []

    def three():
        out = ts.check_three_builds(small, {"PFQ_TILE_ENTRIES": "4000000", "PFQ_TEST_BLOCKS": "1"}, calls=2)
        seen.append(small.gt.last_stats().entry_pack)
        return out
    on, generic = with_knobs(small.gt, {"PFQ_ENTRY_PACK": fmt}, three)
    assert on["passes"] > 1 and generic["passes"] > 1, (on, generic)
    assert seen == [int(fmt == "2")], seen


def test_short_reads_cap_ends_rounds(small):
    """Reads of 25 bp have 5 k-mers: the budget would take 92 pairs a round, the format takes 16."""
    assert KB_SMALL // (25 - K + 1) > ref.PACK_PAIRS
    reads = [r for g in small.genomes for r in cut(g, 25, 400 if len(g) > 100 else 40)]
    reads += [mutate(r, 1) for r in reads[::3]] + [dna(25) for _ in range(100)]
    run_both(Case(small, reads))


def test_thousand_copies_overflow(small):
    """A thousand copies of one read: its probes come a thousand times, LDS bins and buckets overflow and the dropped pairs
    take the fallback."""
    r = small.genomes[5][100:160]
    reads = [r] * 1000 + [mutate(r, 1)] * 20 + cut(small.genomes[6], 60, 50)
    _, stats = run_both(Case(small, reads))
    assert all(st.n_fallback_pairs > 0 for st in stats.values()), {f: st.n_fallback_pairs for f, st in stats.items()}


def test_one_long_read(long_tree):
    """One 20 kbp read: 19 980 k-mers, 44 partial rounds of one pair (id 0); and its substituted twin beside it."""
    g = long_tree.genomes[0]
    r = g[10:20010]
    assert len(r) - K + 1 > 40 * KB_SMALL
    want, _ = run_both(Case(long_tree, [r]))
    assert np.diff(want[1]).tolist() == [1]
    want, _ = run_both(Case(long_tree, [r, mutate(r, 1), orc.revcomp(r)]))
    assert np.diff(want[1]).tolist() == [1, 0, 1]


def test_more_than_256_rounds(long_tree):
    """A chunk of 3 kbp reads: 2980 k-mers are 7 rounds a pair, the tag names 256 — the rest of the chunk takes the fallback."""
    g = long_tree.genomes[1]
    reads = cut(g, 3000, 60)
    assert (3000 - K + 1) // KB_SMALL * len(reads) > ref.PACK_ROUNDS
    reads += [mutate(r, 1) for r in reads[:10]]
    case = Case(long_tree, reads)
    _, stats = run_both(case)
    assert stats["2"].n_fallback_pairs > 0
    # (buckets overflow on this tree in either format: that the round limit was reached is read off the chunk itself)
    st = with_knobs(case.gt, {"PFQ_BLOCK": "0", "PFQ_ENTRY_PACK": "2"}, lambda: (ts.run_query(case, 1.0), case.gt.last_stats())[1])
    chunks = [case.gt.tile_bucket(c, 0, max_words=0) for c in range(case.gt.tile_bucket(0, 0, max_words=0)["n_chunks"])]
    big = max(chunks, key=lambda b: b["n"])
    assert big["packed"] and big["n"] >= 60 and big["n_rounds"] == ref.PACK_ROUNDS, (big["n"], big["n_rounds"])
    last = int(big["round_p0"][-1])                  # round 255 binned (a piece of) this pair: every later pair is flagged
    assert last < big["n"] - 1 and st.n_fallback_pairs >= big["n"] - 1 - last, (last, big["n"], st.n_fallback_pairs)

def test_mixed_sparse_dense_tree(gpu):
    """The tree of test_gpu_tile_lists: columns with slots and dense columns in one pass."""
    m = ts.Shared()
    m.genomes = [ts.dna(n + K - 1) for n in ts.MIXED_KMERS]
    m.ot, m.ids = oracle_tree(m.genomes, K, NBITS, H, SEEDS)
    m.gt = gpu_tree(m.genomes, m.ids, K, NBITS, H, SEEDS)
    try:
        reads = [g[o:o + 100] for g in m.genomes for o in range(0, max(1, len(g) - 100), 9)] + [dna(100) for _ in range(50)]
        reads += [mutate(r, 1) for r in reads[::5]]
        _, stats = run_both(Case(m, reads))
        info = m.gt.tile_lists_info()
        assert info["list_tiles"] > 0 and info["dense_tiles"] > 0 and not stats["2"].pair_stage & ts.STREAM_BIT, info
    finally:
        m.gt.close()


# One tree per build of k_tile_bin that theta = 1 reaches outside block mode: the largest filter of each, in tiles.  (The 8 x 128
# build would hold 281 tiles in LDS; the host runs LDS-tile passes up to 255.)  PFQ_BIN_NARROW=3: the 8 x 256 build.
SHAPES = [(18, 16, 2048, {}), (36, 16, 1024, {}), (72, 16, 512, {}), (144, 16, 256, {}), (255, 8, 128, {}), (18, 8, 256, {"PFQ_BIN_NARROW": "3"})]


@pytest.mark.parametrize("tiles,waves,cap,knobs", SHAPES)
def test_bin_shapes(gpu, tiles, waves, cap, knobs):
    s = ts.Shared()
    s.genomes = [dna(700), dna(650)]
    s.genomes.append(s.genomes[0][:300] + dna(350))
    s.ot, s.ids = oracle_tree(s.genomes, K, tiles << 20, H, SEEDS)
    s.gt = gpu_tree(s.genomes, s.ids, K, tiles << 20, H, SEEDS)
    try:
        reads = [r for g in s.genomes for r in cut(g, 150, 500)] + cut(s.genomes[0], 100, 100) + cut(s.genomes[1], 400, 30)
        reads += [mutate(r, 1) for r in reads[::4]] + [dna(150) for _ in range(50)]
        _, stats = run_both(Case(s, reads), knobs)
        assert all(st.tile_bin_build == build_id(waves, cap) for st in stats.values()), [hex(st.tile_bin_build) for st in stats.values()]
    finally:
        s.gt.close()


# ---------------------------------------------------------------------------------------------------------------
# the default choice
# ---------------------------------------------------------------------------------------------------------------
def test_default_choice(gpu):
    """PFQ_ENTRY_PACK=1 (and unset) on the flagship's bin build, 16 x 512: KB = 384 * 40 / 10 = 1536 k-mers a round, so a call
    packs from 96 k-mers a read (16 pairs are no cap) to 190 (a chunk stays under 256 rounds): 150 bp yes, 25 bp no."""
    tiles = 40
    genomes = [dna(900), dna(800)]
    ot, ids = oracle_tree(genomes, K, tiles << 20, H, SEEDS)
    gt = gpu_tree(genomes, ids, K, tiles << 20, H, SEEDS)
    try:
        for length, packed in ((150, True), (25, False)):
            reads = [r for g in genomes for r in cut(g, length, 300)]
            reads += [mutate(r, 1) for r in reads[::4]]
            for knobs in ({"PFQ_ENTRY_PACK": "1"}, {}):
                st = with_knobs(gt, {"PFQ_BLOCK": "0", **knobs}, lambda: check_query(gt, ot, reads, 1.0, path=1))
                assert (st.path, st.tile_mode, st.tile_bin_build) == (1, 1, build_id(16, 512))
                assert st.entry_pack == packed, (length, knobs, st.entry_pack)
    finally:
        gt.close()
