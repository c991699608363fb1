"""k_tile_bin's round pipeline at threshold 1 (pair entries, tile mode on), against the CPU oracle.

k_tile_bin loads the records of round r + 1 and the pair metadata of round r + 2 while round r bins, and takes them over
before round r's bucket stores; the loads are unconditional (the metadata index clamped to the chunk's last pair, a lane
without a k-mer loading a record of the round), so what is at stake is every edge of a chunk: its first and last round,
rounds that end a chunk of 1, 31, 32, 33 or 1024 pairs, a read split over several rounds, chunks of later passes, and the
overflow fallback.  Each case compares per-leaf counts and every read's hit set with the oracle (check_query) and asserts
the bin build the host launched (tile_bin_build)."""
import pytest

from oracle import pfq_oracle as orc
from test_gpu_parity import RNG, check_query, gpu_tree, make_reads, oracle_tree, rand_dna
from test_gpu_regimes import bin_build, with_knobs

pytestmark = pytest.mark.gpu

K, H = 21, 7
TILE_LOG2_PAIRS = 20
# leaf i gets PAIRS[i] exact positive reads: chunks of 1, 31, 32, 33 pairs, then 1024 + 1; the last leaf's reads include
# LONG reads, each longer than one round's k-mer budget (at most 2048 k-mers with 16 waves, 1024 with 8)
PAIRS = (1, 31, 32, 33, 1025, 36)
LONG, LONG_LEN, GENOME_LEN = 4, 5000, 6000
# tiles on both sides of every cutoff of launch_tile_bin at threshold 1 (18 | 19, 36 | 37, 72 | 73, 144 | 145)
TILES = (18, 19, 36, 37, 72, 73, 144, 145)


def exact_reads(g, n, length):
    out = []
    for i in range(n):
        o = int(RNG.integers(0, len(g) - length + 1))
        r = g[o:o + length]
        out.append(orc.revcomp(r) if i % 2 else r)
    return out


def chunk_reads(genomes):
    reads = []
    for g, n in zip(genomes, PAIRS):
        reads += exact_reads(g, n, 150)
    reads += exact_reads(genomes[-1], LONG, LONG_LEN)
    reads += make_reads(genomes, 0, 40, 150, K)  # random reads and the short / empty edge cases
    order = RNG.permutation(len(reads))
    return [reads[i] for i in order]


def run(gt, ot, reads, knobs=None):
    knobs = dict(knobs or {})
    knobs["PFQ_BLOCK"] = "0"
    return with_knobs(gt, knobs, lambda: check_query(gt, ot, reads, 1.0, path=1))


@pytest.mark.parametrize("tiles", TILES)
def test_chunk_edges_every_bin_build(gpu, tiles):
    nbits = tiles << TILE_LOG2_PAIRS
    genomes = [rand_dna(GENOME_LEN) for _ in PAIRS]
    ot, ids = oracle_tree(genomes, K, nbits, H)
    gt = gpu_tree(genomes, ids, K, nbits, H)
    try:
        reads = chunk_reads(genomes)
        st = run(gt, ot, reads)
        assert (st.tile_mode, st.tile_bin_build) == (1, bin_build(tiles)), (tiles, st.tile_mode, hex(st.tile_bin_build))
        # (1025 reads of a 6000 bp genome repeat their k-mers ~25 times: a few buckets of the many-tile builds overflow
        # into the fallback, by design — nearly every pair must still go through the tile passes)
        assert st.n_chunks >= len(PAIRS) + 1 and st.n_fallback_pairs < st.n_candidates // 10, (st.n_chunks, st.n_fallback_pairs)
        # the same reads in another order: other pairs share a round, other chunks end on a partial round
        st = run(gt, ot, reads[::-1])
        assert st.n_fallback_pairs < st.n_candidates // 10
    finally:
        gt.close()


@pytest.mark.parametrize("tiles", (18, 145))
def test_several_passes(gpu, tiles):
    """Bucket space for a fraction of the chunks: the second call launches every pass the first one needed."""
    nbits = tiles << TILE_LOG2_PAIRS
    genomes = [rand_dna(GENOME_LEN) for _ in PAIRS]
    ot, ids = oracle_tree(genomes, K, nbits, H)
    gt = gpu_tree(genomes, ids, K, nbits, H)
    try:
        reads = chunk_reads(genomes)
        # (the 1024-pair chunk alone needs ~1.0 M entries at 18 tiles, ~1.1 M at 145; the call ~1.3 M / ~1.5 M)
        seen = [run(gt, ot, reads, {"PFQ_TILE_ENTRIES": "1200000"}) for _ in range(2)]
        assert seen[0].tile_passes_needed > 1, seen[0].tile_passes_needed
        assert seen[1].tile_passes_launched == seen[0].tile_passes_needed, (seen[1].tile_passes_launched, seen[0].tile_passes_needed)
        assert seen[1].n_fallback_pairs < seen[1].n_candidates // 10, seen[1].n_fallback_pairs
    finally:
        gt.close()


@pytest.mark.parametrize("tiles", (18, 145))
def test_skewed_chunk_overflows_to_the_fallback(gpu, tiles):
    """1100 copies of one positive read in one leaf: their probes land in the same few places of every tile, far beyond
    what a Poisson count sizes the buckets for.  The flagged pairs are certified by the record kernel: same result."""
    nbits = tiles << TILE_LOG2_PAIRS
    genomes = [rand_dna(GENOME_LEN) for _ in range(4)]
    ot, ids = oracle_tree(genomes, K, nbits, H)
    gt = gpu_tree(genomes, ids, K, nbits, H)
    try:
        one = exact_reads(genomes[0], 1, 150)[0]
        reads = [one] * 1100 + exact_reads(genomes[1], 300, 150) + make_reads(genomes, 0, 30, 150, K)
        order = RNG.permutation(len(reads))
        reads = [reads[i] for i in order]
        st = run(gt, ot, reads)
        assert st.tile_mode == 1 and st.n_fallback_pairs > 0, (st.tile_mode, st.n_fallback_pairs)
    finally:
        gt.close()
