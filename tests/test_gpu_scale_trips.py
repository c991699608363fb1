"""The post-stage kernels of a query call — the hit CSR and its scan, the fragment combine, best rows, LCA, taxonomy, abundance
log and coverage sketch — past one trip of their capped grids, past one block of the two-level scan and past one pass of its top
kernel.  Workload W of tests/test_gpu_lca.py has 3 753 units: there every grid-stride loop runs once, every long-row queue is
drained in one trip and the scan has one block.  Here a call is made of copies of W's units (tests/tiled_ref.py; checked against
the plain references in tests/test_tiled_ref_cpu.py), sized by the kernels' own bounds.

The bounds are mirrored below as constants, and every test first asserts, on the expectation alone, that its input crosses its
bound: a later change of a grid cap makes the test say that it no longer tests anything.  Every comparison is exact and covers
every unit.  Nothing expected comes from the library."""
import numpy as np
import pytest

import cover_ref
import tax_ref
import tiled_ref
from oracle import pfq_oracle as orc
from phagefilter_amd import pack_reads
from test_gpu_abund import same as same_abundance
from test_gpu_best import BW, N_LEAVES, ProbeContains, call, check_best_rows, check_consumers, observe, same_call
from test_gpu_build import _dna, _mutate
from test_gpu_cover import same as same_coverage
from test_gpu_lca import K, best_sets, csr_of, knobs, oracle_sets, pair_scores
from test_gpu_paired import combine
from test_gpu_parity import gpu_tree, oracle_tree
from test_gpu_scores import expected_scores
from test_gpu_tax import random_taxonomy

pytestmark = pytest.mark.gpu

# ---- the kernels' bounds (phagefilter_amd/csrc) ------------------------------------------------------------------------------
SCAN_ITEMS = 4096                        # pfq_kernels.hip `constexpr uint32_t SCAN_ITEMS = 4096`: units per block of launch_scan_u32
WAVES_PER_BLOCK = 4                      # pfq_device.h `constexpr uint32_t WAVES_PER_BLOCK = 4`
ROW_SHORT = 64                           # BEST_ROW_SHORT, LCA_ROW_SHORT, TAX_ROW_SHORT, ABUND_ROW_SHORT, PAIR_SHORT: longer rows go to a wave
LONG_QUEUE_ROWS = 1024 * WAVES_PER_BLOCK   # `wblocks = min(ceil(n / WAVES_PER_BLOCK), 1024)` in launch_best_rows, launch_lca_best,
#                                            launch_tax_rows, launch_pair_combine and launch_pair_fill: queued rows per trip
WAVE_GRID_UNITS = 8192 * WAVES_PER_BLOCK   # `min(ceil(n / WAVES_PER_BLOCK), 8192)` in launch_cover_sketch, launch_hit_scores and
#                                            launch_pair_scores: units per trip of the wave-per-unit kernels
HIT_PAIR_GRID = 2048 * 256               # `dim3(2048), dim3(256)` of k_hit_count / k_hit_scatter (launch_hits_csr, launch_hits_fill)
THREAD_GRID_UNITS = 4096 * 256           # `min(ceil(n / 256), 4096)` blocks of k_best_count / k_best_fill, k_lca_best_span, k_pair_count /
#                                            k_pair_fill, and `dim3(4096)` of k_hit_sort
HIST_GRID_UNITS = 1024 * 4096            # `per_block` 4096 (trees of up to 512 nodes) x at most 1024 blocks: lca_map_blocks, launch_tax_rows,
#                                            launch_abund_count
SCAN_TOP_BLOCKS = 1024                   # k_scan_top: `for (b0 = 0; b0 < n_blocks; b0 += 1024)`, s_run carried from pass to pass

FULL = dict(taxa=True, abundance=True, coverage=True, best=True)


class SW:
    """BW (workload W with its references over best rows) and the same for W's fragments; the expectations of the tiled calls."""

    def __init__(self):
        self.bw = BW()
        w = self.w = self.bw.w
        self.gt, self.ot, self.cm, self.nodes = w.gt, w.ot, w.cm, self.bw.ref
        assert 8 * len(self.cm.table) <= 4096 and 8 * self.nodes.n <= 4096 and 8 * N_LEAVES <= 4096   # per_block is 4096 on this tree
        self.pairs, self.preads = w.pairs(), w.pair_reads()
        self.pseq, self.poff = pack_reads(self.preads)
        self.pprobe = ProbeContains(w.ot, self.preads)
        self._paired, self._exp = {}, {}

    def single(self, thr):
        return self.w.sets(thr), self.bw.scores(thr), self.bw.best(thr)

    def paired(self, thr, mode):
        if (thr, mode) not in self._paired:
            frag = combine(self.w.pair_sets(thr), mode)
            scores = pair_scores(self.ot, self.preads, frag, self.pprobe)
            self._paired[thr, mode] = (frag, scores, best_sets(frag, scores))
        return self._paired[thr, mode]

    def sketcher(self):
        return cover_ref.TreeSketcher(self.ot, share=self.bw.cache)

    def expect(self, n, thr, mode=None, whole=False):
        """The call of n units tiled from W's reads (mode: from W's fragments), with its packed block.  whole: the consumers read
        the whole rows (a call without best rows), and the sketch is left out."""
        key = (n, thr, mode, whole)
        if key not in self._exp:
            sets, scores, best = self.paired(thr, mode) if mode else self.single(thr)
            idx = tiled_ref.tile_index(len(sets), n, n)
            kw = dict(pairs=self.pairs) if mode else dict(reads=self.w.reads)
            exp = tiled_ref.Expect(idx, sets, scores, sets if whole else best, n_leaves=N_LEAVES, cm=self.cm, nodes=self.nodes,
                                   sketcher=None if whole else self.sketcher(), **kw)
            exp.seq, exp.off = tiled_ref.pack_units(self.pseq, self.poff, idx, 2) if mode else tiled_ref.pack_units(self.w.seq, self.w.off, idx)
            self._exp = {key: exp}                                    # (the last one only: the large ones are large)
        return self._exp[key]


@pytest.fixture(scope="module")
def sw(gpu):
    x = SW()
    x.gt.set_taxonomy(*x.bw.tax)
    assert x.gt.taxa() == x.nodes.table
    yield x
    x.gt.close()


def row_lengths(offs):
    return (offs[1:] - offs[:-1]).astype(np.int64)


def check_result(gt, res, exp, tag):
    """The call's own result: CSR, scores and leaf counts."""
    offs, leaves, scores = res
    assert offs.shape == exp.offs.shape and np.array_equal(offs, exp.offs), (tag, np.flatnonzero(offs != exp.offs)[:10] if offs.shape == exp.offs.shape else offs.shape)
    assert np.array_equal(leaves, exp.leaves), (tag, np.flatnonzero(leaves != exp.leaves)[:10])
    assert np.array_equal(scores, exp.scores), (tag, np.flatnonzero(scores != exp.scores)[:10])
    assert [n for _, n in gt.get_leaf_counts()] == exp.counts.tolist(), tag


def check_parts(gt, exp, tag, best=True):
    """The consumers: check_consumers of tests/test_gpu_best.py; without best rows or without a sketch, its parts but that one."""
    if exp.sketch is not None and best:
        return check_consumers(gt, exp, tag)
    if best:
        check_best_rows(gt, exp.csr, tag)
    if exp.sketch is not None:
        same_coverage(gt.coverage(), exp.sketch, tag)
    w_last, w_here, w_below, w_any = exp.taxa
    last = gt.last_taxa()
    assert last.dtype == np.uint32 and np.array_equal(last, w_last), (tag, np.flatnonzero(last != w_last)[:10])
    for name, got, want in zip(("here", "below", "any"), gt.taxon_counts(), (w_here, w_below, w_any)):
        assert np.array_equal(got, want), (tag, name, np.flatnonzero(got != want)[:10])
    same_abundance(gt.abundance(200, 0), exp.est, tag)


def check_full(gt, exp, thr, tag, flags=FULL, plain=False, **kw):
    """One call with the consumers against the expectation; plain: and against the same call without them."""
    gt.reset_counts()
    res = call(gt, exp.seq, exp.off, thr, **flags, **kw)
    seen = observe(gt, None)
    check_result(gt, res, exp, tag)
    check_parts(gt, exp, tag, best=bool(flags.get("best")))
    if plain:
        gt.reset_counts()
        p_res = call(gt, exp.seq, exp.off, thr, **kw)
        same_call(seen, observe(gt, None), res, p_res, (tag, "plain"))
    gt.reset_counts()


def check_lca(gt, exp, thr, kind, tag, **kw):
    """One call with the LCA over all hits or over the best: last_lca per unit, here and below per clade."""
    gt.reset_counts()
    res = call(gt, exp.seq, exp.off, thr, lca=kind, **kw)
    check_result(gt, res, exp, (tag, kind))
    got, want = gt.last_lca(), exp.lca[kind]
    assert got.dtype == np.uint32 and got.shape == want.shape, (tag, kind, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, kind, bad[:10], got[bad[:10]], want[bad[:10]])
    here, below = gt.clade_counts()
    assert np.array_equal(here, exp.clades[kind][0]) and np.array_equal(below, exp.clades[kind][1]), (tag, kind)
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# A. the scan's block edges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,blocks", [(4095, 1), (4096, 1), (4097, 2), (8192, 2)])
def test_a_scan_block_edges(sw, n, blocks):
    """One unit short of a scan block, one full block (off[n] is written by the block's last thread), one unit into the second
    block, two full blocks: the best-rows scan and the hit scan; with fragments the mates' scan (2 n) and the fragments' (n)."""
    gt = sw.gt
    cases = [None] + (["either"] if n % SCAN_ITEMS == 0 else [])
    for mode in cases:
        exp = sw.expect(n, 0.7, mode)
        assert exp.n == n and (n + SCAN_ITEMS - 1) // SCAN_ITEMS == blocks and len(exp.offs) == len(exp.csr[0]) == n + 1
        assert row_lengths(exp.csr[0])[:SCAN_ITEMS - 1].any() and row_lengths(exp.offs)[:SCAN_ITEMS - 1].any()
        if blocks > 1:                                                # (something to add beyond the first block's sum)
            assert exp.csr[0][-1] > exp.csr[0][SCAN_ITEMS] > 0 and exp.offs[-1] > exp.offs[SCAN_ITEMS] > 0
        kw = dict(paired=True, mode=mode) if mode else {}
        for path in (0, 1):
            knobs(gt, path, None)
            try:
                check_full(gt, exp, 0.7, (n, mode, path), **kw)
                check_lca(gt, exp, 0.7, "best", (n, mode, path), **kw)
            finally:
                knobs(gt, -1, None)


# ---------------------------------------------------------------------------------------------------------------
# B. the long-row queues
# ---------------------------------------------------------------------------------------------------------------
def test_b_long_row_queues_single_reads(sw):
    """θ 0: every row lists all 80 leaves, so every unit is queued for a wave by k_best_count, k_lca_best_span (and taken whole by
    the others), and the queues are drained in more than two trips."""
    gt, n = sw.gt, 9001
    exp = sw.expect(n, 0.0)
    assert int((row_lengths(exp.offs) > ROW_SHORT).sum()) == n > 2 * LONG_QUEUE_ROWS
    assert 0 < int((row_lengths(exp.csr[0]) > ROW_SHORT).sum()) < n    # best rows: only the units without k-mers keep every leaf
    for path in (0, 1):
        knobs(gt, path, None)
        try:
            check_full(gt, exp, 0.0, ("B", path))
            for kind in ("all", "best"):
                check_lca(gt, exp, 0.0, kind, ("B", path))
        finally:
            knobs(gt, -1, None)
    whole = sw.expect(n, 0.0, whole=True)                             # without best rows the consumers take the 80-leaf rows themselves
    assert whole.log["n_all_leaves"] == n
    check_full(gt, whole, 0.0, ("B", "whole rows"), flags=dict(taxa=True, abundance=True))


@pytest.mark.parametrize("mode", ["either", "both"])
def test_b_long_row_queues_fragments(sw, mode):
    """θ 0 on fragments: every fragment is all-leaf and listed, so k_pair_count queues each of them for k_pair_long."""
    gt, n = sw.gt, 4500
    exp = sw.expect(n, 0.0, mode)
    assert int((row_lengths(exp.offs) > ROW_SHORT).sum()) == n > LONG_QUEUE_ROWS
    best = sw.paired(0.0, mode)[2]
    no_kmers = [f for f, (a, b) in enumerate(sw.pairs) if max(len(a), len(b)) < K]
    assert len(no_kmers) >= 2 and all(len(best[f]) == N_LEAVES for f in no_kmers)   # nothing to score: the best row stays whole
    assert sum(1 for b in best if len(b) < N_LEAVES) >= 600            # the others: the top scorers only
    check_full(gt, exp, 0.0, ("B", mode), paired=True, mode=mode)
    for kind in ("all", "best"):
        check_lca(gt, exp, 0.0, kind, ("B", mode), paired=True, mode=mode)


def test_b_long_rows_that_are_not_all_leaves(gpu):
    """Rows of 70 of 80 leaves — 70 copies of one genome — are the ones the taxonomy's and the abundance log's wave kernels take
    (an all-leaf row is a shortcut for both): more of them than one trip of k_tax_long drains, with and without best rows (the
    copies tie, so a best row is the whole row)."""
    rng = np.random.default_rng(7080)
    family = _dna(rng, 400)
    genomes = [family] * 70 + [_dna(rng, 400) for _ in range(10)]
    genomes = [genomes[i] for i in rng.permutation(N_LEAVES)]
    nbits, h = 20011, 4
    ot, ids = oracle_tree(genomes, K, nbits, h)
    gt = gpu_tree(genomes, ids, K, nbits, h)
    try:
        tax = random_taxonomy(7081, N_LEAVES)
        nodes = tax_ref.Nodes([ot.tax_id[v] for v in ot.leaves_dfs()], *tax)
        gt.set_taxonomy(*tax)
        assert gt.taxa() == nodes.table
        reads = [family[o:o + 120] for o in range(0, 280, 7)]
        reads = [orc.revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
        reads += [g[40:160] for g in genomes if g != family][:6] + [_dna(rng, 120), b"", b"ACGT"]
        sets = oracle_sets(ot, reads, 1.0)
        offs, leaves = csr_of(sets)
        scores = expected_scores(ot, reads, offs, leaves, ProbeContains(ot, reads))
        best = best_sets(sets, scores)
        n = 6400
        idx = tiled_ref.tile_index(len(reads), n, n)
        seq, off = pack_reads(reads)
        for rows in (best, sets):
            exp = tiled_ref.Expect(idx, sets, scores, rows, n_leaves=N_LEAVES, nodes=nodes, reads=reads,
                                   sketcher=cover_ref.TreeSketcher(ot))
            exp.seq, exp.off = tiled_ref.pack_units(seq, off, idx)
            lens = row_lengths(exp.csr[0])
            assert int(((lens > ROW_SHORT) & (lens < N_LEAVES)).sum()) > LONG_QUEUE_ROWS
            assert exp.log["n_ambiguous"] > LONG_QUEUE_ROWS and exp.log["n_all_leaves"] >= 2 and exp.log["n_unique"] >= 6
            check_full(gt, exp, 1.0, ("70 of 80", rows is best), flags=dict(FULL, best=rows is best))
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# C. the wave-per-unit grids
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr,mode", [(0.7, None), (0.3, None), (0.7, "either"), (0.7, "both")])
def test_c_wave_per_unit_grids(sw, thr, mode):
    """More units than one trip of the coverage kernel and of the score kernels (reads and fragments) takes."""
    gt, n = sw.gt, 40003
    exp = sw.expect(n, thr, mode)
    assert exp.n == n > WAVE_GRID_UNITS
    assert int((row_lengths(exp.csr[0])[WAVE_GRID_UNITS:] > 0).sum()) > 1000 and int(exp.offs[-1] - exp.offs[WAVE_GRID_UNITS]) > 1000
    kw = dict(paired=True, mode=mode) if mode else {}
    check_full(gt, exp, thr, ("C", thr, mode), plain=True, **kw)
    check_lca(gt, exp, thr, "best", ("C", thr, mode), **kw)


def test_c_split_into_three_calls(sw):
    """The same units in three calls leave the counters, the estimate and the sketch of the one call."""
    gt, n, thr = sw.gt, 40003, 0.7
    exp = sw.expect(n, thr)
    best_csr = csr_of(sw.bw.best(thr))
    gt.reset_counts()
    for lo, hi in ((0, n // 7), (n // 7, n // 2), (n // 2, n)):
        seq, off = tiled_ref.pack_units(sw.w.seq, sw.w.off, exp.idx[lo:hi])
        call(gt, seq, off, thr, **FULL)
        check_best_rows(gt, tiled_ref.gather_rows(*best_csr, exp.idx[lo:hi]), (lo, hi))
        assert np.array_equal(gt.last_taxa(), exp.taxa[0][lo:hi]), (lo, hi)
    assert [c for _, c in gt.get_leaf_counts()] == exp.counts.tolist()
    for name, got, want in zip(("here", "below", "any"), gt.taxon_counts(), exp.taxa[1:]):
        assert np.array_equal(got, want), name
    same_abundance(gt.abundance(200, 0), exp.est, "split")
    same_coverage(gt.coverage(), exp.sketch, "split")
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# D. the thread-per-unit grids and the hit-pair kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 1])
def test_d_thread_per_unit_grids(sw, path):
    """More units than one trip of k_best_count / k_best_fill, k_hit_sort and the LCA's thread kernels takes, and more hit pairs
    than one trip of k_hit_count / k_hit_scatter."""
    gt, n, thr = sw.gt, 1100003, 0.7
    exp = sw.expect(n, thr)
    assert exp.n == n > THREAD_GRID_UNITS
    lens = row_lengths(exp.offs)
    n_pairs = int(lens[lens < N_LEAVES].sum())                        # (an all-leaf row is not made of hit pairs)
    assert n_pairs > 2 * HIT_PAIR_GRID and len(exp.leaves) > HIT_PAIR_GRID
    assert int((row_lengths(exp.csr[0])[THREAD_GRID_UNITS:] > 0).sum()) > 1000
    knobs(gt, path, None)
    try:
        check_full(gt, exp, thr, ("D", path))
        check_lca(gt, exp, thr, "all", ("D", path))
    finally:
        knobs(gt, -1, None)


# ---------------------------------------------------------------------------------------------------------------
# E. the scan's top kernel and the histogram kernels
# ---------------------------------------------------------------------------------------------------------------
def short_reads(w, n=2000, length=32):
    """Reads of 32 bases (12 k-mers) from W's genomes: exact, with one substitution, reverse-complemented; foreign ones; some
    shorter than k."""
    rng = np.random.default_rng(3232)
    out = []
    for i in range(n - 290):
        g = w.genomes[int(rng.integers(0, len(w.genomes)))]
        o = int(rng.integers(0, len(g) - length + 1))
        r = g[o:o + length]
        if i % 3 == 0:
            r = _mutate(rng, r, 1)
        out.append(orc.revcomp(r) if i % 2 else r)
    out += [_dna(rng, length) for _ in range(250)]
    out += [_dna(rng, int(rng.integers(1, K))) for _ in range(37)] + [b"", b"ACGT", _dna(rng, K - 1)]
    return [out[i] for i in rng.permutation(len(out))]


@pytest.fixture(scope="module")
def short_base(sw):
    reads = short_reads(sw.w)
    sets = oracle_sets(sw.ot, reads, 0.7)
    offs, leaves = csr_of(sets)
    scores = expected_scores(sw.ot, reads, offs, leaves, ProbeContains(sw.ot, reads))
    best = best_sets(sets, scores)
    n_hit = sum(1 for s in sets if 0 < len(s) < N_LEAVES)
    assert n_hit >= 1000 and sum(1 for s in sets if not s) >= 200 and sum(1 for s in sets if len(s) == N_LEAVES) >= 40
    assert sum(1 for s, b in zip(sets, best) if s != b) >= 100 and sum(1 for b in best if 1 < len(b) < N_LEAVES) >= 100
    return reads, pack_reads(reads), sets, scores, best


@pytest.mark.parametrize("n", [4194305, 4198403])
def test_e_scan_top_and_histogram_second_trip(sw, short_base, n):
    """One unit, and one scan block and three units, more than 1024 scan blocks and than 1024 blocks of 4096 units: the second
    pass of k_scan_top's loop starts from the carried s_run, and the LDS-histogram kernels of the LCA, the taxonomy and the
    abundance log take a second trip."""
    gt, thr = sw.gt, 0.7
    reads, (seq, off), sets, scores, best = short_base
    assert n > HIST_GRID_UNITS and (n + SCAN_ITEMS - 1) // SCAN_ITEMS > SCAN_TOP_BLOCKS
    idx = tiled_ref.tile_index(len(reads), n, n)
    hit = np.array([0 < len(s) < N_LEAVES for s in sets])[idx]         # the call's last unit is one with hits: swapped into place
    j = int(np.flatnonzero(hit)[-1])
    idx[j], idx[-1] = idx[-1], idx[j]
    exp = tiled_ref.Expect(idx, sets, scores, best, n_leaves=N_LEAVES, cm=sw.cm, nodes=sw.nodes, reads=reads)
    exp.seq, exp.off = tiled_ref.pack_units(seq, off, idx)
    first = SCAN_TOP_BLOCKS * SCAN_ITEMS                              # the units of the second pass have rows, so s_run matters
    assert exp.offs[first] > 0 and exp.offs[-1] > exp.offs[first] and exp.csr[0][-1] > exp.csr[0][first] > 0
    assert exp.lca["all"][first:].min() != tiled_ref.NO and exp.taxa[0][first:].min() != tiled_ref.NO
    check_full(gt, exp, thr, ("E", n), flags=dict(taxa=True, abundance=True, best=True))
    check_lca(gt, exp, thr, "all", ("E", n))
