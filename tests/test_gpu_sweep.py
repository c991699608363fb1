"""PFQ_WANT_SWEEP: one flagged call at the lowest threshold of a list leaves, per threshold of the list, what a call of its own
at that threshold would count (include/pfq.h "threshold sweep").

Nothing expected here comes from the library.  The rows are the oracle's (oracle_sets), the scores its k-mer by k-mer counts
(expected_scores), the reduction is tests/sweep_ref.py, and tests/test_sweep_cpu.py checks both against the oracle's rows at
every threshold.  Every comparison is exact and covers every unit.  Everything else of a flagged call must be what the same
call gives without the flag.  Workload W and its helpers are those of tests/test_gpu_lca.py and tests/test_gpu_best.py; the
reads are W's plus the 600 noisy ones of tests/test_sweep_cpu.py, which reach every bin."""
import copy
import ctypes as C

import numpy as np
import pytest

import sweep_ref
import tiled_ref
from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_abund import same as same_abundance
from test_gpu_best import ProbeContains, call, observe, same_call
from test_gpu_lca import K, Device, csr_of, knobs, oracle_sets
from test_gpu_scores import expected_scores
from test_gpu_tax import random_taxonomy
from test_gpu_wide_and_shards import _h4_tree
from test_sweep_cpu import LIST, SweepW

pytestmark = pytest.mark.gpu

PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -4, -6
BASE = LIST[0]
# ---- the kernels' bounds (phagefilter_amd/csrc/pfq_sweep.hip, pfq_kernels.h) ----
WAVES_PER_BLOCK = 4                      # pfq_device.h
SWEEP_ROW_SHORT = 64                     # longer rows are queued for a wave
SWEEP_HIST_LDS = 8192                    # bins of `pass` a block counts in LDS
SWEEP_GRID_ROWS = 1024                   # blocks of 256 threads of k_sweep_rows: 256 units per block and trip
SWEEP_GRID_LONG = 1024                   # blocks of WAVES_PER_BLOCK waves of k_sweep_long: that many queued rows per block and trip


def rows_grid_units(n, bins, lds):
    """Units one trip of k_sweep_rows takes in a call of n units (launch_sweep)."""
    per_block = max(256, 8 * bins) if lds and bins <= SWEEP_HIST_LDS else 256
    return min((n + per_block - 1) // per_block, SWEEP_GRID_ROWS) * 256


def long_grid_rows(n, bins, lds):
    """Queued rows one trip of k_sweep_long drains in a call of n units."""
    per_block = max(WAVES_PER_BLOCK, bins // 8) if lds and bins <= SWEEP_HIST_LDS else WAVES_PER_BLOCK
    return min((n + per_block - 1) // per_block, SWEEP_GRID_LONG) * WAVES_PER_BLOCK


@pytest.fixture(scope="module")
def sw(gpu):
    x = SweepW(device=True)
    x.seq, x.off = pack_reads(x.reads)
    yield x
    x.gt.close()


def sweep_call(gt, seq, off, thr=BASE, **kw):
    return call(gt, seq, off, thr, sweep=True, **kw)


def fresh(gt, thresholds=LIST):
    gt.reset_counts()
    gt.set_sweep(thresholds)


def is_zero(s, n_thr, n_leaves):
    return (s["n_units"] == 0 and s["leaf_units"].shape == (n_thr, n_leaves) and
            not any(s[k].any() for k in sweep_ref.READ_OUT))


def oracle_counts(ot, reads, thr):
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    orc.query_batch(ot, reads, thr, threads=8)
    out = [c for _, c in ot.leaf_counts()]
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------
# 1. parity, paths, histogram paths
# ---------------------------------------------------------------------------------------------------------------
def test_parity_with_the_reference_and_with_runs_of_their_own(sw):
    gt, ref = sw.gt, sw.ref()
    fresh(gt)
    assert is_zero(gt.sweep(), len(LIST), sw.n_leaves)                 # before any flagged call: zeros
    res = sweep_call(gt, sw.seq, sw.off)
    seen = observe(gt, None)
    assert np.array_equal(res[0], csr_of(sw.sets(BASE))[0]) and np.array_equal(res[2], sw.scores(BASE))
    got = gt.sweep()
    sweep_ref.same(got, ref, "W + noisy")
    sweep_ref.same(gt.sweep(), ref, "read twice: not consumed")
    gt.reset_counts()
    p_res = call(gt, sw.seq, sw.off, BASE)
    same_call(seen, observe(gt, None), res, p_res, "the same call without the flag")
    for t, thr in enumerate(LIST):
        gt.reset_counts()
        assert gt.query_packed(sw.seq, sw.off, thr) is None
        own = [c for _, c in gt.get_leaf_counts()]
        assert got["leaf_units"][t].tolist() == own == oracle_counts(sw.ot, sw.reads, thr), thr
    gt.reset_counts()


@pytest.mark.parametrize("lds", [None, "0"])
@pytest.mark.parametrize("path,block", [(0, None), (1, "0"), (1, "1")])
def test_paths_and_histogram_paths(sw, path, block, lds):
    gt = sw.gt
    knobs(gt, path, block)
    gt.set_option("PFQ_SWEEP_LDS", lds)
    try:
        fresh(gt)
        sweep_call(gt, sw.seq, sw.off)
        sweep_ref.same(gt.sweep(), sw.ref(), (path, block, lds))
        if path == 0 and lds is None:                                  # through pfq_text_query and the device-resident entry as well
            n = 700
            text = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(sw.reads[:n]))
            assert gt.parse_text(text, "fasta")["n_records"] == n
            fresh(gt)
            gt.query_text(BASE, want_hits=True, want_scores=True, sweep=True)
            cut = int(csr_of(sw.sets(BASE)[:n])[0][-1])
            want = sweep_ref.sweep(sw.rows(BASE)[:n], sw.scores(BASE)[:cut], sw.lengths[:n], K, LIST, sw.n_leaves)
            sweep_ref.same(gt.sweep(), want, "text")
            dev = Device(sw.seq, sw.off)
            try:
                fresh(gt)
                sweep_call(gt, sw.seq, sw.off, dev=dev)
                sweep_ref.same(gt.sweep(), sw.ref(), "device-resident")
            finally:
                dev.close()
    finally:
        gt.set_option("PFQ_SWEEP_LDS", None)
        knobs(gt, -1, None)
        gt.reset_counts()


def test_lists_with_the_ends_of_the_range(sw):
    """Base 0.0: every row lists all 80 leaves and is taken by a wave; 1.5: only the reads without k-mers pass."""
    gt = sw.gt
    thresholds = (0.0, 0.3, 0.7, 1.0, 1.5)
    want = sw.ref(thresholds)
    assert int(want["units_hit"][0]) == len(sw.reads) and int(want["units_hit"][-1]) == 3 and int(want["entries"][-1]) == 3 * sw.n_leaves
    for lds in (None, "0"):
        gt.set_option("PFQ_SWEEP_LDS", lds)
        try:
            fresh(gt, thresholds)
            sweep_call(gt, sw.seq, sw.off, 0.0)
            sweep_ref.same(gt.sweep(), want, ("ends", lds))
            fresh(gt, thresholds)
            sweep_call(gt, sw.seq, sw.off, -1.0)                       # any threshold not above the list's lowest
            sweep_ref.same(gt.sweep(), want, ("ends, base -1", lds))
        finally:
            gt.set_option("PFQ_SWEEP_LDS", None)
    one = sw.ref((1.0,), base=1.0)                                      # one threshold, and the tile path of threshold 1
    fresh(gt, (1.0,))
    sweep_call(gt, sw.seq, sw.off, 1.0)
    sweep_ref.same(gt.sweep(), one, "one threshold")
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 2. call split, replicas
# ---------------------------------------------------------------------------------------------------------------
def test_call_split_and_replicas(sw, tmp_path):
    gt, ref, n = sw.gt, sw.ref(), len(sw.reads)
    fresh(gt)
    lo = 0
    for size in (1, 7, 1000, 1, n):                                    # calls of 1, 7 and 1000 units, then the rest
        hi = min(lo + size, n)
        seq, off = pack_reads(sw.reads[lo:hi])
        sweep_call(gt, seq, off)
        lo = hi
    assert lo == n
    e_seq, e_off = pack_reads([])
    sweep_call(gt, e_seq, e_off)                                       # an empty call adds nothing
    sweep_ref.same(gt.sweep(), ref, "split")
    gt.reset_counts()
    d = str(tmp_path / "db")
    gt.save(d)
    a, b = BloomTree.load(d), BloomTree.load(d)
    try:
        for t in (a, b):
            t.set_sweep(LIST)
        cut = n // 3
        offs = csr_of(sw.sets(BASE))[0]
        for t, (x, y) in ((a, (0, cut)), (b, (cut, n))):
            seq, off = pack_reads(sw.reads[x:y])
            sweep_call(t, seq, off)
        want_b = sweep_ref.sweep(sw.rows(BASE)[cut:], sw.scores(BASE)[int(offs[cut]):], sw.lengths[cut:], K, LIST, sw.n_leaves)
        sweep_ref.same(b.sweep(), want_b, "replica b alone")
        counts_b = b.get_leaf_counts()
        a.sweep_absorb(b)
        sweep_ref.same(a.sweep(), ref, "absorbed")
        assert is_zero(b.sweep(), len(LIST), sw.n_leaves) and b.get_leaf_counts() == counts_b
        a.sweep_absorb(b)                                              # zeroed counters add nothing
        sweep_ref.same(a.sweep(), ref, "absorbed zeros")
        with pytest.raises(PfqError) as e:
            a.sweep_absorb(a)
        assert e.value.code == PFQ_ERR_ARG
        b.set_sweep(LIST[:-1])
        with pytest.raises(PfqError) as e:
            a.sweep_absorb(b)
        assert e.value.code == PFQ_ERR_ARG and "lists differ" in str(e.value)
        sweep_ref.same(a.sweep(), ref, "refused: unchanged")
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. reset, re-size
# ---------------------------------------------------------------------------------------------------------------
def test_reset_and_prune(sw, tmp_path):
    gt = sw.gt
    T, L = len(LIST), sw.n_leaves
    gt.set_sweep([])
    bytes_without = gt.info().device_bytes
    fresh(gt)
    assert gt.info().device_bytes - bytes_without == 8 * ((2 * T + 1) * L + T + 1)   # the state is counted in device_bytes
    sweep_call(gt, sw.seq, sw.off)
    gt.sweep_reset()
    assert is_zero(gt.sweep(), len(LIST), sw.n_leaves)
    sweep_call(gt, sw.seq, sw.off)
    sweep_ref.same(gt.sweep(), sw.ref(), "after sweep_reset: the list stayed")
    gt.reset_counts()
    assert is_zero(gt.sweep(), len(LIST), sw.n_leaves)
    gt.set_sweep(LIST[1:])                                              # a new list replaces the old one and its counters
    assert is_zero(gt.sweep(), len(LIST) - 1, sw.n_leaves)
    gt.set_sweep([])
    assert gt.sweep()["thresholds"].size == 0 and gt.sweep()["leaf_units"].shape == (0, sw.n_leaves)
    # pruned: the leaves change, the counters are made anew for them, the list stays
    d = str(tmp_path / "db")
    gt.save(d)
    pt, ot = BloomTree.load(d), copy.deepcopy(sw.ot)
    try:
        pt.reset_counts()
        pt.set_sweep(LIST)
        seq, off = pack_reads(sw.reads[:500])
        sweep_call(pt, seq, off)
        pt.prune_tree(4)
        ot.prune(4)
        L = len(ot.leaves_dfs())
        assert 1 < L < sw.n_leaves and pt.info().superset_verified == 1
        assert is_zero(pt.sweep(), len(LIST), L)
        n = 1500
        reads = sw.reads[-n:]
        sets = oracle_sets(ot, reads, BASE)
        offs, leaves = csr_of(sets)
        scores = expected_scores(ot, reads, offs, leaves, ProbeContains(ot, reads))
        want = sweep_ref.sweep([sorted(s) for s in sets], scores, [len(r) for r in reads], K, LIST, L)
        assert len(set(want["top"].tolist())) >= 4
        seq, off = pack_reads(reads)
        sweep_call(pt, seq, off)
        sweep_ref.same(pt.sweep(), want, "pruned")
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. the overflow retry
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", ["0", "100"])
def test_a_block_that_ran_again_is_counted_once(sw, slots):
    gt = sw.gt
    for path in (0, 1):
        knobs(gt, path, None)
        gt.set_option("PFQ_HIT_SLOTS", slots)
        try:
            fresh(gt)
            sweep_call(gt, sw.seq, sw.off)
            c = gt.last_capacity()
            assert c["attempts"] == 2 and c["hit_cap"] == int(slots) < c["hit_cursor"], (path, c)
            sweep_ref.same(gt.sweep(), sw.ref(), ("retry", path, slots))
        finally:
            gt.set_option("PFQ_HIT_SLOTS", None)
            knobs(gt, -1, None)
    gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 5. the grids
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [None, "0"])
def test_past_one_trip_of_the_thread_per_row_grid(sw, lds):
    gt = sw.gt
    n_base = len(sw.reads)
    bins = (len(LIST) + 1) * sw.n_leaves
    n = SWEEP_GRID_ROWS * 256 + n_base if lds == "0" else 3 * n_base
    trip = rows_grid_units(n, bins, lds is None)
    assert bins <= SWEEP_HIST_LDS and n > trip
    idx = tiled_ref.tile_index(n_base, n, n)
    m = tiled_ref.multiplicity(idx, n_base)
    want = sw.ref(mult=m)
    hit = np.array([bool(s) for s in sw.sets(BASE)])[idx]
    assert int(hit[trip:].sum()) > 1000 and want["n_units"] == n        # the later trips have rows to count
    seq, off = tiled_ref.pack_units(sw.seq, sw.off, idx)
    gt.set_option("PFQ_SWEEP_LDS", lds)
    try:
        fresh(gt)
        sweep_call(gt, seq, off)
        sweep_ref.same(gt.sweep(), want, ("rows grid", lds))
    finally:
        gt.set_option("PFQ_SWEEP_LDS", None)
        gt.reset_counts()


@pytest.mark.parametrize("lds", [None, "0"])
def test_more_queued_rows_than_one_trip_drains(sw, lds):
    """Base 0.0: every row has 80 entries and is queued."""
    gt = sw.gt
    thresholds = (0.0, 0.3, 0.7, 1.0)
    n_base, n = len(sw.reads), 9001
    bins = (len(thresholds) + 1) * sw.n_leaves
    assert sw.n_leaves > SWEEP_ROW_SHORT and all(len(s) == sw.n_leaves for s in sw.sets(0.0))
    assert bins <= SWEEP_HIST_LDS and n > 2 * long_grid_rows(n, bins, lds is None)
    idx = tiled_ref.tile_index(n_base, n, n)
    want = sw.ref(thresholds, mult=tiled_ref.multiplicity(idx, n_base))
    assert len(set(want["units_unique"].tolist())) >= 3
    seq, off = tiled_ref.pack_units(sw.seq, sw.off, idx)
    gt.set_option("PFQ_SWEEP_LDS", lds)
    try:
        fresh(gt, thresholds)
        sweep_call(gt, seq, off, 0.0)
        sweep_ref.same(gt.sweep(), want, ("long queue", lds))
    finally:
        gt.set_option("PFQ_SWEEP_LDS", None)
        gt.reset_counts()


# ---------------------------------------------------------------------------------------------------------------
# 6. beside the other post-stages
# ---------------------------------------------------------------------------------------------------------------
def test_beside_taxonomy_abundance_coverage_and_best_rows(sw):
    gt = sw.gt
    gt.set_taxonomy(*random_taxonomy(101, sw.n_leaves))
    full = dict(taxa=True, abundance=True, coverage=True, best=True)

    def state():
        return gt.taxon_counts(), gt.last_taxa(), gt.abundance(200, 0), gt.coverage(), gt.last_best_rows()
    try:
        for lca in (None, "best"):
            gt.reset_counts()
            p_res = call(gt, sw.seq, sw.off, BASE, lca=lca, **full)
            plain, p_state = observe(gt, lca), state()
            fresh(gt)
            res = sweep_call(gt, sw.seq, sw.off, lca=lca, **full)
            same_call(observe(gt, lca), plain, res, p_res, ("combined", lca))
            (tc, lt, ab, cv, br), (p_tc, p_lt, p_ab, p_cv, p_br) = state(), p_state
            assert all(np.array_equal(x, y) for x, y in zip(tc, p_tc)) and np.array_equal(lt, p_lt), lca
            same_abundance(ab, p_ab, lca)
            assert cv.keys() == p_cv.keys() and all(np.array_equal(cv[k], p_cv[k]) for k in cv), lca
            assert all(np.array_equal(x, y) for x, y in zip(br, p_br)), lca
            assert int(br[0][-1]) < int(res[0][-1])                     # (the best rows are shorter than the rows the sweep reads)
            sweep_ref.same(gt.sweep(), sw.ref(), ("combined: the whole rows, not the best", lca))
    finally:
        gt.reset_counts()
        gt.set_sweep([])


# ---------------------------------------------------------------------------------------------------------------
# 7. arguments and state
# ---------------------------------------------------------------------------------------------------------------
def test_documented_error_codes(sw, tmp_path):
    gt = sw.gt
    reads = sw.reads[:60]
    seq, off = pack_reads(reads)
    L, hits = _ffi.lib(), _ffi.Hits()
    full = _ffi.WANT_SWEEP | _ffi.WANT_HITS | _ffi.WANT_SCORES

    def raw(flags, thr=BASE, n=len(reads)):
        return L.pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, n, thr, flags, C.byref(hits)), L.pfq_last_error()
    gt.reset_counts()
    gt.set_sweep([])
    rc, msg = raw(full)
    assert rc == PFQ_ERR_STATE and b"PFQ_WANT_SWEEP" in msg and b"pfq_tree_set_sweep" in msg
    gt.set_sweep(LIST)
    for flags in (_ffi.WANT_SWEEP, _ffi.WANT_SWEEP | _ffi.WANT_HITS, _ffi.WANT_SWEEP | _ffi.WANT_SCORES):
        rc, msg = raw(flags)
        assert rc == PFQ_ERR_ARG and b"PFQ_WANT_SWEEP needs PFQ_WANT_HITS | PFQ_WANT_SCORES" in msg, flags
    for kw in (dict(want_hits=True), dict(want_scores=True), dict()):
        with pytest.raises(ValueError):
            gt.query_packed(seq, off, BASE, sweep=True, **kw)
    rc, msg = raw(full | _ffi.PAIRED)
    assert rc == PFQ_ERR_ARG and b"PFQ_WANT_SWEEP with PFQ_PAIRED" in msg
    for thr in (float(np.nextafter(np.float32(BASE), np.float32(1))), 0.5, 1.0, float("nan")):
        rc, msg = raw(full, thr)
        assert rc == PFQ_ERR_ARG and b"PFQ_WANT_SWEEP" in msg and b"threshold" in msg, thr
    assert is_zero(gt.sweep(), len(LIST), sw.n_leaves)                 # no refused call counted anything
    assert raw(full, BASE)[0] == 0 and gt.sweep()["n_units"] == len(reads)
    rc = L.pfq_query_frames(gt._h, seq.ctypes.data, off.ctypes.data, len(reads), 100, 50, BASE, full, C.byref(_ffi.Segments()))
    assert rc == PFQ_ERR_ARG and b"flags must be 0" in L.pfq_last_error()   # frames keep flags == 0
    # bad lists: the earlier list and its counters stay
    bad = [[0.3, 0.3], [0.5, 0.3], [0.3, float("nan")], [float("nan")], [0.01 * i for i in range(_ffi.SWEEP_MAX + 1)]]
    for lst in bad:
        with pytest.raises(PfqError) as e:
            gt.set_sweep(lst)
        assert e.value.code == PFQ_ERR_ARG and "pfq_tree_set_sweep" in str(e.value), lst
    assert gt.sweep()["n_units"] == len(reads) and np.array_equal(gt.sweep()["thresholds"], np.array(LIST, dtype=np.float32))
    gt.set_sweep([0.01 * i for i in range(_ffi.SWEEP_MAX)])            # the longest list
    assert gt.sweep()["thresholds"].size == _ffi.SWEEP_MAX
    gt.set_sweep([-1.0, 0.0, 2.5, 1e30])                               # any values, ascending
    gt.set_sweep([])
    gt.reset_counts()
    # an empty tree
    empty = BloomTree.new(K, 0.001, 3000, 1, 2)
    try:
        with pytest.raises(PfqError) as e:
            empty.set_sweep(LIST)
        assert e.value.code == PFQ_ERR_STATE
    finally:
        empty.close()
    # a subtree shard
    d = str(tmp_path / "db")
    gt.save(d)
    shard = BloomTree.load_subtree(d, 2, 1)
    try:
        with pytest.raises(PfqError) as e:
            shard.set_sweep(LIST)
        assert e.value.code == PFQ_ERR_UNSUPPORTED and "shard" in str(e.value)
    finally:
        shard.close()
    # a tree whose internal filters are aliased: not superset-verified
    genomes, ot, ids = _h4_tree(320, 32)
    d2 = str(tmp_path / "h4")
    fmt.write_db(ot, d2)
    h4 = BloomTree.load(d2)
    try:
        assert h4.info().superset_verified == 0
        with pytest.raises(PfqError) as e:
            h4.set_sweep(LIST)
        assert e.value.code == PFQ_ERR_UNSUPPORTED and "superset" in str(e.value)
        with pytest.raises(PfqError) as e:
            h4.query_packed(seq, off, BASE, want_hits=True, want_scores=True, sweep=True)
        assert e.value.code == PFQ_ERR_STATE                            # (no list could be set)
        assert h4.sweep()["thresholds"].size == 0
    finally:
        h4.close()
