"""tests/tiled_ref.py against the plain references: for a base of a few hundred units of workload W (the oracle's side only) and
a call of about 2000 units tiled from it, everything tiled_ref.Expect derives from the base's references equals what the same
references give when they are run on the expanded list of units, and the ragged packer gives pack_reads of that list.  So the
GPU tests that compare a large call with tiled_ref compare it with the references themselves.  No device is used."""
import numpy as np
import pytest

import abund_ref
import cover_ref
import tax_ref
import tiled_ref
from phagefilter_amd import pack_reads
from test_gpu_best import N_LEAVES, TAX_SEED, ProbeContains
from test_gpu_lca import K, W, best_sets, csr_of, oracle_sets, pair_scores
from test_gpu_paired import combine, mate_sets
from test_gpu_scores import expected_scores
from test_gpu_tax import random_taxonomy

N_CALL = 2003
THRESHOLDS = (0.7, 0.0)


class Base:
    """A few hundred of W's reads and fragments with the references' helpers, built once."""

    def __init__(self):
        w = W(device=False)
        self.ot, self.cm = w.ot, w.cm
        n = len(w.reads)
        self.reads = [w.reads[i] for i in list(range(0, n - 3, 13)) + [n - 3, n - 2, n - 1]]
        pairs = w.pairs()
        self.pairs = [p for i, p in enumerate(pairs) if i % 3 == 0 or max(len(p[0]), len(p[1])) < K]      # (both mates short: whole rows)
        self.preads = [m for p in self.pairs for m in p]
        self.probe = ProbeContains(w.ot, self.reads + self.preads)
        self.nodes = tax_ref.Nodes([w.ot.tax_id[v] for v in w.ot.leaves_dfs()], *random_taxonomy(TAX_SEED, N_LEAVES))
        self.cache = cover_ref.TreeSketcher(w.ot)
        self.idx = tiled_ref.tile_index(len(self.reads), N_CALL, 1)
        self.pidx = tiled_ref.tile_index(len(self.pairs), N_CALL, 2)
        self._pair_scores = {}

    def single(self, reads, thr):
        """(sets, scores, best) of single reads, by the references."""
        sets = oracle_sets(self.ot, reads, thr)
        offs, leaves = csr_of(sets)
        scores = expected_scores(self.ot, reads, offs, leaves, self.probe)
        return sets, scores, best_sets(sets, scores)

    def paired(self, preads, thr, mode):
        frag = combine(mate_sets(self.ot, preads, thr), mode)
        for v in range(self.ot.n_nodes):
            self.ot.mapped_reads[v] = 0
        key = (len(preads), thr)                                       # (at θ 0 `either` and `both` list the same rows: scored once)
        if key not in self._pair_scores or self._pair_scores[key][0] != frag:
            self._pair_scores[key] = (frag, pair_scores(self.ot, preads, frag, self.probe))
        scores = self._pair_scores[key][1]
        return frag, scores, best_sets(frag, scores)

    def sketcher(self):
        return cover_ref.TreeSketcher(self.ot, share=self.cache)


@pytest.fixture(scope="module")
def base():
    return Base()


def same_as_direct(base, exp, sets, scores, best, reads=None, pairs=None):
    """`exp`, tiled from the base, against the references run on the whole call, whose rows are sets / scores / best."""
    cm, nodes = base.cm, base.nodes
    offs, leaves = csr_of(sets)
    assert exp.offs.dtype == np.uint64 and np.array_equal(exp.offs, offs)
    assert exp.leaves.dtype == np.uint32 and np.array_equal(exp.leaves, leaves)
    assert np.array_equal(exp.scores, scores)
    counts = np.zeros(N_LEAVES, dtype=np.int64)
    for s in sets:
        for c in s:
            counts[c] += 1
    assert np.array_equal(exp.counts, counts)
    b_offs, b_leaves = csr_of(best)
    assert np.array_equal(exp.csr[0], b_offs) and np.array_equal(exp.csr[1], b_leaves) and exp.csr[1].dtype == np.uint32
    for kind, rows in (("all", sets), ("best", best)):
        want = cm.expected(rows)
        assert exp.lca[kind].dtype == np.uint32 and np.array_equal(exp.lca[kind], want)
        here, below = cm.here_below(want)
        assert np.array_equal(exp.clades[kind][0], here) and np.array_equal(exp.clades[kind][1], below)
        assert exp.clades[kind][0].dtype == np.uint64
    for got, want in zip(exp.taxa, nodes.counts(best)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    rows = [sorted(s) for s in best]
    log = abund_ref.classify(rows, N_LEAVES)
    assert exp.log == log
    assert exp.est == abund_ref.estimate(log, 200, 0)
    sk = base.sketcher()
    sk = sk.add_pairs(rows, pairs) if pairs is not None else sk.add_reads(rows, reads)
    for k in ("n_leaves", "p", "n_units", "registers", "units", "matched"):
        assert getattr(exp.sketch.sk, k) == getattr(sk.sk, k), k
    return log


def test_the_index_repeats_some_units_and_not_others(base):
    for idx, n_base in ((base.idx, len(base.reads)), (base.pidx, len(base.pairs))):
        m = tiled_ref.multiplicity(idx, n_base)
        assert len(idx) == N_CALL and 200 <= n_base <= 400
        assert int((m == 1).sum()) >= n_base // 3 and int((m > 1).sum()) >= n_base // 3 and int(m.max()) >= 10
        assert np.array_equal(idx, tiled_ref.tile_index(n_base, N_CALL, 1 if idx is base.idx else 2))      # seeded
        assert not np.array_equal(np.sort(idx), idx)
    assert {b"", b"ACGT"} <= set(base.reads) and any(0 < len(r) < K for r in base.reads)
    assert any(len(a) < K or len(b) < K for a, b in base.pairs) and (b"", b"") in base.pairs
    with pytest.raises(AssertionError):
        tiled_ref.multiplicity(np.array([0, 0, 2]), 3)                  # a base unit that never occurs


def test_ragged_packer_equals_pack_reads(base):
    seq, off = pack_reads(base.reads)
    got = tiled_ref.pack_units(seq, off, base.idx)
    want = pack_reads(tiled_ref.expand(base.reads, base.idx))
    assert got[0].dtype == want[0].dtype == np.uint8 and got[1].dtype == want[1].dtype == np.uint64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    seq, off = pack_reads(base.preads)
    got = tiled_ref.pack_units(seq, off, base.pidx, 2)
    expanded = tiled_ref.expand(base.preads, base.pidx, 2)
    assert expanded[:2] == list(base.pairs[int(base.pidx[0])]) and len(expanded) == 2 * N_CALL
    want = pack_reads(expanded)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_ragged_gather_in_chunks(base, monkeypatch):
    """The gather takes a bounded number of entries at a time: the same result whatever the bound, rows longer than it and
    empty rows at a chunk's edge included."""
    seq, off = pack_reads(base.reads)
    want = tiled_ref.pack_units(seq, off, base.idx)
    for chunk in (1, 149, 150, 151, 4096):
        monkeypatch.setattr(tiled_ref, "GATHER_CHUNK", chunk)
        got = tiled_ref.pack_units(seq, off, base.idx)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), chunk


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_single_reads(base, thr):
    sets, scores, best = base.single(base.reads, thr)
    exp = tiled_ref.Expect(base.idx, sets, scores, best, n_leaves=N_LEAVES, cm=base.cm, nodes=base.nodes, sketcher=base.sketcher(),
                           reads=base.reads)
    expanded = tiled_ref.expand(base.reads, base.idx)
    d_sets, d_scores, d_best = base.single(expanded, thr)
    log = same_as_direct(base, exp, d_sets, d_scores, d_best, reads=expanded)
    if thr > 0:                                                       # every class of the log is there, so every counter is scaled
        assert min(log[k] for k in ("n_unhit", "n_unique", "n_ambiguous", "n_all_leaves")) >= 3 and len(log["rows"]) >= 10
        assert any(s != b for s, b in zip(sets, best))
    else:
        assert all(len(s) == N_LEAVES for s in sets) and log["n_unhit"] == 0
    # the consumers over the whole rows (a call without best rows) tile the same way
    exp = tiled_ref.Expect(base.idx, sets, scores, sets, n_leaves=N_LEAVES, nodes=base.nodes, reads=base.reads,
                           sketcher=base.sketcher() if thr > 0 else None)
    for got, want in zip(exp.taxa, base.nodes.counts(d_sets)):
        assert np.array_equal(got, want)
    assert exp.log == abund_ref.classify([sorted(s) for s in d_sets], N_LEAVES)
    if thr > 0:
        sk = base.sketcher().add_reads([sorted(s) for s in d_sets], expanded)
        assert (exp.sketch.sk.registers, exp.sketch.sk.units, exp.sketch.sk.matched) == (sk.sk.registers, sk.sk.units, sk.sk.matched)


@pytest.mark.parametrize("mode", ["either", "both"])
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_fragments(base, thr, mode):
    frag, scores, best = base.paired(base.preads, thr, mode)
    exp = tiled_ref.Expect(base.pidx, frag, scores, best, n_leaves=N_LEAVES, cm=base.cm, nodes=base.nodes, sketcher=base.sketcher(),
                           pairs=base.pairs)
    expanded = tiled_ref.expand(base.preads, base.pidx, 2)
    pairs = [(expanded[2 * f], expanded[2 * f + 1]) for f in range(N_CALL)]
    log = same_as_direct(base, exp, *base.paired(expanded, thr, mode), pairs=pairs)
    assert log["n_units"] == N_CALL and log["n_all_leaves"] >= 2
    if thr > 0:
        assert log["n_ambiguous"] >= 10 and log["n_unique"] >= 10


def test_multiplicities_leave_the_plain_references_alone():
    """abund_ref and cover_ref with `mult`: m copies of a row are that row with mult m; without it nothing changed."""
    rows = [[], [3], [1, 2], [0, 1, 2, 3], [1, 2], [2]]
    m = [2, 3, 1, 4, 5, 1]
    spelled = [r for r, k in zip(rows, m) for _ in range(k)]
    assert abund_ref.classify(rows, 4, mult=m) == abund_ref.classify(spelled, 4)
    assert abund_ref.classify(rows, 4)["n_units"] == len(rows)
    a, b = cover_ref.Sketch(2, 4), cover_ref.Sketch(2, 4)
    for h in (5, 77, 5, 123456789):
        a.add_hash(1, h, 3)
        for _ in range(3):
            b.add_hash(1, h)
    assert (a.registers, a.matched) == (b.registers, b.matched) and a.matched == [0, 12]
