"""Long-lived trees through mixed calls.  A tree carries state from one call to the next: the hints that size and steer the
next call (pairs, hits and candidates per read, the share of dirty pairs, tile passes), the block-mode choice, scratch
buffers that only grow, the stream of the previous call.  A seeded random sequence of calls on one tree — workloads, sizes,
thresholds, flags and entry points (host, device on stream 0, two non-blocking streams, total_bytes = 0, a window into a
larger device buffer) — is checked call by call against the oracle, and the leaf counters against its running total.
Stretches of counts-only calls across stream switches run without a synchronising read in between.  PFQ_SEQUENCE_SEEDS
sets the number of seeds (default 2)."""
import os

import numpy as np
import pytest

from hipbuf import DeviceBuffer, stream_create, stream_destroy, stream_synchronize
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, pack_reads
from test_gpu_capacity import close_families
from test_gpu_paired import combine, make_pairs, mate_sets
from test_gpu_parity import RNG, gpu_tree, hits_of, make_reads, oracle_hits, oracle_tree, rand_dna
from test_gpu_regimes import mutate, substituted_reads
from test_gpu_scores import expected_scores, long_reads

pytestmark = pytest.mark.gpu

K = 21
SEEDS = int(os.environ.get("PFQ_SEQUENCE_SEEDS", "2"))
THRESHOLDS = (1.0, 0.7, 0.3, 0.0)


class Model:
    """The oracle's side of a sequence: per-leaf running totals by name, and the base of the delta export."""

    def __init__(self, ot):
        self.ot = ot
        self.total = {t: 0 for t, _ in ot.leaf_counts()}
        self.base = dict(self.total)

    def names(self):
        return [t for t, _ in self.ot.leaf_counts()]

    def query(self, reads, thr, paired=None):
        """Oracle hit list (sorted (read or fragment, column)) of one call; adds its counts to the running total."""
        ot = self.ot
        names = self.names()
        if paired:
            sets = combine(mate_sets(ot, reads, thr), paired)
        else:
            for v in range(ot.n_nodes):
                ot.mapped_reads[v] = 0
            ohits, _, _ = orc.query_batch(ot, reads, thr)
            col = {v: i for i, v in enumerate(ot.leaves_dfs())}
            sets = [set() for _ in reads]
            for r, v in ohits:
                sets[r].add(col[v])
        for s in sets:
            for c in s:
                self.total[names[c]] += 1
        return sorted((r, c) for r, s in enumerate(sets) for c in s)

    def reset(self):
        self.total = {t: 0 for t in self.total}
        self.base = dict(self.total)


def workload(kind, genomes, fam, singles, n):
    if kind == "negative":
        return [rand_dna(150) for _ in range(n)]
    if kind == "single":
        return make_reads(singles, n, 0, 150, K, errors=False)[:n]
    if kind == "family":
        return make_reads(fam, n, 0, 150, K, errors=False)[:n]
    if kind == "short":
        return [rand_dna(int(RNG.integers(0, K))) for _ in range(n // 2)] + make_reads(genomes, n // 2, 0, 150, K)
    if kind == "long":
        return long_reads(genomes, 6) + make_reads(genomes, n, n // 8, 150, K)
    return make_reads(genomes, n // 2, n // 8, 150, K) + substituted_reads(genomes, n // 2)     # errors


class Runner:
    """Entry points of one tree; device buffers stay alive until the next synchronisation."""

    def __init__(self, gt):
        self.gt = gt
        self.streams = [stream_create(), stream_create()]
        self.which = 0
        self.last_stream = 0
        self.alive = []

    def close(self):
        self.sync()
        for s in self.streams:
            stream_destroy(s)

    def sync(self):
        for s in self.streams:
            stream_synchronize(s)
        self.alive = []

    def device(self, seq, off, entry):
        """(d_seq, d_off, total_bytes) of one block as `entry` hands it over."""
        total = int(off[-1])
        if entry == "window":     # offsets start at a non-zero base inside a larger buffer, one of a larger offset array
            base, lead = int(RNG.integers(1, 4096)), int(RNG.integers(1, 9))
            big = np.concatenate([np.frombuffer(rand_dna(base), dtype=np.uint8), seq, np.zeros(64, dtype=np.uint8)])
            offs = np.concatenate([np.zeros(lead, dtype=np.uint64), off + np.uint64(base), np.zeros(3, dtype=np.uint64)])
            bs, bo = DeviceBuffer.from_numpy(big), DeviceBuffer.from_numpy(offs)
            self.alive += [bs, bo]
            return bs.ptr, bo.ptr + 8 * lead, base + total      # (total_bytes = offsets[n_reads])
        bs, bo = DeviceBuffer.from_numpy(seq), DeviceBuffer.from_numpy(off)
        self.alive += [bs, bo]
        return bs.ptr, bo.ptr, 0 if entry == "bytes0" else total

    def call(self, reads, thr, entry, hits, scores, paired):
        gt = self.gt
        seq, off = pack_reads(reads)
        kw = dict(paired=paired is not None, pair_mode=paired or "either")
        self.last_stream = 0    # (pfq_query_batch runs on the default stream)
        if entry == "host":
            return gt.query_packed(seq, off, thr, want_hits=hits, want_scores=scores, **kw)
        stream = 0
        if entry == "streams":
            self.which ^= 1
            stream = self.last_stream = self.streams[self.which]
        d_seq, d_off, total = self.device(seq, off, entry)
        if hits:
            res = gt.query_device_hits(d_seq, d_off, len(reads), total, thr, stream=stream, want_scores=scores, **kw)
            return tuple(np.array(x) for x in res)
        gt.query_device(d_seq, d_off, len(reads), total, thr, stream=stream, **kw)
        return None

    def delta_round_trip(self, model):
        """export_counts_delta / import_counts_delta on the stream of the last query: delta == total - base; counters
        unchanged, the base moves to the total."""
        gt, nl = self.gt, len(model.total)
        stream = self.last_stream
        d = DeviceBuffer(8 * nl)
        gt.export_counts_delta(d.ptr, stream)
        stream_synchronize(stream)
        names = model.names()
        assert d.to_numpy(np.uint64).tolist() == [model.total[t] - model.base[t] for t in names]
        gt.import_counts_delta(d.ptr, stream)
        stream_synchronize(stream)
        model.base = dict(model.total)


def check_counts(gt, model):
    got = gt.get_leaf_counts()
    assert [t for t, _ in got] == model.names()
    assert dict(got) == model.total


def run_sequence(gt, ot, genomes, fam, singles, seed, n_calls, inserts=()):
    rng = np.random.default_rng(seed)
    model, runner = Model(ot), Runner(gt)
    pending = list(inserts)
    try:
        for i in range(n_calls):
            if pending and i == n_calls // 2:          # greedy insertions in the middle of the sequence
                runner.sync()
                check_counts(gt, model)
                for g, name in pending:
                    gt.insert(g, name)
                    orc.greedy_insert(ot, g, name)
                    model.total[name] = model.base[name] = 0
                pending = []
                check_counts(gt, model)
            op = rng.random()
            if op < 0.06:
                runner.sync()
                gt.reset_counts()
                model.reset()
                continue
            if op < 0.12:
                runner.delta_round_trip(model)
                continue
            kind = ("negative", "single", "family", "short", "long", "errors")[int(rng.integers(0, 6))]
            thr = THRESHOLDS[int(rng.integers(0, 4))]
            gt.set_path(int(rng.choice([-1, 1])))
            entry = ("host", "dev0", "streams", "streams", "bytes0", "window")[int(rng.integers(0, 6))]
            flag = ("counts", "counts", "counts", "hits", "scores", "either", "both")[int(rng.integers(0, 7))]
            n = int(rng.choice([150, 400, 1500]))
            if flag in ("either", "both"):
                pairs = make_pairs(genomes, K, n // 14)
                reads = [m for p in pairs for m in p]
            else:
                reads = workload(kind, genomes, fam, singles, n)
            if flag == "scores":
                reads = reads[:300]
            paired = flag if flag in ("either", "both") else None
            hits = flag != "counts" and (flag in ("hits", "scores") or rng.random() < 0.5)
            want = model.query(reads, thr, paired)
            res = runner.call(reads, thr, entry, hits, flag == "scores", paired)
            ctx = (seed, i, kind, thr, entry, flag, n)
            if hits:
                assert hits_of(res[0], res[1]) == want, ctx
                if flag == "scores":
                    assert np.array_equal(res[2].astype(np.int64), expected_scores(ot, reads, res[0], res[1])), ctx
                check_counts(gt, model)
            elif rng.random() < 0.25:                   # (most counts-only calls are followed by another one unsynchronised)
                check_counts(gt, model)
        runner.sync()
        check_counts(gt, model)
    finally:
        runner.close()


@pytest.fixture(scope="module")
def balanced(gpu):
    fam = close_families(3)
    singles = [rand_dna(3000) for _ in range(6)]
    genomes = fam + singles
    ot, ids = oracle_tree(genomes, K, 131071, 7)
    gt = gpu_tree(genomes, ids, K, 131071, 7)
    yield genomes, fam, singles, ot, gt
    gt.close()


@pytest.mark.parametrize("seed", range(SEEDS))
def test_balanced_family_tree_sequence(balanced, seed):
    genomes, fam, singles, ot, gt = balanced
    gt.reset_counts()
    run_sequence(gt, ot, genomes, fam, singles, 7100 + seed, 36)


@pytest.mark.parametrize("seed", range(SEEDS))
def test_greedy_tree_sequence_with_inserts(gpu, seed):
    base = rand_dna(3000)
    fam = [base] + [mutate(base, 2) for _ in range(5)]
    singles = [rand_dna(int(RNG.integers(2500, 3500))) for _ in range(4)]
    genomes = fam + singles
    ids = [f"S{seed}_{i}" for i in range(len(genomes))]
    extra = [mutate(base, 3), rand_dna(3000)]
    ot = orc.build_greedy_tree(genomes, ids, K, 0.001, 5000, 5, 10)
    gt = BloomTree.new(K, 0.001, 5000, 5, 10)
    try:
        for g, i in zip(genomes, ids):
            gt.insert(g, i)
        run_sequence(gt, ot, genomes + extra, fam + extra[:1], singles, 7300 + seed, 32,
                     inserts=[(extra[0], f"S{seed}_x0"), (extra[1], f"S{seed}_x1")])
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# fixed patterns for the hints
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1.0, 0.3])
def test_negative_family_negative_block_mode_auto(balanced, thr):
    """Negative -> family -> negative blocks on the bucketed path with block mode left to the host: the candidates per read
    of one call steer the next call's choice, the results never depend on it."""
    genomes, fam, singles, ot, gt = balanced
    gt.reset_counts()
    gt.set_path(1)
    model = Model(ot)
    modes = []
    for kind in ("negative", "family", "family", "negative", "family"):
        reads = workload(kind, genomes, fam, singles, 1500)
        want = model.query(reads, thr)
        seq, off = pack_reads(reads)
        offs, leaves = gt.query_packed(seq, off, thr, want_hits=True)
        assert hits_of(offs, leaves) == want, (thr, kind)
        check_counts(gt, model)
        modes.append(gt.last_stats().tile_mode)
    assert 2 in modes, modes            # family reads (about 8 leaves each) reach block mode
    gt.set_path(-1)


def test_small_block_after_large(balanced):
    """2^18 reads (the bucketed path on its own), then small blocks on the direct and bucketed paths, on two streams."""
    genomes, fam, singles, ot, gt = balanced
    gt.reset_counts()
    gt.set_path(-1)
    n = 1 << 18
    seq = np.empty(n * 150 + 16, dtype=np.uint8)
    seq[-16:] = 0
    fam_np = np.stack([np.frombuffer(g, dtype=np.uint8) for g in fam])
    pos = orc.synth_reads(0x5EED77, 0, n // 8, 150, fam_np, fam_np.shape[1])
    seq[:n // 8 * 150] = pos.reshape(-1)
    seq[n // 8 * 150:n * 150] = np.frombuffer(b"ACGT", dtype=np.uint8)[RNG.integers(0, 4, (n - n // 8) * 150)]
    off = np.arange(n + 1, dtype=np.uint64) * 150
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    ohits, _, _ = orc.query_batch_packed(ot, seq, off, 1.0, threads=8)
    model = Model(ot)
    model.total = dict(ot.leaf_counts())
    runner = Runner(gt)
    try:
        d_seq, d_off, total = runner.device(seq, off, "dev0")
        gt.query_device(d_seq, d_off, n, total, 1.0, stream=runner.streams[0])
        assert gt.last_stats().path == 1
        runner.which = 0
        for path in (-1, 1, -1):
            gt.set_path(path)
            for thr in (1.0, 0.3):
                reads = workload("family", genomes, fam, singles, 300)
                want = model.query(reads, thr)
                res = runner.call(reads, thr, "streams", True, False, None)
                assert hits_of(res[0], res[1]) == want, (path, thr)
        check_counts(gt, model)
        assert len(ohits) > n // 8
    finally:
        runner.close()
        gt.set_path(-1)


def test_prune_reopened_copy_mid_sequence(balanced, tmp_path):
    """Counts, save, reopen, prune the copy: the copy queries like a pruned oracle tree; the original goes on counting."""
    genomes, fam, singles, ot, gt = balanced
    gt.reset_counts()
    gt.set_path(-1)
    model = Model(ot)
    reads = workload("family", genomes, fam, singles, 400)
    model.query(reads, 1.0)
    seq, off = pack_reads(reads)
    gt.query_packed(seq, off, 1.0)
    d = str(tmp_path / "db")
    gt.save(d)
    copy = BloomTree.load(d)
    try:
        pt, _ = oracle_tree(genomes, K, 131071, 7)
        pt.prune(2)
        copy.prune_tree(2)
        copy.reset_counts()
        for thr in (1.0, 0.3):
            for v in range(pt.n_nodes):
                pt.mapped_reads[v] = 0
            ohits, _, _ = orc.query_batch(pt, reads, thr)
            copy.reset_counts()
            offs, leaves = copy.query_packed(seq, off, thr, want_hits=True)
            assert hits_of(offs, leaves) == oracle_hits(pt, ohits), thr
            assert copy.get_leaf_counts() == pt.leaf_counts(), thr
            model.query(reads, thr)
            gt.query_packed(seq, off, thr)
            check_counts(gt, model)
    finally:
        copy.close()


def test_destroyed_stream_then_another_stream(balanced):
    """A caller synchronises and destroys the stream of its last call, then calls on another stream (and reads stats):
    the tree must wait for that call without touching the destroyed stream (it once synchronised the stale handle)."""
    genomes, fam, singles, ot, gt = balanced
    gt.reset_counts()
    gt.set_path(1)
    model = Model(ot)
    try:
        for i in range(6):
            runner = Runner(gt)
            reads = workload("family", genomes, fam, singles, 400)
            model.query(reads, 1.0)
            runner.call(reads, 1.0, "streams", False, False, None)
            runner.close()                                   # synchronised, then destroyed
            reads = workload("errors", genomes, fam, singles, 300)
            want = model.query(reads, 0.7)
            seq, off = pack_reads(reads)
            offs, leaves = gt.query_packed(seq, off, 0.7, want_hits=True) if i % 2 else (None, None)
            if i % 2 == 0:
                gt.query_packed(seq, off, 0.7)
                assert gt.last_stats().n_reads == len(reads)
            else:
                assert hits_of(offs, leaves) == want, i
            check_counts(gt, model)
    finally:
        gt.set_path(-1)
