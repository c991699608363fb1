"""PFQ_WANT_SCORES / pfq_last_hit_scores: every hit (read, leaf) also gets the number of the read's k-mers the leaf's filter
contains (num_matches of query_passes, query.rs:38-49).  The expected score is computed independently, k-mer by k-mer, with
the oracle's get_kmers and bf_contains on the oracle's own tree (or on filters copied back from the device where the device
built them).  Every case also checks that the leaf counts and the hit CSR with scores equal those of the same call without."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_parity import RNG, gpu_tree, hits_of, make_reads, oracle_hits, oracle_tree, rand_dna

pytestmark = pytest.mark.gpu

THRESHOLDS = (1.0, 0.999, 0.75, 0.5, 0.3, 0.0, 1.5)
PFQ_ERR_ARG = -1


class Contains:
    """bf_contains over rows of a filter matrix, the row handed to the oracle's C library once."""

    def __init__(self, ot, rows=None):
        self.ot, self.rows, self.cache = ot, rows, {}

    def row(self, r):
        if r not in self.cache:
            a = np.ascontiguousarray(self.ot.bits[r] if self.rows is None else self.rows(r), dtype=np.uint64)
            self.cache[r] = (a, a.ctypes.data_as(C.POINTER(C.c_uint64)))
        return self.cache[r][1]

    def count(self, r, kmers):
        p, ot, f = self.row(r), self.ot, orc.lib().orc_bf_contains
        return sum(f(p, ot.nbits, ot.num_hashes, ot.seed1, ot.seed2, km, len(km)) for km in kmers)


def expected_scores(ot, reads, offs, leaves, contains=None):
    """The oracle's score of every entry of the CSR: leaf column -> the oracle tree's leaf node -> its filter row."""
    contains = contains or Contains(ot)
    col_row = [ot.filter_of[v] for v in ot.leaves_dfs()]
    out = np.zeros(len(leaves), dtype=np.int64)
    for r in range(len(offs) - 1):
        if offs[r] == offs[r + 1]:
            continue
        kmers = orc.get_kmers(reads[r], ot.kmer_size)
        for j in range(int(offs[r]), int(offs[r + 1])):
            out[j] = contains.count(col_row[int(leaves[j])], kmers)
    return out


def check_scores(gt, ot, reads, thr, contains=None, with_oracle_hits=True):
    """Hits and counts with scores == without; scores == the oracle's.  Returns the number of hits."""
    seq, off = pack_reads(reads)
    gt.reset_counts()
    offs0, leaves0 = gt.query_packed(seq, off, thr, want_hits=True)
    counts0 = gt.get_leaf_counts()
    gt.reset_counts()
    offs, leaves, scores = gt.query_packed(seq, off, thr, want_hits=True, want_scores=True)
    assert gt.get_leaf_counts() == counts0, thr
    assert np.array_equal(offs, offs0) and np.array_equal(leaves, leaves0), thr
    assert scores.dtype == np.uint32 and scores.shape == leaves.shape
    if with_oracle_hits:
        for v in range(ot.n_nodes):
            ot.mapped_reads[v] = 0
        ohits, _, _ = orc.query_batch(ot, reads, thr)
        assert hits_of(offs, leaves) == oracle_hits(ot, ohits), thr
    want = expected_scores(ot, reads, offs, leaves, contains)
    assert np.array_equal(scores.astype(np.int64), want), (thr, np.flatnonzero(scores != want)[:10])
    for r in range(len(reads)):                                   # need <= score <= n_kmers for every hit
        n = max(len(reads[r]) - ot.kmer_size + 1, 0)
        s = scores[int(offs[r]):int(offs[r + 1])]
        assert ((s >= orc.need(thr, n)) & (s <= n)).all() if len(s) else True, (thr, r)
    return len(leaves)


def long_reads(genomes, n, lo=2000, hi=5000):
    """Reads of 2 - 5 kbp (more than 256 k-mers) cut from genomes long enough, a few of them with substitutions."""
    out = []
    for i in range(n):
        g = genomes[i % len(genomes)]
        L = min(int(RNG.integers(lo, hi)), len(g))
        o = int(RNG.integers(0, len(g) - L + 1))
        r = bytearray(g[o:o + L])
        for p in RNG.integers(0, L, i % 4 * 7):
            r[int(p)] = ord("ACGT"[(b"ACGT".find(bytes([r[int(p)]])) + 1) % 4])
        out.append(bytes(r))
    return out


def reads_for(genomes, k):
    reads = make_reads(genomes, 160, 40, 150, k)                  # (empty, "A", k - 1, k, k + 1 bases; N, IUPAC, lowercase)
    reads += long_reads(genomes, 6)
    reads += [b"ACGTNRYKM" * 30, genomes[0][:200].lower(), genomes[1][:k], b"N" * (k + 5)]
    return reads


# ---------------------------------------------------------------------------------------------------------------
# geometries x thresholds
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,nbits,h,n_genomes", [(1, 50021, 6, 6), (21, 50021, 6, 8), (31, 200003, 8, 8), (64, 100003, 5, 6),
                                                  (21, 4294967291, 4, 2), (21, 400009, 200, 4)])
def test_scores_geometries_and_thresholds(gpu, k, nbits, h, n_genomes):
    """k 1 to 64; filters below 2^30 bits (probe records), of 2^32 - 5 bits (no records) and of 200 hashes (no records)."""
    genomes = [rand_dna(int(RNG.integers(5500, 7000))) for _ in range(n_genomes)]
    ot, ids = oracle_tree(genomes, k, nbits, h)
    gt = gpu_tree(genomes, ids, k, nbits, h)
    reads = reads_for(genomes, k)
    for thr in THRESHOLDS:
        check_scores(gt, ot, reads, thr)
    gt.close()


@pytest.mark.parametrize("path", [0, 1])
def test_scores_both_query_paths(gpu, path):
    genomes = [rand_dna(int(RNG.integers(5200, 6000))) for _ in range(16)]
    genomes[9] = genomes[3][:4000] + genomes[9][4000:]             # reads that hit two leaves
    ot, ids = oracle_tree(genomes, 21, 100003, 7)
    gt = gpu_tree(genomes, ids, 21, 100003, 7)
    gt.set_path(path)
    reads = reads_for(genomes, 21)
    for thr in THRESHOLDS:
        check_scores(gt, ot, reads, thr)
        assert gt.last_stats().path == (path if 0 < thr <= 1 else 0)
    gt.close()


@pytest.mark.parametrize("knob", [("PFQ_TILE", "0"), ("PFQ_RECORD_GB", "0"), ("PFQ_TILE_COUNTS", "0")])
def test_scores_certificate_fallbacks(gpu, knob):
    genomes = [rand_dna(3000) for _ in range(12)]
    ot, ids = oracle_tree(genomes, 21, 65521, 6)
    gt = gpu_tree(genomes, ids, 21, 65521, 6)
    gt.set_path(1)
    gt.set_option(*knob)
    reads = reads_for(genomes, 21)
    for thr in (1.0, 0.75, 0.3):
        check_scores(gt, ot, reads, thr)
    gt.close()


def test_scores_block_mode_families_of_8(gpu):
    """Families of 8 related genomes: reads pass several leaves of one block; block mode forced on the bucketed path."""
    genomes = []
    for _ in range(4):
        base = bytearray(rand_dna(4000))
        for s in range(8):
            g = bytearray(base)
            for p in RNG.integers(0, len(g), 0 if s == 0 else 20):
                g[int(p)] = ord("ACGT"[(b"ACGT".find(bytes([g[int(p)]])) + 1) % 4])
            genomes.append(bytes(g))
    ot, ids = oracle_tree(genomes, 21, 131071, 7)
    gt = gpu_tree(genomes, ids, 21, 131071, 7)
    gt.set_path(1)
    gt.set_option("PFQ_BLOCK", "1")
    reads = make_reads(genomes, 400, 50, 150, 21) + long_reads(genomes, 4)
    for thr in (1.0, 0.9, 0.5, 0.3):
        n_hits = check_scores(gt, ot, reads, thr)
        assert gt.last_stats().tile_mode == 2, thr
        assert n_hits > 2 * 400 * 0.5, thr                          # several strains per read
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# trees
# ---------------------------------------------------------------------------------------------------------------
def test_scores_greedy_tree(gpu):
    """A tree built by the reference's greedy insertion on the device (pfq_tree_insert); the oracle builds its own."""
    genomes = [rand_dna(int(RNG.integers(2500, 3500))) for _ in range(9)]
    genomes[4] = genomes[2][:2000] + genomes[4][2000:]
    ids = [f"G{i}" for i in range(len(genomes))]
    ot = orc.build_greedy_tree(genomes, ids, 21, 0.001, 5000, 5, 10)
    gt = BloomTree.new(21, 0.001, 5000, 5, 10)
    for g, i in zip(genomes, ids):
        gt.insert(g, i)
    assert [t for t, _ in gt.get_leaf_counts()] == [t for t, _ in ot.leaf_counts()]
    reads = reads_for(genomes, 21)
    for thr in (1.0, 0.75, 0.3, 0.0):
        check_scores(gt, ot, reads, thr)
    gt.close()


def test_scores_non_union_and_shared_filters(gpu, tmp_path):
    """Internal filters that are not unions (guard columns) and two nodes sharing one .bf, written with write_db."""
    genomes = [rand_dna(3000) for _ in range(8)]
    ot, ids = oracle_tree(genomes, 21, 50021, 6)
    internal = [v for v in range(ot.n_nodes) if not ot.is_leaf(v)]
    ot.bits[ot.filter_of[internal[1]]][::2] = 0
    a, b = internal[2], internal[3]
    ot.bf_path[b] = ot.bf_path[a]
    ot.filter_of[b] = ot.filter_of[a]
    leaves = ot.leaves_dfs()
    ot.bf_path[leaves[5]] = ot.bf_path[leaves[4]]                  # two leaves naming one filter
    ot.filter_of[leaves[5]] = ot.filter_of[leaves[4]]
    d = str(tmp_path / "db")
    fmt.write_db(ot, d)
    gt = BloomTree.load(d)
    assert gt.info().superset_verified == 0
    reads = reads_for(genomes, 21)
    for path in (0, 1):
        gt.set_path(path)
        for thr in (1.0, 0.6, 0.3, 0.0):
            check_scores(gt, ot, reads, thr)
    gt.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_scores_pruned_tree(gpu, depth):
    genomes = [rand_dna(2500) for _ in range(11)]
    ot, ids = oracle_tree(genomes, 21, 60013, 5)
    gt = gpu_tree(genomes, ids, 21, 60013, 5)
    ot.prune(depth)
    gt.prune_tree(depth)
    reads = reads_for(genomes, 21)
    for thr in (1.0, 0.5, 0.3):
        check_scores(gt, ot, reads, thr)
    gt.close()


def test_scores_subtree_shard(gpu, tmp_path):
    genomes = [rand_dna(3000) for _ in range(13)]
    genomes[7] = genomes[2]
    ot, ids = oracle_tree(genomes, 21, 50021, 7)
    d = str(tmp_path / "db")
    fmt.write_db(ot, d)
    reads = reads_for(genomes, 21)
    for index in (0, 1):
        sh_o, first = orc.subtree_shard(ot, 2, index)
        sh = BloomTree.load_subtree(d, 2, index)
        assert sh.info().shard_first_leaf == first
        for thr in (1.0, 0.5):
            check_scores(sh, sh_o, reads, thr)
        sh.close()


def test_scores_two_level_tree(gpu):
    """More than 2048 leaves: the coarse level lists reads per leaf group (k_classify<..., LIST>)."""
    genomes = [rand_dna(int(RNG.integers(150, 260))) for _ in range(2300)]
    genomes[2100] = genomes[10]
    ot, ids = oracle_tree(genomes, 20, 16381, 5)
    gt = gpu_tree(genomes, ids, 20, 16381, 5)
    reads = make_reads(genomes, 400, 100, 150, 20)
    for path in (0, 1):
        gt.set_path(path)
        for thr in (1.0, 0.9, 0.4):
            check_scores(gt, ot, reads, thr)
            assert gt.last_stats().coarse_cols > 0
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------
def test_scores_abi_errors(gpu):
    genomes = [rand_dna(1000) for _ in range(4)]
    ot, ids = oracle_tree(genomes, 21, 20011, 5)
    gt = gpu_tree(genomes, ids, 21, 20011, 5)
    L = _ffi.lib()
    seq, off = pack_reads([genomes[0][:150], genomes[1][:150]])
    hits = _ffi.Hits()
    sc, n = C.POINTER(C.c_uint32)(), C.c_uint64()
    assert L.pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, 2, 1.0, _ffi.WANT_SCORES, C.byref(hits)) == PFQ_ERR_ARG
    assert L.pfq_last_hit_scores(gt._h, C.byref(sc), C.byref(n)) == PFQ_ERR_ARG
    offs, leaves, scores = gt.query_packed(seq, off, 1.0, want_hits=True, want_scores=True)
    assert list(scores) == [130] * len(leaves) and len(leaves) >= 2
    assert L.pfq_last_hit_scores(gt._h, C.byref(sc), C.byref(n)) == 0 and n.value == len(leaves)
    gt.query_packed(seq, off, 1.0, want_hits=True)                 # a call without scores ends their validity
    with pytest.raises(PfqError) as e:
        gt.last_hit_scores()
    assert e.value.code == PFQ_ERR_ARG
    gt.query_packed(seq, off, 1.0)
    assert L.pfq_last_hit_scores(gt._h, C.byref(sc), C.byref(n)) == PFQ_ERR_ARG
    e_seq, e_off = pack_reads([])
    offs, leaves, scores = gt.query_packed(e_seq, e_off, 0.5, want_hits=True, want_scores=True)
    assert len(offs) == 1 and len(leaves) == 0 and len(scores) == 0
    gt.close()


def test_scores_device_resident_block(gpu):
    """query_device_hits(..., want_scores=True) on reads resident in HBM."""
    from hipbuf import DeviceBuffer, synchronize
    genomes = [rand_dna(3000) for _ in range(8)]
    ot, ids = oracle_tree(genomes, 21, 50021, 6)
    gt = gpu_tree(genomes, ids, 21, 50021, 6)
    reads = [r for r in make_reads(genomes, 200, 50, 150, 21, errors=False) if len(r) == 150]
    seq, off = pack_reads(reads)
    d_seq, d_off = DeviceBuffer.from_numpy(seq), DeviceBuffer.from_numpy(off)
    synchronize()
    for thr in (1.0, 0.7, 0.3):
        offs, leaves, scores = gt.query_device_hits(d_seq.ptr, d_off.ptr, len(reads), int(off[-1]), thr, 0, want_scores=True)
        offs, leaves, scores = offs.copy(), leaves.copy(), scores.copy()
        assert np.array_equal(scores.astype(np.int64), expected_scores(ot, reads, offs, leaves)), thr
        o2, l2 = gt.query_device_hits(d_seq.ptr, d_off.ptr, len(reads), int(off[-1]), thr, 0)
        assert np.array_equal(o2, offs) and np.array_equal(l2, leaves)
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# the full config-3 geometry
# ---------------------------------------------------------------------------------------------------------------
def test_scores_config3_geometry(gpu):
    """1024 leaves of 50 kbp, nbits 71 887 936, 10 hashes, k 21; 300 000 reads of 150 bp, half from the genomes with 1 %
    substitutions (bucketed pipeline chosen by the library), at 0.3 and 0.7.  Scores of the first 20 000 reads checked
    against the oracle on the device's own leaf filters, one leaf at a time."""
    from hipbuf import DeviceBuffer, synchronize
    from test_gpu_full_geometry import GLEN, H, K, N_LEAVES, N_READS, NBITS, RLEN, SEEDS, _reads
    L = _ffi.lib()
    d_gen = DeviceBuffer(N_LEAVES * GLEN)
    _ffi.check(L.pfq_synth_genomes_device(d_gen.ptr, N_LEAVES, GLEN, 0x5EED0000, None))
    synchronize()
    ids = [f"G{i:05d}" for i in range(N_LEAVES)]
    gt = BloomTree.build_balanced_device(d_gen.ptr, GLEN, N_LEAVES, ids, K, NBITS, H, SEEDS[0], SEEDS[1], 0.001, 5000000)
    genomes = d_gen.to_numpy().reshape(N_LEAVES, GLEN)
    d_gen.free()
    ot = orc.balanced_topology(ids, K, NBITS, H, SEEDS[0], SEEDS[1], 0.001, 5000000, alloc_bits=False)
    leaf_nodes = ot.leaves_dfs()
    seq, off = _reads(genomes, np.random.default_rng(20261015), N_READS, 0.01)
    n_sample = 20000
    sample = [seq[int(off[r]):int(off[r + 1])].tobytes() for r in range(n_sample)]
    for thr in (0.3, 0.7):
        gt.reset_counts()
        offs0, leaves0 = gt.query_packed(seq, off, thr, want_hits=True)
        counts0 = gt.get_leaf_counts()
        gt.reset_counts()
        offs, leaves, scores = gt.query_packed(seq, off, thr, want_hits=True, want_scores=True)
        assert gt.last_stats().path == 1
        assert gt.get_leaf_counts() == counts0 and np.array_equal(offs, offs0) and np.array_equal(leaves, leaves0), thr
        end = int(offs[n_sample])
        assert end > 0.3 * n_sample
        kmers = {}
        by_leaf = {}
        for r in range(n_sample):
            for j in range(int(offs[r]), int(offs[r + 1])):
                by_leaf.setdefault(int(leaves[j]), []).append((r, j))
        for c, pairs in by_leaf.items():                           # one leaf filter on the host at a time
            ot.bits = gt.node_filter(leaf_nodes[c])[None, :]
            cont = Contains(ot)
            for r, j in pairs:
                if r not in kmers:
                    kmers[r] = orc.get_kmers(sample[r], K)
                assert int(scores[j]) == cont.count(0, kmers[r]), (thr, r, c)
        n_k = RLEN - K + 1
        assert (scores[:end] >= orc.need(thr, n_k)).all() and (scores[:end] <= n_k).all()
    gt.close()
