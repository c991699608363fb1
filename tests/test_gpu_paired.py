"""PFQ_PAIRED / PFQ_PAIR_BOTH: reads 2i and 2i + 1 are the mates of fragment i.  Each mate is judged like an unpaired read
(query.rs:38-158); the fragment's hit set is the union (`either`) or the intersection (`both`) of the mates' sets, the leaf
counters count fragments and a fragment's score on a leaf is the sum of its mates' matched k-mers on that leaf's filter.
Expected results come from the oracle's per-mate query_batch, combined here; expected scores from the oracle's get_kmers and
bf_contains, k-mer by k-mer."""
import ctypes as C

import numpy as np
import pytest

from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_parity import RNG, gpu_tree, make_reads, oracle_tree, rand_dna
from test_gpu_scores import Contains

pytestmark = pytest.mark.gpu

THRESHOLDS = (1.0, 0.7, 0.3, 0.0)
MODES = ("either", "both")
PFQ_ERR_ARG = -1


def mutate(r, n):
    r = bytearray(r)
    for p in RNG.integers(0, len(r), n):
        r[int(p)] = ord("ACGT"[(b"ACGT".find(bytes([r[int(p)]])) + 1) % 4])
    return bytes(r)


def cut(g, length=150):
    L = min(length, len(g))
    o = int(RNG.integers(0, len(g) - L + 1))
    return g[o:o + L]


def make_pairs(genomes, k, n_each=25):
    """Mate mixes: both mates from one genome (R2 reverse-complemented, as sequenced), mates from two genomes, one foreign
    mate, both foreign, a mate shorter than k (empty, one base, k - 1), N-rich, lowercase and IUPAC mates."""
    pairs = []
    for i in range(n_each):
        g = genomes[int(RNG.integers(0, len(genomes)))]
        o = int(RNG.integers(0, max(1, len(g) - 400)))
        pairs.append((g[o:o + 150], orc.revcomp(g[o + 250:o + 400])))
        g2 = genomes[int(RNG.integers(0, len(genomes)))]
        pairs.append((cut(g), cut(g2)))
        pairs.append((mutate(cut(g), i % 3), rand_dna(150)) if i % 2 else (rand_dna(150), cut(g)))
        pairs.append((rand_dna(150), rand_dna(150)))
        short = [b"", b"A", rand_dna(max(k - 1, 0))][i % 3]
        pairs.append((short, cut(g)) if i % 2 else (cut(g2), short))
        n_rich = bytearray(cut(g))
        for p in RNG.integers(0, len(n_rich), 12):
            n_rich[int(p)] = ord("N")
        pairs.append((bytes(n_rich), cut(g).lower()))
        pairs.append((b"ACGTNRYKM" * 17, cut(g2)))
    pairs += [(b"", b""), (b"A", rand_dna(max(k - 1, 0))), (genomes[0][:k], genomes[-1][:k])]
    order = RNG.permutation(len(pairs))
    return [pairs[i] for i in order]


def mate_sets(ot, reads, thr):
    """Per mate: its leaf columns, from the oracle's own query_batch (every read on its own)."""
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    ohits, _, _ = orc.query_batch(ot, reads, thr)
    col = {v: i for i, v in enumerate(ot.leaves_dfs())}
    sets = [set() for _ in reads]
    for r, v in ohits:
        sets[r].add(col[v])
    return sets


def combine(sets, mode):
    return [sets[2 * f] | sets[2 * f + 1] if mode == "either" else sets[2 * f] & sets[2 * f + 1] for f in range(len(sets) // 2)]


def check_pairs(gt, ot, pairs, thr, mode, contains=None, oracle=None):
    """Fragment lists, counters (with and without PFQ_WANT_HITS) and pair scores == the oracle's.  Returns the stats."""
    reads = [m for p in pairs for m in p]
    seq, off = pack_reads(reads)
    gt.reset_counts()
    offs, leaves, scores = gt.query_packed(seq, off, thr, want_hits=True, want_scores=True, paired=True, pair_mode=mode)
    st = gt.last_stats()
    counts = gt.get_leaf_counts()
    gt.reset_counts()
    assert gt.query_packed(seq, off, thr, paired=True, pair_mode=mode) is None
    assert gt.get_leaf_counts() == counts, (thr, mode)
    gt.reset_counts()
    o2, l2 = gt.query_packed(seq, off, thr, want_hits=True, paired=True, pair_mode=mode)
    assert np.array_equal(o2, offs) and np.array_equal(l2, leaves), (thr, mode)

    want = combine(oracle if oracle is not None else mate_sets(ot, reads, thr), mode)
    assert len(offs) == len(pairs) + 1
    for f, s in enumerate(want):
        assert leaves[int(offs[f]):int(offs[f + 1])].tolist() == sorted(s), (thr, mode, f, pairs[f])
    names = [t for t, _ in ot.leaf_counts()]
    exp_counts = [0] * len(names)
    for s in want:
        for c in s:
            exp_counts[c] += 1
    assert counts == list(zip(names, exp_counts)), (thr, mode)

    contains = contains or Contains(ot)
    col_row = [ot.filter_of[v] for v in ot.leaves_dfs()]
    kmers = [orc.get_kmers(r, ot.kmer_size) for r in reads]
    for f in range(len(pairs)):
        for j in range(int(offs[f]), int(offs[f + 1])):
            row = col_row[int(leaves[j])]
            exp = contains.count(row, kmers[2 * f]) + contains.count(row, kmers[2 * f + 1])
            assert int(scores[j]) == exp, (thr, mode, f, int(leaves[j]))
    return st


# ---------------------------------------------------------------------------------------------------------------
# thresholds x modes x paths
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [0, 1])
def test_paired_thresholds_modes_paths(gpu, path):
    genomes = [rand_dna(int(RNG.integers(4000, 5000))) for _ in range(16)]
    genomes[9] = genomes[3][:3000] + genomes[9][3000:]             # mates that hit two leaves
    ot, ids = oracle_tree(genomes, 21, 100003, 7)
    gt = gpu_tree(genomes, ids, 21, 100003, 7)
    gt.set_path(path)
    pairs = make_pairs(genomes, 21)
    reads = [m for p in pairs for m in p]
    for thr in THRESHOLDS:
        sets = mate_sets(ot, reads, thr)
        for mode in MODES:
            st = check_pairs(gt, ot, pairs, thr, mode, oracle=sets)
            assert st.path == (path if 0 < thr <= 1 else 0), (thr, mode)
    gt.close()


@pytest.mark.parametrize("k,nbits,h", [(1, 50021, 6), (31, 200003, 8), (64, 100003, 5)])
def test_paired_geometries(gpu, k, nbits, h):
    genomes = [rand_dna(int(RNG.integers(3000, 4000))) for _ in range(8)]
    ot, ids = oracle_tree(genomes, k, nbits, h)
    gt = gpu_tree(genomes, ids, k, nbits, h)
    pairs = make_pairs(genomes, k, 10)
    for thr in (1.0, 0.5):
        for mode in MODES:
            check_pairs(gt, ot, pairs, thr, mode)
    gt.close()


def test_paired_block_mode_families(gpu):
    """Families of 8 related genomes: block mode forced on the bucketed path."""
    genomes = []
    for _ in range(4):
        base = rand_dna(4000)
        genomes += [base] + [mutate(base, 20) for _ in range(7)]
    ot, ids = oracle_tree(genomes, 21, 131071, 7)
    gt = gpu_tree(genomes, ids, 21, 131071, 7)
    gt.set_path(1)
    gt.set_option("PFQ_BLOCK", "1")
    pairs = make_pairs(genomes, 21, 20)
    for thr in (1.0, 0.7, 0.3):
        for mode in MODES:
            st = check_pairs(gt, ot, pairs, thr, mode)
            assert st.tile_mode == 2, (thr, mode)
    gt.close()


def test_paired_long_mate_lists(gpu):
    """Mates passing more than 64 leaves: the fragments are merged by a wave (merge path), listed or only counted."""
    base = rand_dna(3000)
    genomes = [base] + [mutate(base, 3) for _ in range(95)] + [rand_dna(3000) for _ in range(4)]
    ot, ids = oracle_tree(genomes, 21, 65521, 5)
    gt = gpu_tree(genomes, ids, 21, 65521, 5)
    pairs = [(cut(base), orc.revcomp(cut(base))) for _ in range(30)]
    pairs += [(cut(base), cut(genomes[-1])) for _ in range(10)]    # one long list, one short
    pairs += [(cut(base), b"AC") for _ in range(5)]                # one long list, one all-hit mate
    pairs += [(rand_dna(150), cut(base)) for _ in range(5)]
    order = RNG.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    for thr in (0.9, 0.6, 0.0):
        for mode in MODES:
            check_pairs(gt, ot, pairs, thr, mode)
    seq, off = pack_reads([m for p in pairs for m in p])             # two mates of over 64 leaves each: merged by a wave
    mo, _ = gt.query_packed(seq, off, 0.6, want_hits=True)
    n_mate = np.diff(mo)
    both_long = [f for f in range(len(pairs)) if n_mate[2 * f] > 64 and n_mate[2 * f + 1] > 64]
    assert len(both_long) > 5
    for mode in MODES:
        offs, _ = gt.query_packed(seq, off, 0.6, want_hits=True, paired=True, pair_mode=mode)
        assert max(int(offs[f + 1] - offs[f]) for f in both_long) > 64, mode
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# trees
# ---------------------------------------------------------------------------------------------------------------
def test_paired_colliding_internal_names(gpu, tmp_path):
    """Internal filters that are not unions and two nodes sharing one .bf (guard columns), written with write_db."""
    genomes = [rand_dna(3000) for _ in range(8)]
    ot, ids = oracle_tree(genomes, 21, 50021, 6)
    internal = [v for v in range(ot.n_nodes) if not ot.is_leaf(v)]
    ot.bits[ot.filter_of[internal[1]]][::2] = 0
    a, b = internal[2], internal[3]
    ot.bf_path[b] = ot.bf_path[a]
    ot.filter_of[b] = ot.filter_of[a]
    d = str(tmp_path / "db")
    fmt.write_db(ot, d)
    gt = BloomTree.load(d)
    assert gt.info().superset_verified == 0
    pairs = make_pairs(genomes, 21, 15)
    for path in (0, 1):
        gt.set_path(path)
        for thr in THRESHOLDS:
            for mode in MODES:
                check_pairs(gt, ot, pairs, thr, mode)
    gt.close()


def test_paired_two_level_tree(gpu):
    """More than 2048 leaves: the two-level frontier underneath."""
    genomes = [rand_dna(int(RNG.integers(300, 420))) for _ in range(2300)]
    genomes[2100] = genomes[10]
    ot, ids = oracle_tree(genomes, 20, 16381, 5)
    gt = gpu_tree(genomes, ids, 20, 16381, 5)
    reads = make_reads(genomes, 300, 60, 150, 20)
    pairs = [(reads[2 * i], reads[2 * i + 1]) for i in range(len(reads) // 2)]
    pairs += [(cut(g), orc.revcomp(cut(g))) for g in genomes[:100]]
    mates = [m for p in pairs for m in p]
    sets = {thr: mate_sets(ot, mates, thr) for thr in (1.0, 0.4)}
    for path in (0, 1):
        gt.set_path(path)
        for thr in (1.0, 0.4):
            for mode in MODES:
                st = check_pairs(gt, ot, pairs, thr, mode, oracle=sets[thr])
                assert st.coarse_cols > 0
    gt.close()


def test_paired_subtree_shards_concatenate(gpu, tmp_path):
    """Each subtree shard combines its own leaves: the shards' fragment lists, shifted by their first leaf and concatenated
    in shard order, and their counts are the whole tree's."""
    genomes = [rand_dna(3000) for _ in range(13)]
    genomes[7] = genomes[2]
    ot, ids = oracle_tree(genomes, 21, 50021, 7)
    d = str(tmp_path / "db")
    fmt.write_db(ot, d)
    whole = BloomTree.load(d)
    pairs = make_pairs(genomes, 21, 12)
    seq, off = pack_reads([m for p in pairs for m in p])
    n_shards = BloomTree.shard_count(d, 2)
    assert n_shards > 1
    for thr in (1.0, 0.5, 0.0):
        for mode in MODES:
            whole.reset_counts()
            offs, leaves, scores = whole.query_packed(seq, off, thr, want_hits=True, want_scores=True, paired=True, pair_mode=mode)
            lists = [[] for _ in pairs]
            slists = [[] for _ in pairs]
            counts = []
            for index in range(n_shards):
                sh = BloomTree.load_subtree(d, 2, index)
                first = int(sh.info().shard_first_leaf)
                o, l, sc = sh.query_packed(seq, off, thr, want_hits=True, want_scores=True, paired=True, pair_mode=mode)
                for f in range(len(pairs)):
                    lists[f] += [first + int(x) for x in l[int(o[f]):int(o[f + 1])]]
                    slists[f] += [int(x) for x in sc[int(o[f]):int(o[f + 1])]]
                counts += sh.get_leaf_counts()
                sh.close()
            assert lists == [leaves[int(offs[f]):int(offs[f + 1])].tolist() for f in range(len(pairs))], (thr, mode)
            assert slists == [scores[int(offs[f]):int(offs[f + 1])].tolist() for f in range(len(pairs))], (thr, mode)
            assert counts == whole.get_leaf_counts(), (thr, mode)
    whole.close()


# ---------------------------------------------------------------------------------------------------------------
# counters, ABI, Python conveniences
# ---------------------------------------------------------------------------------------------------------------
def test_paired_counters_accumulate_and_unpaired_unchanged(gpu):
    genomes = [rand_dna(3000) for _ in range(8)]
    ot, ids = oracle_tree(genomes, 21, 50021, 6)
    gt = gpu_tree(genomes, ids, 21, 50021, 6)
    pairs = make_pairs(genomes, 21, 10)
    reads = [m for p in pairs for m in p]
    seq, off = pack_reads(reads)
    sets = mate_sets(ot, reads, 0.7)
    frag = combine(sets, "either")
    gt.reset_counts()
    gt.query_packed(seq, off, 0.7, paired=True)
    gt.query_packed(seq, off, 0.7, want_hits=True, paired=True)
    per_leaf = [sum(c in s for s in frag) for c in range(len(genomes))]
    assert [c for _, c in gt.get_leaf_counts()] == [2 * c for c in per_leaf]
    gt.reset_counts()                                              # unpaired calls are untouched by paired ones
    offs, leaves = gt.query_packed(seq, off, 0.7, want_hits=True)
    assert len(offs) == len(reads) + 1
    assert [set(leaves[int(offs[r]):int(offs[r + 1])].tolist()) for r in range(len(reads))] == sets
    assert [c for _, c in gt.get_leaf_counts()] == [sum(c in s for s in sets) for c in range(len(genomes))]
    gt.close()


def test_paired_abi_errors_and_conveniences(gpu):
    from hipbuf import DeviceBuffer, synchronize
    genomes = [rand_dna(2000) for _ in range(4)]
    ot, ids = oracle_tree(genomes, 21, 20011, 5)
    gt = gpu_tree(genomes, ids, 21, 20011, 5)
    L = _ffi.lib()
    seq, off = pack_reads([genomes[0][:150], genomes[1][:150], genomes[2][:150]])
    hits = _ffi.Hits()
    for flags in (_ffi.PAIRED, _ffi.PAIRED | _ffi.WANT_HITS, _ffi.PAIRED | _ffi.PAIR_BOTH | _ffi.WANT_HITS):
        assert L.pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, 3, 1.0, flags, C.byref(hits)) == PFQ_ERR_ARG
    assert L.pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, 2, 1.0, _ffi.PAIR_BOTH, C.byref(hits)) == PFQ_ERR_ARG
    with pytest.raises(ValueError):
        gt.query_packed(seq, off[:3], 1.0, paired=True, pair_mode="neither")
    with pytest.raises(PfqError) as e:
        gt.query_packed(seq, off, 1.0, want_hits=True, paired=True)
    assert e.value.code == PFQ_ERR_ARG
    e_seq, e_off = pack_reads([])
    offs, leaves, scores = gt.query_packed(e_seq, e_off, 0.5, want_hits=True, want_scores=True, paired=True)
    assert len(offs) == 1 and len(leaves) == 0 and len(scores) == 0

    r1 = [genomes[0][:150], genomes[1][:150], rand_dna(150), b""]
    r2 = [orc.revcomp(genomes[0][300:450]), genomes[2][:150], genomes[3][:150], genomes[3][500:650]]
    assert gt.query_pairs(r1, r2, 1.0) == [[0], [1, 2], [3], [0, 1, 2, 3]]
    assert gt.query_pairs(r1, r2, 1.0, "both") == [[0], [], [], [3]]
    with pytest.raises(ValueError):
        gt.query_pairs(r1, r2[:3], 1.0)

    reads = [m for p in zip(r1, r2) for m in p]
    seq, off = pack_reads(reads)
    d_seq, d_off = DeviceBuffer.from_numpy(seq), DeviceBuffer.from_numpy(off)
    synchronize()
    for mode, want in (("either", [[0], [1, 2], [3], [0, 1, 2, 3]]), ("both", [[0], [], [], [3]])):
        offs, leaves, scores = gt.query_device_hits(d_seq.ptr, d_off.ptr, len(reads), int(off[-1]), 1.0, 0, want_scores=True,
                                                    paired=True, pair_mode=mode)
        assert [leaves[int(offs[f]):int(offs[f + 1])].tolist() for f in range(4)] == want
        n = [max(len(r) - 20, 0) for r in reads]                   # theta = 1: a mate contains all of its k-mers where it hits
        assert scores[0] == n[0] + n[1]
        gt.reset_counts()
        gt.query_device(d_seq.ptr, d_off.ptr, len(reads), int(off[-1]), 1.0, 0, paired=True, pair_mode=mode)
        assert [c for _, c in gt.get_leaf_counts()] == [sum(c in w for w in want) for c in range(4)]
    gt.close()
