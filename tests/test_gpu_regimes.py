"""Query parity in every regime the host picks from the filter size, the hash count and the knobs.

The certificate machinery of the bucketed path is chosen from nbits and num_hashes alone: which k_tile_bin<W, CAP, MODE>
build bins the probes (from the number of filter tiles), whether LDS tiles are used at all, whether block mode is eligible,
how many L2 slices k_verify_rec / k_verify walk, and whether probe records exist (nbits < 2^30, <= 35 hashes).  Every case
here compares a query with the CPU oracle exactly as check_query does (per-leaf counts, every read's hit set,
n_hits + n_allhit * leaves), some also each hit's score, AND asserts the regime it was written for through pfq_last_stats
(path, tile_mode, n_slices, tile_bin_build), so that a moved threshold makes a case fail instead of drifting off its branch."""
import shutil

import numpy as np
import pytest

from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree
from test_gpu_parity import RNG, check_query, gpu_tree, make_reads, oracle_tree, rand_dna
from test_gpu_scores import THRESHOLDS, check_scores, long_reads

pytestmark = pytest.mark.gpu

K = 21


# ---------------------------------------------------------------------------------------------------------------
# the host's rules, restated (a change of any of them must show up here)
# ---------------------------------------------------------------------------------------------------------------
TILE_LOG2_PAIRS, TILE_LOG2_COUNTS, TILE_LOG2_BLOCK = 20, 19, 17   # pfq_kernels.h:186, :195, :205
SLICE_TARGET_BYTES = 2560 << 10                                   # pfq_host.cpp:846
# k_tile_bin builds in the order launch_tile_bin tries them (pfq_kernels.hip:2165-2190): (waves, bin capacity, shapes allowed)
BIN_BUILDS = ((16, 2048, (0,)), (16, 1024, (0,)), (16, 512, (0,)), (16, 256, (0, 2, 3)), (8, 128, (0, 1, 2, 3)))


def build_id(waves, cap):
    return waves << 16 | cap


def n_tiles(nbits, log2):
    return (((nbits + 63) // 64) * 64 + (1 << log2) - 1) >> log2


def bin_build(tiles, shape=0):
    """launch_tile_bin: the deepest bins whose LDS, (2 NT + 64 + tiles (CAP + 4)) dwords, fit 148 KiB.  shape: PFQ_BIN_NARROW
    (1: no 16-wave build deeper than 8x128, 3: 8x256 where it fits 74 KiB), PFQ_BIN_WIDE=1 (2: 16x256 at most)."""
    nt = (tiles + 63) & ~63
    lds = lambda cap: (2 * nt + 64 + tiles * (cap + 4)) * 4
    if shape == 3 and lds(256) <= 74 * 1024:
        return build_id(8, 256)
    for waves, cap, shapes in BIN_BUILDS:
        if shape in shapes and lds(cap) <= 148 * 1024:
            return build_id(waves, cap)
    return build_id(16, 60)


def expected_regime(nbits, h, thr, *, path=1, block=False, knobs=None):
    """(path, tile_mode, n_slices, tile_bin_build) of a query with set_path(path) and PFQ_BLOCK=1 if `block`; n_slices is
    None on the direct path (it reports nothing there)."""
    knobs = knobs or {}
    tile_knob = int(knobs.get("PFQ_TILE", -1))
    record_gb = int(knobs.get("PFQ_RECORD_GB", -1))
    recs = nbits < (1 << 30) and h <= 35 and record_gb != 0               # pfq_host.cpp:913 (room assumed)
    thr_one, thr_frac = thr == 1.0, 0.0 < thr < 1.0
    bucketed = path == 1 and (thr_one or thr_frac)                        # :915-916
    if bucketed and thr_frac and not recs:                                # :919
        bucketed = False
    if not bucketed:
        return (0, 0, None, 0)
    block_mode = block and recs and n_tiles(nbits, TILE_LOG2_BLOCK) <= 560 and tile_knob != 0   # :945-949
    log2 = TILE_LOG2_BLOCK if block_mode else (TILE_LOG2_PAIRS if thr_one else TILE_LOG2_COUNTS)  # :1309
    tiles = n_tiles(nbits, log2)
    tile_on = recs and (block_mode or tiles < 256) and tile_knob != 0    # :1316-1317
    slice_target = int(knobs["PFQ_SLICE_KB"]) << 10 if int(knobs.get("PFQ_SLICE_KB", 0)) > 0 else SLICE_TARGET_BYTES
    n_words, slices = (nbits + 63) // 64, 1
    while slices < 8 and (n_words * 8 + slices - 1) // slices > slice_target:   # :1215
        slices <<= 1
    narrow, wide = int(knobs.get("PFQ_BIN_NARROW", 0)), int(knobs.get("PFQ_BIN_WIDE", 0))
    shape = narrow if narrow > 0 else (2 if wide > 0 else 0)
    tile_mode = (2 if block_mode else 1) if tile_on else 0
    return (1, tile_mode, slices, bin_build(tiles, shape) if tile_on else 0)


def regime_of(st):
    return (st.path, st.tile_mode, st.n_slices if st.path else None, st.tile_bin_build)


def with_knobs(gt, knobs, fn):
    for key, val in knobs.items():
        gt.set_option(key, val)
    try:
        return fn()
    finally:
        for key in knobs:
            gt.set_option(key, None)


def check_regime(gt, ot, reads, thr, *, path=1, block=False, knobs=None, scores=False, want=None):
    """check_query in the regime expected_regime names (and `want`, where the case states it), with scores if asked.  Block
    mode is forced on or off: left to itself the host picks it from the candidates per read of earlier calls."""
    knobs = dict(knobs or {})
    knobs["PFQ_BLOCK"] = "1" if block else "0"
    exp = expected_regime(ot.nbits, ot.num_hashes, thr, path=path, block=block, knobs=knobs)
    if want is not None:
        assert exp == want, ("the host rule restated here disagrees with the case's table", exp, want)

    def run():
        st = check_query(gt, ot, reads, thr, path=path)
        got = regime_of(st)
        n_hits = st.n_hits + st.n_allhit_reads
        if scores:
            check_scores(gt, ot, reads, thr, with_oracle_hits=False)
        return got, n_hits

    got, n_hits = with_knobs(gt, knobs, run)
    assert got == exp, (ot.nbits, ot.num_hashes, thr, path, block, knobs, got, exp)
    return n_hits


# ---------------------------------------------------------------------------------------------------------------
# genomes and reads
# ---------------------------------------------------------------------------------------------------------------
def mutate(g, n):
    g = bytearray(g)
    for p in RNG.integers(0, len(g), n):
        g[int(p)] = ord("ACGT"[(b"ACGT".find(bytes([g[int(p)]])) + 1) % 4])
    return bytes(g)


def family_genomes(n_families, length=3000, singles=4):
    """Families of 8 strains (strain 1 a twin of strain 0, the others 20 substitutions away: reads pass several leaves of
    one block), then single genomes, one of them sharing a prefix with the next."""
    genomes = []
    for _ in range(n_families):
        base = rand_dna(length)
        genomes += [base, base] + [mutate(base, 20) for _ in range(6)]
    solo = [rand_dna(length) for _ in range(singles)]
    if singles >= 2:
        solo[1] = solo[0][:1000] + solo[1][1000:]
    return genomes + solo


def substituted_reads(genomes, n, length=150):
    """Reads of a genome with one substitution: some get past the dense screen, and only their certificate (every probe of
    every k-mer) rejects them at threshold 1."""
    out = []
    for i in range(n):
        g = genomes[int(RNG.integers(0, len(genomes)))]
        o = int(RNG.integers(0, len(g) - length + 1))
        r = mutate(g[o:o + length], 1)
        out.append(orc.revcomp(r) if i % 2 else r)
    return out


def regime_reads(genomes, n=3000):
    """Lengths 150 / 100 / 700 and shorter than k, N, lowercase, reverse complements, substitutions, foreign reads."""
    reads = make_reads(genomes, n // 2, n // 8, 150, K) + make_reads(genomes, n // 8, 20, 100, K)
    reads += make_reads(genomes, 8, 2, 700, K) + substituted_reads(genomes, n // 4)
    RNG.shuffle(reads)
    return reads


# ---------------------------------------------------------------------------------------------------------------
# a + b: k_tile_bin builds by geometry, and both sides of every cutoff
# ---------------------------------------------------------------------------------------------------------------
# (nbits, build at theta = 1, at theta < 1, in block mode, slices): "-" no LDS tiles, "pairs" block mode ineligible
GEOMETRIES = [
    (7_000_003, "16x2048", "16x2048", "16x512", 1),
    (12_000_007, "16x2048", "16x1024", "16x256", 1),
    (30_000_001, "16x1024", "16x512", "8x128", 2),
    (100_000_007, "16x256", "8x128", "pairs", 8),              # 763 block tiles: the pair pipeline, tile_mode 1
    (200_000_033, "8x128", "-", "pairs", 8),                   # 382 tiles at theta < 1: the record kernel counts
    (144 << 17, "16x2048", "16x1024", "16x256", 1),            # 18 / 36 / 144 tiles: the last of a build in every mode
    ((144 << 17) + 1, "16x1024", "16x512", "8x128", 1),        # 19 / 37 / 145
    (560 << 17, "16x512", "16x256", "16x60", 4),               # the largest filter of block mode
    ((560 << 17) + 1, "16x512", "16x256", "pairs", 4),
    (255 << 20, "8x128", "-", "pairs", 8),                     # the largest filter with tiles at theta = 1
    ((255 << 20) + 1, "-", "-", "pairs", 8),                   # k_verify_rec on 8 slices
]


def parse_build(s):
    if s == "-":
        return 0
    w, c = s.split("x")
    return build_id(int(w), int(c))


@pytest.mark.parametrize("nbits,b_one,b_frac,b_block,slices", GEOMETRIES)
def test_builds_and_cutoffs_match_oracle(gpu, nbits, b_one, b_frac, b_block, slices):
    """12 leaves (a family of 8 with twins, four singles with a shared prefix), 7 hashes; threshold 1 on both paths, 0.7 and
    0.3 bucketed, block mode at 1 and 0.7.  The +1 sizes leave a last tile, and a last word, with one valid bit."""
    h = 7
    genomes = family_genomes(1)
    ot, ids = oracle_tree(genomes, K, nbits, h)
    gt = gpu_tree(genomes, ids, K, nbits, h)
    reads = regime_reads(genomes)
    pair_mode = lambda b: (1, 1 if b != "-" else 0, slices, parse_build(b))
    blk_one = pair_mode(b_one) if b_block == "pairs" else (1, 2, slices, parse_build(b_block))
    blk_frac = pair_mode(b_frac) if b_block == "pairs" else (1, 2, slices, parse_build(b_block))
    try:
        assert check_regime(gt, ot, reads, 1.0, path=0, want=(0, 0, None, 0)) > 0
        assert check_regime(gt, ot, reads, 1.0, want=pair_mode(b_one)) > 0
        for thr in (0.7, 0.3):
            check_regime(gt, ot, reads, thr, want=pair_mode(b_frac))
        check_regime(gt, ot, reads, 1.0, block=True, want=blk_one)
        check_regime(gt, ot, reads, 0.7, block=True, want=blk_frac)
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# c: the limits of the 32-bit residues and of the probe records
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,n_genomes", [((1 << 30) - 1, 3), (1 << 30, 3), ((1 << 30) + 1, 2), ((1 << 32) - 5, 2)])
def test_record_and_32bit_limits(gpu, tmp_path, nbits, n_genomes):
    """2^30 - 1: records and mod_nbits30 at its largest d, no tiles, 8 slices.  2^30 and up: no records; threshold 1 is
    certified by the re-hashing k_verify, thresholds below 1 stay on the direct kernel.  Both paths, with scores.
    The device builds the tree (its filters must equal the oracle's), but the queries run on the ORACLE's filters, written to
    a database and opened: build and query share the probe walk, so a walk wrong in both would agree with itself.  (The sliced
    matrix takes 16 GB of HBM at 2^30 and 66 GB at 2^32 - 5; one tree at a time, the last case is the largest.)"""
    h = 9
    genomes = family_genomes(0, length=4000, singles=n_genomes)
    ot, ids = oracle_tree(genomes, K, nbits, h)
    gt = gpu_tree(genomes, ids, K, nbits, h)
    try:
        for v in range(ot.n_nodes):
            assert np.array_equal(gt.node_filter(v), ot.bits[ot.filter_of[v]]), v
    finally:
        gt.close()
    db = str(tmp_path / "db")
    fmt.write_db(ot, db)
    gt = BloomTree.load(db)
    reads = make_reads(genomes, 200, 40, 150, K) + substituted_reads(genomes, 60) + long_reads(genomes, 2)
    recs = nbits < (1 << 30)
    try:
        for thr in (1.0, 0.7, 0.3, 0.0):
            for path in (0, 1):
                want = expected_regime(nbits, h, thr, path=path)
                if path == 1 and thr > 0:
                    assert want[:3] == ((1, 0, 8) if thr == 1.0 or recs else (0, 0, None)), want
                n = check_regime(gt, ot, reads, thr, path=path, scores=True, want=want)
                assert n > 0, (thr, path)
    finally:
        gt.close()
        shutil.rmtree(db)


# ---------------------------------------------------------------------------------------------------------------
# d: hash counts at the ends of the records' carry word
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 2, 34, 35, 36, 48])
def test_hash_counts_match_oracle(gpu, h):
    """h = 35: the record's carry word uses all 32 bits; 36: no records (theta < 1 on the direct kernel); 1 and 2: no probe
    walk at all, the dense screen's all-ones row word.  Every threshold of test_gpu_scores, both paths, with scores."""
    nbits = 1_048_573
    genomes = family_genomes(0, length=3500, singles=5)
    genomes[4] = genomes[2]
    ot, ids = oracle_tree(genomes, K, nbits, h)
    gt = gpu_tree(genomes, ids, K, nbits, h)
    reads = make_reads(genomes, 200, 50, 150, K) + substituted_reads(genomes, 60) + long_reads(genomes, 2)
    try:
        for thr in THRESHOLDS:
            for path in (0, 1):
                want = expected_regime(nbits, h, thr, path=path)
                if h >= 36 and 0 < thr < 1:
                    assert want[0] == 0
                check_regime(gt, ot, reads, thr, path=path, scores=True, want=want)
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# e: every launch-shape and A/B knob of §9a at its extreme values
# ---------------------------------------------------------------------------------------------------------------
KNOB_NBITS, KNOB_H = 300_007, 7
KNOBS = [
    {},
    {"PFQ_BIN_NARROW": "1"},                                    # 8x128
    {"PFQ_BIN_NARROW": "3"},                                    # 8x256, two blocks per CU
    {"PFQ_BIN_WIDE": "1"},                                      # 16x256
    {"PFQ_BIN_BLOCKS": "1"},
    {"PFQ_TEST_BLOCKS": "1"},
    {"PFQ_BIN_BLOCKS": "1", "PFQ_TEST_BLOCKS": "1", "PFQ_BIN_NARROW": "1"},
    {"PFQ_TILE": "0", "PFQ_VERIFY_BLOCKS": "8"},                # (without tiles k_verify_rec sees every pair)
    {"PFQ_TILE": "0", "PFQ_VERIFY_CHUNK": "1"},
    {"PFQ_TILE": "0", "PFQ_VERIFY_CHUNK": "64"},
    {"PFQ_TILE": "0", "PFQ_VERIFY_SUB": "1"},
    {"PFQ_TILE": "0", "PFQ_VERIFY_SUB": "16"},
    {"PFQ_TILE": "0", "PFQ_VERIFY_THREADS": "64"},
    {"PFQ_TILE": "0", "PFQ_VERIFY_THREADS": "1024", "PFQ_VERIFY_CHUNK": "64", "PFQ_VERIFY_SUB": "16"},
    {"PFQ_TILE": "0", "PFQ_SLICE_KB": "20"},                    # 2 slices of a 300 k-bit filter
    {"PFQ_TILE": "0", "PFQ_SLICE_KB": "10"},                    # 4
    {"PFQ_TILE": "0", "PFQ_SLICE_KB": "1"},                     # 8
    {"PFQ_TILE": "0", "PFQ_SLICE_KB": "1", "PFQ_VERIFY_THREADS": "64", "PFQ_VERIFY_BLOCKS": "8"},
    {"PFQ_SLICE_KB": "1"},                                      # tiles, and the fallback on 8 slices
    {"PFQ_NO_TAIL_BATCH": "1"},
    {"PFQ_SCREEN_RECS": "0"},
    {"PFQ_RECORD_GB": "0", "PFQ_SLICE_KB": "1"},                # the re-hashing k_verify on 8 slices
]


@pytest.fixture(scope="module")
def knob_tree(gpu):
    """16 leaves in two families of 8 (real candidate masks in block mode), 300 k bits, 7 hashes (filters about 7 % full)."""
    genomes = family_genomes(2, singles=0)
    ot, ids = oracle_tree(genomes, K, KNOB_NBITS, KNOB_H)
    gt = gpu_tree(genomes, ids, K, KNOB_NBITS, KNOB_H)
    reads = regime_reads(genomes, 1200)
    yield genomes, ot, gt, reads
    gt.close()


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda d: ",".join(f"{k[4:]}={v}" for k, v in d.items()) or "default")
def test_knob_matrix_matches_oracle(knob_tree, knobs):
    """theta = 1 and 0.7 on the pair pipeline and in block mode, under each knob setting; the builds a knob forces are
    asserted through tile_bin_build."""
    _, ot, gt, reads = knob_tree
    for thr, block in ((1.0, False), (0.7, False), (1.0, True), (0.7, True)):
        check_regime(gt, ot, reads, thr, block=block, knobs=knobs)
    if knobs.get("PFQ_BIN_NARROW") == "1":
        assert expected_regime(KNOB_NBITS, KNOB_H, 1.0, knobs=knobs)[3] == build_id(8, 128)
    if knobs.get("PFQ_BIN_NARROW") == "3":
        assert expected_regime(KNOB_NBITS, KNOB_H, 1.0, knobs=knobs)[3] == build_id(8, 256)
    if knobs.get("PFQ_BIN_WIDE") == "1":
        assert expected_regime(KNOB_NBITS, KNOB_H, 1.0, knobs=knobs)[3] == build_id(16, 256)
    if "PFQ_SLICE_KB" in knobs:
        assert expected_regime(KNOB_NBITS, KNOB_H, 1.0, knobs=knobs)[2] == {"20": 2, "10": 4, "1": 8}[knobs["PFQ_SLICE_KB"]]


def test_coarse_min_leaves_two_level_below_2048(gpu):
    """PFQ_COARSE_MIN_LEAVES=1024 on an 1100-leaf tree: a coarse level and two groups of 1024 columns."""
    genomes = [rand_dna(int(RNG.integers(200, 400))) for _ in range(1100)]
    genomes[1050] = genomes[3]                                     # twins in different leaf groups
    genomes[7] = genomes[6][:150] + genomes[7][150:]
    ot, ids = oracle_tree(genomes, K, 60013, 4)
    gt = gpu_tree(genomes, ids, K, 60013, 4)
    reads = make_reads(genomes, 500, 150, 150, K) + substituted_reads(genomes, 100)
    try:
        flat = check_query(gt, ot, reads, 1.0, path=1)
        assert flat.coarse_cols == 0 and flat.leaf_groups == 1

        def two_level():
            for thr in (1.0, 0.7):
                for path in (0, 1):
                    st = check_query(gt, ot, reads, thr, path=path)
                    assert st.coarse_cols > 0 and st.leaf_groups == 2, (thr, path, st.coarse_cols, st.leaf_groups)
        with_knobs(gt, {"PFQ_COARSE_MIN_LEAVES": "1024"}, two_level)
    finally:
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# f: batching of the last windows (16 or 32 k-mers, or none)
# ---------------------------------------------------------------------------------------------------------------
def tail_batch(avg_len, k):
    """a.batch_tails (pfq_host.cpp:1222-1228): 32 when the reads' average last window has 17 - 32 k-mers, else 16."""
    tl = ((avg_len - k + 1) & 63) if avg_len >= k else 0
    return 32 if 16 < tl <= 32 else 16


@pytest.mark.parametrize("length,tail", [(84, 0), (85, 1), (100, 16), (101, 17), (116, 32), (117, 33)])
def test_tail_batching_matches_oracle(knob_tree, length, tail):
    """Reads of one length (average last window of `tail` k-mers) at threshold 1 on the bucketed path, with and without
    PFQ_NO_TAIL_BATCH."""
    genomes, ot, gt, _ = knob_tree
    assert (length - K + 1) & 63 == tail
    reads = [r for r in make_reads(genomes, 700, 100, length, K) + substituted_reads(genomes, 200, length) if len(r) == length]
    assert tail_batch(length, K) == (32 if tail in (17, 32) else 16)
    for knobs in ({}, {"PFQ_NO_TAIL_BATCH": "1"}):
        assert check_regime(gt, ot, reads, 1.0, knobs=knobs) > 0
