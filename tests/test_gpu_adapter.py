"""pfq_tree_set_adapters / pfq_prep_reads / pfq_prep_last_adapters on the device against tests/adapter_ref.py: cut, which, every
total, begin, len, reason, kept and the prepared CSR exactly — over read lengths and start alignments that cross every piece and
group size of the kernel, over the adapters' lengths, set sizes, O and E, for pairs, together with the other steps, over more reads
than a grid trip holds and for split blocks; then the classification of a block with read-through against query_packed of the cut
reads."""
import ctypes as C

import numpy as np
import pytest

import adapter_ref
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_abund import strain_families
from test_gpu_build import SEEDS, _dna
from test_gpu_prep import (H, K, NBITS, PFQ_ERR_ARG, PFQ_ERR_STATE, PIECES, PREP_SHORT_MAX, PREP_WAVE_MAX, SCAN_ITEMS, TOTALS, TRIP_READS,
                           counts_of, pack_quals)

pytestmark = pytest.mark.gpu

AD33 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
AD2 = b"CTGTCTCTTATACACATCT"
NONE = adapter_ref.NO_ADAPTER
LENGTHS = [0, 1, 4, 5, 6, 15, 16, 17, 63, 64, 65, 240, 241, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 9000]
ADAPTER_TOTALS = ("n_reads", "n_found", "bases_cut", "found")


def mutate(rng, a, n):
    """`a` with exactly n bases replaced by another base."""
    t = bytearray(a)
    for j in rng.choice(len(a), n, replace=False).tolist():
        t[j] = ord("ACGT"[("ACGT".index(chr(t[j])) + int(rng.integers(1, 4))) % 4])
    return bytes(t)


def plant(rng, L, p, insert=AD33):
    """A random read of L bases that carries `insert` (and a random tail behind it) from position p on."""
    return (_dna(rng, p) + insert + _dna(rng, L))[:L]


class Case:
    def __init__(self):
        rng = self.rng = np.random.default_rng(3300)
        self.genomes = strain_families(rng, 4, 3, 2000, 0.006, 4)
        self.ids = [f"A{i:02d}" for i in range(16)]
        self.gt = BloomTree.build_balanced(self.genomes, self.ids, K, NBITS, H, *SEEDS)

    def check(self, reads, quals, set1, set2=(), O=5, E=10, paired=False, want_reads=True, packed=None, **params):
        """One device call against the reference: what the adapter step and the prep report, and the CSR."""
        gt = self.gt
        want = adapter_ref.prep_block(reads, quals, set1, set2, O, E, paired=paired, **params)
        if quals is None:
            (seq, off), qual, hq = packed or pack_reads(reads), None, None
        else:
            seq, off, qual, hq = packed or pack_quals(reads, quals)
        gt.set_adapters(set1, set2, min_overlap=O, max_error_percent=E)
        got = gt.prep_reads(seq, off, qual, hq, paired=paired, want_reads=want_reads, **params)
        ad = gt.last_adapters()
        tag = (len(reads), [len(a) for a in set1], [len(a) for a in set2], O, E, paired, params)
        for k in ADAPTER_TOTALS:
            assert ad[k] == want[k], (tag, k, ad[k], want[k])
        for k in TOTALS:
            assert got[k] == want[k], (tag, k, got[k], want[k])
        if want_reads:
            for k, src, dtype in (("cut", ad, np.uint32), ("which", ad, np.uint8), ("begin", got, np.uint32), ("len", got, np.uint32),
                                  ("reason", got, np.uint32), ("kept", got, np.uint32)):
                g, w = src[k], np.array(want[k], dtype=dtype)
                assert g.dtype == dtype and g.shape == w.shape, (tag, k)
                bad = np.flatnonzero(g != w)
                assert bad.size == 0, (tag, k, bad[:8], g[bad[:8]], w[bad[:8]], [(len(reads[i]), int(off[i]) & 15) for i in bad[:8]] if k != "kept" else None)
        else:
            assert all(got[k] is None for k in ("begin", "len", "reason", "kept")) and ad["cut"] is None and ad["which"] is None, tag
        cseq, coff = gt.prep_csr()
        assert coff.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in want["kept_reads"]], dtype=np.int64)]).tolist(), tag
        assert cseq.tobytes() == b"".join(want["kept_reads"]), tag
        want["off"] = off
        return want


@pytest.fixture(scope="module")
def case(gpu):
    x = Case()
    yield x
    x.gt.set_adapters([])
    x.gt.close()


def length_block(rng, O, E):
    """Reads of every length of LENGTHS with the adapter planted where the rule has its edges, in a shuffled order; the reads
    that straddle a piece edge are made once their start alignment is known."""
    m = len(AD33)
    allowed = E * m // 100
    specs = []
    for L in LENGTHS:
        for p in sorted({0, 1, 15, 16, 17, L - m - 1, L - m, L - O, L - O + 1}):
            if 0 <= p < L:
                specs.append((L, "plant", p))
        specs += [(L, "none", 0), (L, "two", 0), (L, "bound", allowed), (L, "bound", allowed + 1), (L, "n", 1), (L, "n", allowed + 1), (L, "lower", 0)]
    for L, edge in ((400, PIECES[0]), (1300, PIECES[1]), (4500, PIECES[2]), (9000, 2 * PIECES[2])):
        specs += [(L, "edge", edge + d) for d in (-33, -1, 0, 1, 33)] * 3
    reads, at = [], 0
    for i in rng.permutation(len(specs)).tolist():
        L, kind, x = specs[i]
        p = int(rng.integers(0, max(L - m, 1)))
        if kind == "plant":
            s = plant(rng, L, x)
        elif kind == "none":
            s = _dna(rng, L)
        elif kind == "two":
            s = plant(rng, L, p, AD33 + _dna(rng, 7) + AD33)
        elif kind == "bound":
            s = plant(rng, L, p, mutate(rng, AD33, x))
        elif kind == "n":
            t = bytearray(AD33)
            for j in rng.choice(m, x, replace=False).tolist():
                t[j] = ord("N") if j % 2 else ord("n")
            s = plant(rng, L, p, bytes(t))
        elif kind == "lower":
            s = plant(rng, L, p, AD33.lower())
        else:                                                         # the adapter begins x bytes into the read's aligned span
            s = plant(rng, L, x - (at & 15))
        assert len(s) == L
        reads.append(s)
        at += L
    return reads


@pytest.mark.parametrize("O,E", [(5, 10), (13, 0)])
def test_lengths_round_every_piece_and_group(case, O, E):
    rng = np.random.default_rng(41 + O)
    reads = length_block(rng, O, E)
    want = case.check(reads, None, [AD33], O=O, E=E)
    off = want["off"].astype(np.int64)
    assert {int(o) & 15 for o in off[:-1]} == set(range(16))
    cuts = [(len(s), (int(o) & 15) + c) for s, o, c, w in zip(reads, off, want["cut"], want["which"]) if w != NONE]
    # matches in the first, second and a later piece of every build
    for lo, hi, piece in ((0, PREP_SHORT_MAX, PIECES[0]), (PREP_SHORT_MAX + 1, PREP_WAVE_MAX, PIECES[1]), (PREP_WAVE_MAX + 1, 1 << 30, PIECES[2])):
        pieces = {x // piece for L, x in cuts if lo <= L <= hi}
        assert {0, 1} <= pieces and max(pieces) >= (2 if piece != PIECES[0] else 1), (piece, pieces)
    assert len(reads) // 2 < want["n_found"] == sum(1 for w in want["which"] if w != NONE) < len(reads) - 40
    # the reads cut to nothing are kept as empty reads; with a minimum length they are dropped
    assert any(c == 0 and len(s) for s, c in zip(reads, want["cut"]))
    case.check(reads, None, [AD33], O=O, E=E, min_length=K, poly_x=10)


@pytest.fixture(scope="module")
def mixed(case):
    """Short reads for the parameter grid: every adapter of the pool planted somewhere, with 0 to 3 mismatches, some reads without."""
    rng = np.random.default_rng(77)
    pool = {m: _dna(rng, m) for m in (5, 8, 13, 33, 63, 64)}
    extra = {m: [_dna(rng, m) for _ in range(8)] for m in (5, 13, 64)}
    reads = []
    for i in range(140):
        L = int(rng.integers(0, 200)) if i % 35 else (600, 1100, 4200, 600)[i // 35]
        a = pool[int(rng.choice(list(pool)))] if i % 4 else extra[int(rng.choice(list(extra)))][int(rng.integers(8))]
        if i % 7 == 0:
            reads.append(_dna(rng, L))
        else:
            reads.append(plant(rng, L, int(rng.integers(0, L + 1)), mutate(rng, a, min(int(rng.integers(0, 4)), len(a)))))
    return pool, extra, reads, pack_reads(reads)


@pytest.mark.parametrize("O", [1, 5, 13, 64])
def test_adapter_lengths_set_sizes_overlaps_and_errors(case, mixed, O):
    pool, extra, reads, packed = mixed
    for E in (0, 10, 50):
        eligible = [a for m, a in pool.items() if m >= O]
        eight = (eligible + extra[5 if O <= 5 else 13 if O <= 13 else 64])[:8]
        assert len(eight) == 8 and all(len(a) >= O for a in eight)
        which = set()
        for n, set1 in enumerate([*([a] for a in eligible), eight]):
            want = case.check(reads, None, set1, O=O, E=E, packed=packed, want_reads=n % 3 != 2)
            which |= set(want["which"])
        assert len(which - {NONE}) >= (2 if O <= 13 else 1)


def test_pairs(case):
    rng = np.random.default_rng(12)
    reads = []
    for i in range(120):
        L = int(rng.integers(30, 160))
        ad = (AD33, AD2, None)[int(rng.integers(3))]
        reads.append(_dna(rng, L) if ad is None else plant(rng, L, int(rng.integers(0, L)), ad))
    params = dict(min_length=K)
    both = case.check(reads, None, [AD33], [AD2], paired=True, **params)
    assert sum(both["found"][:8]) > 10 and sum(both["found"][8:]) > 10 and both["n_reason"]["mate"] > 0
    assert both["found"][1:8] == [0] * 7 and both["found"][9:] == [0] * 7
    one = case.check(reads, None, [AD33, AD2], paired=True, **params)            # second mates use set 1
    assert sum(one["found"][8:]) == 0 and one["found"][0] > 10 and one["found"][1] > 10
    assert one["cut"] != both["cut"]
    unpaired = case.check(reads, None, [AD33], [AD2], paired=False, **params)    # set 2 serves nobody
    assert sum(unpaired["found"][8:]) == 0 and unpaired["n_reason"]["mate"] == 0


def test_together_with_the_other_steps(case):
    rng = np.random.default_rng(13)
    reads, quals = [], []
    for i in range(160):
        L = int(rng.integers(0, 300)) if i % 9 else int(rng.choice([700, 4300]))
        p = int(rng.integers(0, L + 1))
        s = bytearray(plant(rng, L, p) if i % 5 else _dna(rng, L))
        if i % 4 == 0 and p > 14:
            s[p - 12:p] = b"G" * 12                                   # a poly-G tail in front of the adapter
        if i % 6 == 0:
            for j in rng.integers(0, max(L, 1), 5).tolist():
                if j < L:
                    s[j] = ord("N")
        q = bytearray(rng.choice(np.frombuffer(b"#+5?IJ", dtype=np.uint8), L, p=[.05, .05, .1, .2, .3, .3]).astype(np.uint8))
        if i % 3 == 0 and p > 8:
            q[p - 6:] = b"#" * (L - p + 6)                            # the qualities fall off in front of the adapter
        reads.append(bytes(s))
        quals.append(None if i % 13 == 12 else bytes(q))
    packed = pack_quals(reads, quals)
    reasons = set()
    for par in (dict(trim_quality=20, trim_window=4), dict(trim_quality=20, trim_window=50, poly_x=10, min_length=21),
                dict(poly_x=10, max_n=3, min_complexity=30), dict(trim_quality=2, trim_window=1, min_length=50, max_n=0),
                dict(trim_quality=41, trim_window=4, poly_x=1, min_length=1, min_complexity=100)):
        reasons |= set(case.check(reads, quals, [AD33], packed=packed, **par)["reason"])
        case.check(reads, quals, [AD33, AD2], [AD2], O=8, E=20, paired=True, packed=packed, **par)
    assert reasons == {0, 1, 2, 3}


def test_more_reads_than_a_grid_trip_and_split_blocks(case):
    rng = np.random.default_rng(14)
    base = [plant(rng, L, p) for L, p in ((150, 0), (150, 40), (150, 117), (150, 140), (151, 146), (100, 60), (64, 31))]
    base += [_dna(rng, 150), _dna(rng, 33), plant(rng, 150, 90, mutate(rng, AD33, 2)), plant(rng, 150, 90, mutate(rng, AD33, 9))]
    long_reads = [plant(rng, 600, 580), plant(rng, 4200, 4150), _dna(rng, 4200)]
    idx = rng.integers(0, len(base), TRIP_READS + 2 * SCAN_ITEMS + 78).tolist()
    reads = [base[i] for i in idx]
    for j in range(30):
        reads[len(reads) - 1 - 50 * j] = long_reads[j % 3]
    assert len(reads) > TRIP_READS and len(reads) % 2 == 0
    packed = pack_reads(reads)
    params = dict(min_length=K, poly_x=10)
    whole = case.check(reads, None, [AD33], packed=packed, **params)
    assert whole["n_found"] > TRIP_READS // 2 and whole["n_kept"] > TRIP_READS // 2 and whole["n_reason"]["short"] > SCAN_ITEMS
    assert any(w != NONE and i > TRIP_READS and len(reads[i]) > PREP_WAVE_MAX for i, w in enumerate(whole["which"]))
    case.check(reads, None, [AD33], packed=packed, want_reads=False, **params)    # None arrays, the same totals
    cuts = [0, 2 * (len(reads) // 6), 2 * (len(reads) // 4) + 2, len(reads)]
    for paired in (False, True):
        full = whole if not paired else case.check(reads, None, [AD33], [AD33[:20]], paired=True, packed=packed, want_reads=False, **params)
        parts = [case.check(reads[a:b], None, [AD33], [AD33[:20]], paired=paired, **params) for a, b in zip(cuts, cuts[1:])]
        for k in ("cut", "which", "begin", "len", "reason", "kept_reads"):
            assert sum((p[k] for p in parts), []) == full[k], (paired, k)
        for k in ("n_reads", "n_found", "bases_cut", "n_kept", "bases_in", "bases_kept", "n_trimmed"):
            assert sum(p[k] for p in parts) == full[k], (paired, k)
        assert [sum(v) for v in zip(*(p["found"] for p in parts))] == full["found"]


@pytest.fixture(scope="module")
def read_through(case):
    """Reads of 150 bases from the tree's genomes whose inserts are 0 .. 220 bases: behind a short insert the adapter and a random
    tail."""
    rng, g = case.rng, case.genomes
    reads, inserts = [], []
    for a, n in zip(rng.integers(0, 1700, 400).tolist(), rng.integers(0, 221, 400).tolist()):
        reads.append((g[int(rng.integers(16))][a:a + n] + AD33 + _dna(rng, 150))[:150])
        inserts.append(n)
    return reads, inserts


@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_classification_equals_query_packed_of_the_cut_reads(case, read_through, thr):
    gt = case.gt
    reads, inserts = read_through
    params = dict(min_length=K)
    want = adapter_ref.prep_block(reads, None, [AD33], (), 5, 10, **params)
    planted = [i for i, n in enumerate(inserts) if n <= 150 - 5]
    assert sum(1 for i in planted if want["cut"][i] == inserts[i]) >= 0.95 * len(planted) and len(planted) > 200
    gt.reset_counts()
    raw_off, _ = gt.query_packed(*pack_reads(reads), thr, want_hits=True)
    gt.reset_counts()
    want_off, want_leaves, want_scores = gt.query_packed(*pack_reads(want["kept_reads"]), thr, want_hits=True, want_scores=True)
    want_counts = counts_of(gt)
    if thr == 1.0:                                                    # the feature doing its job: read-through hides a read, the cut finds it
        raw_hit = np.diff(raw_off.astype(np.int64)) > 0
        # a raw read whose insert is shorter than the read hits nothing — unless its few adapter bases happen to be the genome's
        # next bases (one base in four is), and then the read is a piece of a genome and must hit
        for i, n in enumerate(inserts):
            if n < 150:
                assert bool(raw_hit[i]) == any(reads[i] in g for g in case.genomes), (i, n)
        assert not any(raw_hit[i] for i, n in enumerate(inserts) if n <= 150 - 13)
        assert int((np.diff(want_off.astype(np.int64)) > 0).sum()) >= 0.9 * want["n_kept"] > 300
    gt.reset_counts()
    case.check(reads, None, [AD33], **params)
    assert counts_of(gt).sum() == 0                                   # preparing changes no counter
    off, leaves, scores = gt.query_prep(thr, want_hits=True, want_scores=True)
    assert off.tolist() == want_off.tolist() and leaves.tolist() == want_leaves.tolist() and scores.tolist() == want_scores.tolist()
    assert counts_of(gt).tolist() == want_counts.tolist()
    assert gt.last_stats().n_reads == want["n_kept"]
    gt.reset_counts()


def test_state_and_arguments(case):
    gt = case.gt
    fresh = BloomTree.build_balanced(case.genomes[:4], case.ids[:4], K, NBITS, H, *SEEDS)
    seq, off = pack_reads([b"ACGTACGTAC" + AD33[:9], b"ACGT"])
    with pytest.raises(PfqError) as e:
        fresh.last_adapters()                                         # no prep yet
    assert e.value.code == PFQ_ERR_STATE
    plain = fresh.prep_reads(seq, off, want_reads=True)
    for call in (fresh.last_adapters, fresh.last_adapters_ms):
        with pytest.raises(PfqError) as e:
            call()                                                    # the last prep ran without adapters
        assert e.value.code == PFQ_ERR_STATE
    nine = [AD33[i:i + 12] for i in range(9)]
    for bad, named in ((dict(set1=[AD33, None]), "adapter 1 of set 1"), (dict(set1=[b"ACGTNACGT"]), "ACGTNACGT"), (dict(set1=[b"ACGU-ACGT"]), "adapter 0 of set 1"),
                       (dict(set1=[b"ACGT"]), "ACGT"), (dict(set1=[b"A" * 65]), "adapter 0 of set 1"), (dict(set1=[AD33], set2=[AD33, b"ACG"]), "adapter 1 of set 2"),
                       (dict(set1=nine), "set 1"), (dict(set1=[AD33], set2=nine), "set 2"), (dict(set1=[AD33], min_overlap=0), "min_overlap"),
                       (dict(set1=[b"A" * 64], min_overlap=65), "min_overlap"), (dict(set1=[AD33], max_error_percent=51), "max_error_percent"),
                       (dict(set1=[], set2=[AD33]), "set 1"), (dict(set1=[AD33[:12]], min_overlap=13), "adapter 0 of set 1")):
        with pytest.raises(PfqError) as e:
            fresh.set_adapters(**bad)
        assert e.value.code == PFQ_ERR_ARG and named in str(e.value), (bad, str(e.value))
    L = _ffi.lib()
    arr = (C.c_char_p * 1)(AD33)
    assert L.pfq_tree_set_adapters(None, arr, 1, None, 0, 5, 10) == PFQ_ERR_ARG
    assert L.pfq_tree_set_adapters(fresh._h, None, 1, None, 0, 5, 10) == PFQ_ERR_ARG
    assert L.pfq_tree_set_adapters(fresh._h, arr, 1, None, 1, 5, 10) == PFQ_ERR_ARG
    assert L.pfq_prep_last_adapters(fresh._h, None) == PFQ_ERR_ARG and L.pfq_debug_last_adapters(fresh._h, None) == PFQ_ERR_ARG
    with pytest.raises(PfqError):
        fresh.last_adapters()                                         # refused calls set nothing
    # set, used, kept over a prune, dropped
    before = fresh.info().device_bytes
    fresh.set_adapters([AD33.lower().decode()], min_overlap=5, max_error_percent=10)       # str, lower case: stored in upper case
    got = fresh.prep_reads(seq, off, want_reads=True)
    ad = fresh.last_adapters()
    assert ad["cut"].tolist() == [10, 4] and ad["which"].tolist() == [0, NONE] and (ad["n_found"], ad["bases_cut"], ad["found"][0]) == (1, 9, 1)
    assert got["len"].tolist() == [10, 4] and got["n_trimmed"] == 1 and got["bases_in"] == 23 == plain["bases_in"]
    assert fresh.info().device_bytes > before                         # the new buffers are counted
    assert fresh.last_adapters_ms() >= 0.0 and len(fresh.last_prep_ms()) == 3
    fresh.prune_tree(1)
    again = fresh.prep_reads(seq, off)
    assert again["bases_kept"] == 14 and fresh.last_adapters()["cut"] is None and fresh.last_adapters()["n_found"] == 1
    fresh.set_adapters([], None)
    dropped = fresh.prep_reads(seq, off, want_reads=True)
    assert all(np.array_equal(dropped[k], plain[k]) if isinstance(plain[k], np.ndarray) else dropped[k] == plain[k] for k in plain)
    with pytest.raises(PfqError) as e:
        fresh.last_adapters()
    assert e.value.code == PFQ_ERR_STATE
    fresh.close()
    # no reads: the adapter step reports an empty block
    gt.set_adapters([AD33])
    assert gt.prep_reads(*pack_reads([]), want_reads=True)["n_reads"] == 0
    ad = gt.last_adapters()
    assert (ad["n_reads"], ad["n_found"], ad["bases_cut"], ad["cut"].size, ad["which"].size) == (0, 0, 0, 0, 0)
