"""pfq_tree_set_mate_overlap / pfq_prep_reads / pfq_prep_last_overlap on the device against tests/overlap_ref.py: insert and
mismatches per fragment, every total and the histogram, the adapter step's own results, begin, len, reason, kept and the prepared
CSR exactly — over mate lengths and start alignments round every word of the kernel's planes, inserts at every edge of the rule,
O and E, together with adapters and the trim steps, over more fragments than a grid trip holds and for split blocks; then the
classification of read-through fragments against the cut mates."""
import ctypes as C

import numpy as np
import pytest

import adapter_ref
import overlap_ref
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_abund import strain_families
from test_gpu_build import SEEDS, _dna
from test_gpu_prep import H, K, NBITS, PFQ_ERR_ARG, PFQ_ERR_STATE, SCAN_ITEMS, TOTALS, TRIP_READS, counts_of, pack_quals
from test_overlap_cpu import fragment, revcomp

pytestmark = pytest.mark.gpu

AD33 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
NO = overlap_ref.NO_INSERT
UNIT = b"ACGGTCATTG"


def other_base(rng, c):
    return ord("ACGT"[("ACGT".index(chr(c & 0xDF)) + int(rng.integers(1, 4))) % 4])


def planted(rng, I, L1, L2, n_mm=0, kind="sub", guard=False):
    """Mates of an insert of I bases with exactly n_mm mismatching pairs inside the overlap (substitutions, or N / n in either
    mate); guard: an N in each base just outside the overlap, which no hypothesis I compares."""
    a, b = (bytearray(s) for s in fragment(rng, I, L1, L2))
    lo, hi = max(0, I - L2), min(I, L1)
    if n_mm:
        for t, i in enumerate(rng.choice(np.arange(lo, hi), n_mm, replace=False).tolist()):
            if kind == "sub":
                a[i] = other_base(rng, a[i])
            elif t % 2:
                a[i] = ord("Nn"[t // 2 % 2])
            else:
                b[I - 1 - i] = ord("nN"[t // 2 % 2])
    if guard:
        for i in (lo - 1, hi):
            if 0 <= i < L1:
                a[i] = ord("N")
            if 0 <= I - 1 - i < L2:
                b[I - 1 - i] = ord("N")
    return bytes(a), bytes(b)


def lengths_of(O):
    return sorted({0, 1, O - 1, O, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151, 255, 256, 257, 511, 512, 513})


def shape_block(rng, O, E):
    """Fragments of equal and unequal mates of every length of lengths_of(O), with inserts where the rule has its edges, with
    exactly the allowed number of mismatches and one more, in a shuffled order."""
    Ls = lengths_of(O)
    frags = []
    for L1, L2 in [(L, L) for L in Ls] + [(L, Ls[(i + 5) % len(Ls)]) for i, L in enumerate(Ls)]:
        lo, hi = min(L1, L2), max(L1, L2)
        for I in sorted({O, O + 1, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, L1 + L2 - O, L1 + L2 - O + 1}):
            if I >= 0:
                frags.append(planted(rng, I, L1, L2))
        for I in (lo - 3, hi + 2):
            o = min(I, L1) - max(0, I - L2)
            if not (O <= I <= L1 + L2 - O and o >= O):
                continue
            allowed = E * o // 100
            for kind in ("sub", "n"):
                frags += [planted(rng, I, L1, L2, n, kind, guard=True) for n in (allowed, allowed + 1) if n <= o]
            a, b = planted(rng, I, L1, L2)
            frags.append((a.lower(), b[:L2 // 2] + b[L2 // 2:].lower()))
        frags.append((b"A" * L1, b"T" * L2))
        unit = (UNIT * 60)[:hi + 7]                                   # a period-10 repeat: every tenth hypothesis matches
        frags.append(((unit + _dna(rng, L1))[:L1], (revcomp(unit) + _dna(rng, L2))[:L2]))
    return [s for i in rng.permutation(len(frags)).tolist() for s in frags[i]]


class Case:
    def __init__(self):
        rng = self.rng = np.random.default_rng(3400)
        self.genomes = strain_families(rng, 4, 3, 2000, 0.006, 4)
        self.ids = [f"A{i:02d}" for i in range(16)]
        self.gt = BloomTree.build_balanced(self.genomes, self.ids, K, NBITS, H, *SEEDS)

    def check(self, reads, quals, O, E, set1=(), set2=(), adapter_O=5, adapter_E=10, want_reads=True, packed=None, **params):
        """One paired device call against the reference: what the overlap step, the adapter step and the prep report, and the CSR."""
        gt = self.gt
        want = overlap_ref.prep_block(reads, quals, O, E, set1, set2, adapter_O, adapter_E, **params)
        if quals is None:
            (seq, off), qual, hq = packed or pack_reads(reads), None, None
        else:
            seq, off, qual, hq = packed or pack_quals(reads, quals)
        gt.set_adapters(set1, set2, min_overlap=adapter_O, max_error_percent=adapter_E)
        gt.set_mate_overlap(O, E)
        got = gt.prep_reads(seq, off, qual, hq, paired=True, want_reads=want_reads, **params)
        ov = gt.last_overlap()
        tag = (len(reads), O, E, [len(a) for a in set1], params)
        for k in overlap_ref.TOTALS:
            assert ov[k] == want[k], (tag, k, ov[k], want[k])
        assert ov["hist"].dtype == np.uint64 and ov["hist"].tolist() == want["hist"], tag
        for k in TOTALS:
            assert got[k] == want[k], (tag, k, got[k], want[k])
        checks = [("insert", ov, np.uint32, want), ("mismatches", ov, np.uint32, want), ("begin", got, np.uint32, want), ("len", got, np.uint32, want),
                  ("reason", got, np.uint32, want), ("kept", got, np.uint32, want)]
        if len(set1):
            ad = gt.last_adapters()                                   # the adapter step reports what it reports without the overlap
            for k in ("n_reads", "n_found", "bases_cut", "found"):
                assert ad[k] == want["adapters"][k], (tag, k)
            checks += [("cut", ad, np.uint32, want["adapters"]), ("which", ad, np.uint8, want["adapters"])]
        else:
            with pytest.raises(PfqError):
                gt.last_adapters()
        if want_reads:
            for k, src, dtype, ref in checks:
                g, w = src[k], np.array(ref[k], dtype=dtype)
                assert g.dtype == dtype and g.shape == w.shape, (tag, k)
                bad = np.flatnonzero(g != w)
                per = 2 if k in ("insert", "mismatches") else 1
                assert bad.size == 0, (tag, k, bad[:8], g[bad[:8]], w[bad[:8]],
                                       [(len(reads[per * i]), len(reads[per * i + per - 1]), int(off[per * i]) & 15) for i in bad[:8]] if k != "kept" else None)
        else:
            assert all(got[k] is None for k in ("begin", "len", "reason", "kept")) and ov["insert"] is None and ov["mismatches"] is None, tag
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
    x.gt.set_mate_overlap(0)
    x.gt.close()


@pytest.mark.parametrize("O,E", [(30, 10), (1, 0), (12, 50), (512, 10)])
def test_lengths_inserts_and_bounds(case, O, E):
    rng = np.random.default_rng(100 + O)
    reads = shape_block(rng, O, E)
    want = case.check(reads, None, O, E)
    off = want["off"].astype(np.int64)
    assert {int(o) & 15 for o in off[:-1:2]} == set(range(16)) and {int(o) & 15 for o in off[1:-1:2]} == set(range(16))
    assert want["n_skipped"] > 20 and want["n_analysed"] > 250
    if O < 512:
        assert want["n_overlapped"] > 250 and 100 < want["n_readthrough"] < want["n_overlapped"] and want["reads_cut"] > 150
        assert E == 0 or sum(1 for m in want["mismatches"] if m > 0) > 50
        assert sum(1 for i in want["insert"] if i == NO) > 100
    else:                                                             # only whole mates of 512 bases can overlap, at I = 512
        assert {i for i in want["insert"] if i != NO} == {512} and want["n_readthrough"] == 0
    case.check(reads, None, O, E, min_length=K, poly_x=10)


def test_with_adapters_and_the_trim_steps(case):
    rng = np.random.default_rng(21)
    reads, quals = [], []
    for n in range(120):
        L1, L2 = (int(v) for v in rng.integers(40, 200, 2))
        I = int(rng.integers(20, 260))
        a, b = fragment(rng, I, L1, L2)
        if n % 3 == 0 and I < L1:
            a = (a[:I] + AD33 + _dna(rng, L1))[:L1]                   # the adapter where the overlap says it is
        if n % 4 == 0:
            a = (a[:11] + AD33 + _dna(rng, L1))[:L1]                  # an adapter in front of the insert's end: the adapter cuts more
        if n % 5 == 0:
            b = (_dna(rng, L2 - 20) + AD33)[:L2] if I > L2 else b     # an adapter where the overlap finds nothing
        if n % 7 == 0 and I > 14:
            a = a[:I - 12] + b"G" * 12 + a[I:]                        # a poly-G tail in front of the cut
        if n % 11 == 5:
            b = bytearray(b)
            for j in rng.integers(0, L2, 5).tolist():
                b[j] = ord("N")
            b = bytes(b)
        if n % 17 == 3:
            a = (b"AAAAAAAAAC" * 20)[:L1]
        qs = []
        for s in (a, b):
            q = bytearray(rng.choice(np.frombuffer(b"#+5?IJ", dtype=np.uint8), len(s), p=[.05, .05, .1, .2, .3, .3]).astype(np.uint8))
            if n % 3 == 1 and I > 8:
                q[I - 6:] = b"#" * len(q[I - 6:])                     # the qualities fall off in front of the cut
            qs.append(bytes(q))
        reads += [a, b]
        quals += [None if n % 13 == 12 else qs[0], qs[1]]
    packed = pack_quals(reads, quals)
    reasons = set()
    for par in (dict(), dict(trim_quality=20, trim_window=4), dict(trim_quality=20, trim_window=50, poly_x=10, min_length=21),
                dict(poly_x=10, max_n=3, min_complexity=30), dict(trim_quality=2, trim_window=1, min_length=50, max_n=0)):
        want = case.check(reads, quals, 30, 10, [AD33], packed=packed, **par)
        reasons |= set(want["reason"])
        ad = want["adapters"]["cut"]
        assert sum(1 for c, o in zip(ad, want["ocut"]) if c < o) > 10 and sum(1 for c, o in zip(ad, want["ocut"]) if c > o) > 10
        assert want["cut"] == [min(c, o) for c, o in zip(ad, want["ocut"])]
        case.check(reads, quals, 12, 20, [AD33], [AD33[:20]], adapter_O=8, adapter_E=20, packed=packed, **par)
        case.check(reads, quals, 30, 10, packed=packed, **par)
    assert reasons == {0, 1, 2, 3, 4}


def test_more_fragments_than_a_grid_trip_and_split_blocks(case):
    rng = np.random.default_rng(22)
    base = [planted(rng, I, L1, L2, n) for I, L1, L2, n in ((30, 150, 150, 0), (31, 150, 150, 3), (100, 150, 150, 0), (149, 150, 151, 2), (150, 150, 150, 0),
                                                             (220, 150, 150, 0), (271, 150, 150, 0), (400, 150, 150, 0), (60, 100, 64, 0), (90, 150, 150, 9),
                                                             (90, 150, 150, 10))]
    base += [(b"A" * 150, b"T" * 150), (_dna(rng, 33), b""), (_dna(rng, 120) + AD33[:30], _dna(rng, 150))]
    long_frags = [planted(rng, 100, 600, 150), planted(rng, 100, 150, 513), planted(rng, 700, 4200, 4200)]
    n_frag = (TRIP_READS + 2 * SCAN_ITEMS + 78) // 2
    frags = [base[i] for i in rng.integers(0, len(base), n_frag).tolist()]
    for j in range(30):
        frags[n_frag - 1 - 50 * j] = long_frags[j % 3]
    reads = [s for f in frags for s in f]
    assert len(reads) > TRIP_READS
    packed = pack_reads(reads)
    params = dict(min_length=K, poly_x=10)
    whole = case.check(reads, None, 30, 10, packed=packed, **params)
    assert whole["n_skipped"] == 30 and whole["n_readthrough"] > n_frag // 4 and whole["n_overlapped"] > whole["n_readthrough"] + n_frag // 8
    assert whole["n_kept"] > TRIP_READS // 2 and whole["n_reason"]["short"] > SCAN_ITEMS
    case.check(reads, None, 30, 10, packed=packed, want_reads=False, **params)         # None arrays, the same totals
    with_ad = case.check(reads, None, 30, 10, [AD33], packed=packed, want_reads=False, **params)
    cuts = [0, 2 * (len(reads) // 6), 2 * (len(reads) // 4) + 2, len(reads)]
    assert with_ad["insert"] == whole["insert"] and with_ad["hist"] == whole["hist"] and with_ad["bases_kept"] < whole["bases_kept"]
    parts = [case.check(reads[a:b], None, 30, 10, [AD33], **params) for a, b in zip(cuts, cuts[1:])]
    for k in ("insert", "mismatches", "begin", "len", "reason", "kept_reads"):
        assert sum((p[k] for p in parts), []) == with_ad[k], k
    for k in (*overlap_ref.TOTALS, "n_reads", "n_kept", "bases_in", "bases_kept", "n_trimmed"):
        assert sum(p[k] for p in parts) == with_ad[k], k
    assert [sum(v) for v in zip(*(p["hist"] for p in parts))] == with_ad["hist"]


def substitute(rng, s, rate):
    t = bytearray(s)
    for j in np.flatnonzero(rng.random(len(s)) < rate).tolist():
        t[j] = other_base(rng, t[j])
    return bytes(t)


@pytest.fixture(scope="module")
def read_through(case):
    """Fragments of 150-base mates from the tree's genomes whose inserts are 30 .. 220 bases: behind a short insert a random
    adapter of the mate's own and a random tail."""
    rng, g = case.rng, case.genomes
    reads, inserts = [], []
    for at, n in zip(rng.integers(0, 1700, 400).tolist(), rng.integers(30, 221, 400).tolist()):
        ins = g[int(rng.integers(16))][at:at + n]
        reads += [(ins + _dna(rng, 33) + _dna(rng, 150))[:150], (revcomp(ins) + _dna(rng, 33) + _dna(rng, 150))[:150]]
        inserts.append(n)
    return reads, inserts


@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_classification_equals_query_pairs_of_the_cut_mates(case, read_through, thr):
    gt = case.gt
    reads, inserts = read_through
    params = dict(min_length=K)
    want = overlap_ref.prep_block(reads, None, 30, 10, **params)
    assert want["insert"] == inserts and want["mismatches"] == [0] * len(inserts)      # error-free inserts are all recovered
    assert want["n_kept"] == len(reads) and want["n_readthrough"] == sum(1 for n in inserts if n < 150) > 150
    cut = want["kept_reads"]
    kw = dict(want_hits=True, want_scores=True, paired=True)
    gt.reset_counts()
    raw_off, _, _ = gt.query_packed(*pack_reads(reads), thr, **kw)
    gt.reset_counts()
    want_off, want_leaves, want_scores = gt.query_packed(*pack_reads(cut), thr, **kw)
    want_counts = counts_of(gt)
    gt.reset_counts()
    rows = gt.query_pairs(cut[0::2], cut[1::2], thr)
    assert [sorted(r) for r in rows] == [sorted(want_leaves[int(a):int(b)].tolist()) for a, b in zip(want_off, want_off[1:])]
    assert counts_of(gt).tolist() == want_counts.tolist()
    if thr == 1.0:                                                    # the feature doing its job: read-through hides a fragment, the cut finds it
        raw_hit = np.diff(raw_off.astype(np.int64)) > 0
        assert not any(raw_hit[f] for f, n in enumerate(inserts) if n <= 137)
        assert int((np.diff(want_off.astype(np.int64)) > 0).sum()) >= 0.9 * len(inserts)
    gt.reset_counts()
    case.check(reads, None, 30, 10, **params)
    assert counts_of(gt).sum() == 0                                   # preparing changes no counter
    off, leaves, scores = gt.query_prep(thr, **kw)
    assert off.tolist() == want_off.tolist() and leaves.tolist() == want_leaves.tolist() and scores.tolist() == want_scores.tolist()
    assert counts_of(gt).tolist() == want_counts.tolist()
    gt.reset_counts()


def test_inserts_recovered_under_substitutions(case, read_through):
    reads, inserts = read_through
    rng = np.random.default_rng(23)
    noisy = [substitute(rng, s, 0.01) for s in reads]
    want = case.check(noisy, None, 30, 10, min_length=K)
    right = sum(1 for got, n in zip(want["insert"], inserts) if got == n)
    assert all(got in (n, NO) for got, n in zip(want["insert"], inserts))         # none gets a different insert
    assert right >= 0.98 * len(inserts), right
    assert sum(want["mismatches"]) > 100


def test_state_and_arguments(case):
    gt = case.gt
    gt.set_adapters([])
    fresh = BloomTree.build_balanced(case.genomes[:4], case.ids[:4], K, NBITS, H, *SEEDS)
    ins = b"ACGTTGCAAGGCTTAGCCATGCAAGTCTGACCTGAAGT"
    mates = [ins + b"TTTTTTTTTT", revcomp(ins) + b"GGGGGGGGGG"]
    seq, off = pack_reads(mates)
    with pytest.raises(PfqError) as e:
        fresh.last_overlap()                                          # no prep yet
    assert e.value.code == PFQ_ERR_STATE
    plain = fresh.prep_reads(seq, off, paired=True, want_reads=True)
    for call in (fresh.last_overlap, fresh.last_overlap_ms):
        with pytest.raises(PfqError) as e:
            call()                                                    # the last prep ran without the overlap
        assert e.value.code == PFQ_ERR_STATE
    for bad, named in ((dict(min_overlap=513), "min_overlap"), (dict(min_overlap=1 << 31), "min_overlap"), (dict(max_error_percent=51), "max_error_percent"),
                       (dict(min_overlap=512, max_error_percent=100), "max_error_percent")):
        with pytest.raises(PfqError) as e:
            fresh.set_mate_overlap(**bad)
        assert e.value.code == PFQ_ERR_ARG and named in str(e.value), (bad, str(e.value))
    L = _ffi.lib()
    assert L.pfq_tree_set_mate_overlap(None, 30, 10) == PFQ_ERR_ARG
    assert L.pfq_prep_last_overlap(fresh._h, None) == PFQ_ERR_ARG and L.pfq_prep_last_overlap(None, C.byref(_ffi.PrepOverlap())) == PFQ_ERR_ARG
    assert L.pfq_debug_last_overlap(fresh._h, None) == PFQ_ERR_ARG and L.pfq_debug_last_overlap(None, C.byref(C.c_double())) == PFQ_ERR_ARG
    fresh.prep_reads(seq, off, paired=True)
    with pytest.raises(PfqError):
        fresh.last_overlap()                                          # refused calls set nothing
    # set, used, not used without pairs, kept over a prune, dropped
    before = fresh.info().device_bytes
    fresh.set_mate_overlap()                                          # 30, 10
    got = fresh.prep_reads(seq, off, paired=True, want_reads=True)
    ov = fresh.last_overlap()
    assert ov["insert"].tolist() == [len(ins)] and ov["mismatches"].tolist() == [0] and ov["hist"][len(ins)] == 1 and ov["hist"].sum() == 1
    assert [ov[k] for k in overlap_ref.TOTALS] == [1, 1, 0, 1, 1, 2, 20]
    assert got["len"].tolist() == [len(ins)] * 2 and got["n_trimmed"] == 2 and got["bases_in"] == plain["bases_in"] == 2 * len(ins) + 20
    assert fresh.info().device_bytes > before                         # the new buffers are counted
    assert fresh.last_overlap_ms() >= 0.0 and len(fresh.last_prep_ms()) == 3
    unpaired = fresh.prep_reads(seq, off, want_reads=True)            # no mates: the step does not run
    assert unpaired["len"].tolist() == plain["len"].tolist() == [len(s) for s in mates]
    with pytest.raises(PfqError) as e:
        fresh.last_overlap()
    assert e.value.code == PFQ_ERR_STATE
    fresh.prune_tree(1)
    again = fresh.prep_reads(seq, off, paired=True)
    ov = fresh.last_overlap()
    assert again["bases_kept"] == 2 * len(ins) and ov["insert"] is None and ov["n_overlapped"] == 1 and ov["hist"][len(ins)] == 1
    fresh.set_mate_overlap(0)
    dropped = fresh.prep_reads(seq, off, paired=True, want_reads=True)
    assert all(np.array_equal(dropped[k], plain[k]) if isinstance(plain[k], np.ndarray) else dropped[k] == plain[k] for k in plain)
    with pytest.raises(PfqError) as e:
        fresh.last_overlap()
    assert e.value.code == PFQ_ERR_STATE
    fresh.close()
    # no reads: the step reports an empty block
    gt.set_mate_overlap(30, 10)
    assert gt.prep_reads(*pack_reads([]), paired=True, want_reads=True)["n_reads"] == 0
    ov = gt.last_overlap()
    assert [ov[k] for k in overlap_ref.TOTALS] == [0] * 7 and ov["hist"].sum() == 0 and ov["insert"].size == 0 and ov["mismatches"].size == 0
