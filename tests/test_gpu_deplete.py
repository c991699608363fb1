"""pfq_prep_deplete on the device against tests/deplete_ref.py (the CPU oracle on what tests/prep_ref.py keeps; never the device
classifier): every total, kept, reason and the prepared CSR after the call, the screen's leaf counters, the main tree's counters
untouched; then the classification of the depleted block against query_packed of the survivors, blocks of more units than one
scan block and one grid trip, pairs in both modes, screens in sequence with the previous block's classification still queued,
the edges, the all-hit path and every refusal; then the call behind the adapter, mate-overlap and mate-correction steps of the
prep, whose results it must leave alone, and the overflow retry on a screen that has counters to lose and a call in flight."""
import ctypes as C

import numpy as np
import pytest

import correct_ref
import deplete_ref
import overlap_ref
import prep_ref
from hipbuf import DeviceBuffer, stream_create, stream_destroy, stream_synchronize
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, _ffi, pack_reads
from test_gpu_build import SEEDS, _dna, _one_child_db
from test_gpu_overlap import AD33, other_base
from test_gpu_prep import (H, K, LONG_LENGTHS, NBITS, PFQ_ERR_ARG, PFQ_ERR_STATE, PFQ_ERR_UNSUPPORTED, SCAN_ITEMS, SHORT_LENGTHS, TRIP_READS,
                           counts_of, pack_quals)

pytestmark = pytest.mark.gpu

PFQ_ERR_FORMAT = -3
KA, HA, NBITS_A, SEEDS_A = 17, 3, 100003, (0x1111222233334444, 0x9999AAAABBBBCCCC)      # screen A: its own k, hashes, size and seeds
KB, HB, NBITS_B = 19, 5, 60013                                                           # screen B: one leaf
GLEN = 10000
TRIM = dict(trim_quality=20, trim_window=4, min_length=5)
THR = 0.7


def substitute(read, at):
    return read[:at] + bytes([{65: 67, 67: 71, 71: 84, 84: 65}[read[at]]]) + read[at + 1:]


def piece(rng, g, n):
    o = int(rng.integers(0, len(g) - n + 1))
    return g[o:o + n]


def dress(rng, body):
    """(read, qualities): three worthless leading bases and eight trailing ones round a body of 29 bases or more, so that the
    trimmer has to move both ends; shorter bodies stay as they are."""
    if len(body) < 29:
        return body, b"I" * len(body)
    return _dna(rng, 3) + body + _dna(rng, 8), b"#" * 3 + b"I" * len(body) + b"#" * 8


class Case:
    def __init__(self):
        rng = self.rng = np.random.default_rng(2026)
        self.main_g = [_dna(rng, GLEN) for _ in range(16)]
        self.a_g = [_dna(rng, GLEN) for _ in range(4)]
        self.b_g = [self.main_g[5]]                                   # screen B takes reads of one main genome away
        ids = lambda p, n: [f"{p}{i:02d}" for i in range(n)]
        self.main_o = orc.build_balanced_tree(self.main_g, ids("P", 16), K, NBITS, H, *SEEDS)
        self.a_o = orc.build_balanced_tree(self.a_g, ids("A", 4), KA, NBITS_A, HA, *SEEDS_A)
        self.b_o = orc.build_balanced_tree(self.b_g, ids("B", 1), KB, NBITS_B, HB, *SEEDS)
        self.main = BloomTree.build_balanced(self.main_g, ids("P", 16), K, NBITS, H, *SEEDS)
        self.a = BloomTree.build_balanced(self.a_g, ids("A", 4), KA, NBITS_A, HA, *SEEDS_A)
        self.b = BloomTree.build_balanced(self.b_g, ids("B", 1), KB, NBITS_B, HB, *SEEDS)
        reads, quals = [], []
        for L in SHORT_LENGTHS + LONG_LENGTHS:
            n = max(L - 11, 0) if L >= 40 else L
            bodies = [piece(rng, self.a_g[int(rng.integers(4))], n), piece(rng, self.a_g[int(rng.integers(4))], n),
                      piece(rng, self.main_g[int(rng.integers(16))], n), piece(rng, self.main_g[5], n), _dna(rng, n)]
            if n:
                bodies[1] = substitute(bodies[1], n // 2)
            for body in bodies:
                s, q = dress(rng, body)
                assert len(s) == L
                reads.append(s)
                quals.append(q)
        order = rng.permutation(len(reads)).tolist()
        self.reads, self.quals = [reads[i] for i in order], [quals[i] for i in order]
        # the reference alone, before any device call
        self.prep = prep_ref.prep_block(self.reads, self.quals, **TRIM)
        assert any(self.prep["begin"]) and 0 < self.prep["n_kept"] < len(self.reads)
        self.ref = self.deplete(self.prep, self.a_o, THR)
        n = self.ref["n_units"]
        assert 4 * self.ref["units_removed"] >= n and 4 * self.ref["n_kept"] >= n, (n, self.ref["units_removed"])
        assert sum(map(bool, deplete_ref.leaf_sets(self.main_o, self.ref["survivors"], THR))) >= 10   # some survivors hit the main tree

    @staticmethod
    def deplete(prep, screen, thr, paired=False, both=False):
        return deplete_ref.deplete(prep["kept_reads"], screen, thr, paired=paired, both=both, kept=prep["kept"], reason=prep["reason"])

    def prepare(self, reads, quals, paired=False, want_reads=True, **params):
        if quals is None:
            return self.main.prep_reads(*pack_reads(reads), paired=paired, want_reads=want_reads, **params)
        return self.main.prep_reads(*pack_quals(reads, quals), paired=paired, want_reads=want_reads, **params)

    def check(self, got, want, tag, arrays=True):
        """What a prep_deplete() returned and the block it left against the reference's."""
        for k in deplete_ref.TOTALS:
            assert got[k] == want[k], (tag, k, got[k], want[k])
        if arrays:
            for k in ("kept", "reason"):
                g, w = got[k], np.array(want[k], dtype=np.uint32)
                assert g.dtype == np.uint32 and g.shape == w.shape, (tag, k, g.shape, w.shape)
                bad = np.flatnonzero(g != w)
                assert bad.size == 0, (tag, k, bad[:8], g[bad[:8]], w[bad[:8]])
        else:
            assert got["kept"] is None and got["reason"] is None, tag
        cseq, coff = self.main.prep_csr()
        assert np.array_equal(coff, np.concatenate([[0], np.cumsum([len(r) for r in want["survivors"]], dtype=np.int64)]).astype(np.uint64)), tag
        assert cseq.tobytes() == b"".join(want["survivors"]), tag


@pytest.fixture(scope="module")
def case(gpu):
    x = Case()
    yield x
    for t in (x.main, x.a, x.b):
        t.close()


def fresh(*trees):
    for t in trees:
        t.reset_counts()


def test_one_block(case):
    main, a = case.main, case.a
    fresh(main, a)
    main.query_packed(*pack_reads(case.reads[:9]), THR)              # counters that the deplete must leave alone
    before = counts_of(main)
    prep = case.prepare(case.reads, case.quals, **TRIM)
    assert prep["kept"].tolist() == case.prep["kept"]
    got = main.prep_deplete(a, THR)
    case.check(got, case.ref, "one block")
    assert counts_of(a).tolist() == case.ref["leaf_counts"] and sum(case.ref["leaf_counts"]) > 0
    assert counts_of(main).tolist() == before.tolist()
    ms = main.last_deplete_ms()
    assert len(ms) == 2 and all(v >= 0.0 for v in ms)
    # the unchanged classifier on the depleted block == query_packed of the survivors
    fresh(main)
    want_off, want_leaves = main.query_packed(*pack_reads(case.ref["survivors"]), THR, want_hits=True)
    want_counts = counts_of(main)
    assert want_counts.sum() > 0
    fresh(main)
    off, leaves = main.query_prep(THR, want_hits=True)
    assert off.tolist() == want_off.tolist() and leaves.tolist() == want_leaves.tolist()
    assert counts_of(main).tolist() == want_counts.tolist()
    assert main.last_stats().n_reads == case.ref["n_kept"]
    # the same screen again removes nothing, after a classification of the block as well
    again = main.prep_deplete(a, THR)
    want = dict(case.ref, n_units=case.ref["n_kept"], units_removed=0, reads_removed=0, bases_removed=0)
    case.check(again, want, "again")
    assert counts_of(a).tolist() == case.ref["leaf_counts"]           # the survivors add nothing to the screen
    # a block prepared without want_reads: the totals alone
    fresh(a)
    case.prepare(case.reads, case.quals, want_reads=False, **TRIM)
    case.check(main.prep_deplete(a, THR), case.ref, "totals only", arrays=False)
    assert counts_of(a).tolist() == case.ref["leaf_counts"]
    fresh(main, a)


def test_large_block(case):
    """More units than one scan block and more reads than one grid trip, of 30 bases: 512 distinct reads tiled, so the
    reference asks the oracle once per distinct read."""
    rng = np.random.default_rng(31)
    base = [piece(rng, case.a_g[i % 4], 30) if i % 3 == 0 else piece(rng, case.main_g[i % 16], 30) if i % 3 == 1 else _dna(rng, 30) for i in range(512)]
    idx = rng.integers(0, 512, TRIP_READS + 2 * SCAN_ITEMS + 77).tolist()
    reads = [base[i] for i in idx]
    prep = prep_ref.prep_block(reads, None, min_length=5)
    want = case.deplete(prep, case.a_o, 1.0)
    assert want["n_units"] > TRIP_READS and want["units_removed"] > SCAN_ITEMS and want["n_kept"] > SCAN_ITEMS
    fresh(case.a)
    case.prepare(reads, None, min_length=5)
    case.check(case.main.prep_deplete(case.a, 1.0), want, "large")
    assert counts_of(case.a).tolist() == want["leaf_counts"]
    fresh(case.a)


def fragments(case):
    rng = np.random.default_rng(8)
    a, m = case.a_g, case.main_g
    under_k = piece(rng, a[0], KA - 1)                                # passes every leaf of the screen; min_length keeps it
    frags = [(piece(rng, a[0], 150), piece(rng, a[0], 120)), (piece(rng, a[1], 150), piece(rng, m[2], 150)), (piece(rng, m[3], 90), piece(rng, a[2], 300)),
             (piece(rng, m[4], 150), _dna(rng, 150)), (under_k, piece(rng, a[3], 100)), (under_k, _dna(rng, 100)), (_dna(rng, 100), _dna(rng, 8)),
             (under_k, _dna(rng, 9)), (piece(rng, a[0], 150), piece(rng, a[1], 150)), (_dna(rng, 3), piece(rng, a[1], 150)),
             (substitute(piece(rng, a[2], 200), 100), _dna(rng, 200)), (piece(rng, m[5], 600), piece(rng, m[5], 4200))]
    frags = [frags[i] for i in rng.integers(0, len(frags), 300).tolist()] + frags
    return [s for f in frags for s in f]


@pytest.mark.parametrize("mode", ["either", "both"])
@pytest.mark.parametrize("thr", [1.0, THR])
def test_pairs(case, mode, thr):
    reads = fragments(case)
    prep = prep_ref.prep_block(reads, None, paired=True, min_length=5)
    assert prep["n_reason"]["mate"] > 0
    want = case.deplete(prep, case.a_o, thr, paired=True, both=mode == "both")
    assert 0 < want["units_removed"] < want["n_units"] and want["reads_removed"] == 2 * want["units_removed"]
    if thr == 1.0:                                                    # the fragment with a mate under the screen's k: the other mate decides with "both"
        either = case.deplete(prep, case.a_o, thr, paired=True)
        assert (want["units_removed"] < either["units_removed"]) == (mode == "both")
    fresh(case.a, case.main)
    case.prepare(reads, None, paired=True, min_length=5)
    case.check(case.main.prep_deplete(case.a, thr, paired=True, pair_mode=mode), want, (mode, thr))
    assert counts_of(case.a).tolist() == want["leaf_counts"]
    want_off, want_leaves = case.main.query_packed(*pack_reads(want["survivors"]), thr, want_hits=True, paired=True)
    want_counts = counts_of(case.main)
    fresh(case.main)
    off, leaves = case.main.query_prep(thr, want_hits=True, paired=True)
    assert off.tolist() == want_off.tolist() and leaves.tolist() == want_leaves.tolist() and len(off) == want["n_kept"] // 2 + 1
    assert counts_of(case.main).tolist() == want_counts.tolist()
    fresh(case.a, case.main)


def oracle_counts(tree, reads, thr):
    out = [0] * len(tree.leaves_dfs())
    for row in deplete_ref.leaf_sets(tree, reads, thr):
        for c in row:
            out[c] += 1
    return out


def test_sequences_of_calls(case):
    """A, then B, then two classifications; and four blocks, each prepared and depleted while the counts-only classification of
    the one before is still queued, so that both CSR sets are used twice."""
    main, a, b = case.main, case.a, case.b
    fresh(main, a, b)
    n = len(case.reads)
    cuts = [0, n // 5, n // 2, 3 * n // 4, n]
    want_main, want_a, want_b = np.zeros(16, np.int64), np.zeros(4, np.int64), np.zeros(1, np.int64)
    removed_by_b = 0
    for lo, hi in zip(cuts, cuts[1:]):
        reads, quals = case.reads[lo:hi], case.quals[lo:hi]
        prep = prep_ref.prep_block(reads, quals, **TRIM)
        ra = case.deplete(prep, case.a_o, THR)
        rb = deplete_ref.deplete(ra["survivors"], case.b_o, THR, kept=ra["kept"], reason=ra["reason"])
        removed_by_b += rb["units_removed"]
        case.prepare(reads, quals, **TRIM)
        case.check(main.prep_deplete(a, THR), ra, ("A", lo))
        case.check(main.prep_deplete(b, THR), rb, ("B", lo))
        main.query_prep(THR)                                          # counts only: returns once queued
        main.query_prep(THR)
        want_a += np.array(ra["leaf_counts"])
        want_b += np.array(rb["leaf_counts"])
        want_main += 2 * np.array(oracle_counts(case.main_o, rb["survivors"], THR))
    assert removed_by_b > 0 and want_main.sum() > 0
    assert counts_of(main).tolist() == want_main.tolist()
    assert counts_of(a).tolist() == want_a.tolist() and counts_of(b).tolist() == want_b.tolist()
    fresh(main, a, b)


def test_edges(case):
    main, a = case.main, case.a
    rng = np.random.default_rng(3)
    fresh(main, a)
    gone = [piece(rng, case.a_g[i % 4], 40 + i) for i in range(300)]
    want = deplete_ref.deplete(gone, case.a_o, 1.0)
    assert want["n_kept"] == 0 and want["units_removed"] == 300
    case.prepare(gone, None)
    case.check(main.prep_deplete(a, 1.0), want, "everything removed")
    off, leaves = main.query_prep(1.0, want_hits=True)
    assert off.tolist() == [0] and leaves.size == 0 and counts_of(main).sum() == 0
    zero = dict(want, n_units=0, units_removed=0, reads_removed=0, bases_removed=0)
    case.check(main.prep_deplete(a, 1.0), zero, "nothing is left to ask")              # n_kept == 0: a no-op that returns zeros
    assert counts_of(a).tolist() == want["leaf_counts"]
    fresh(a)
    stay = [_dna(rng, 40 + i) for i in range(300)]
    want = deplete_ref.deplete(stay, case.a_o, 1.0)
    assert want["units_removed"] == 0
    case.prepare(stay, None)
    case.check(main.prep_deplete(a, 1.0), want, "nothing removed")
    assert counts_of(a).sum() == 0
    for reads in ([b"ACGT", b"AC", b""], []):                         # all dropped by the prep; an empty block
        prep = prep_ref.prep_block(reads, None, min_length=5)
        want = case.deplete(prep, case.a_o, 1.0)
        assert want["n_units"] == 0
        case.prepare(reads, None, min_length=5)
        got = main.prep_deplete(a, 1.0)
        case.check(got, want, reads)
        assert got["reason"].tolist() == [1] * len(reads)
    assert counts_of(a).sum() == 0 and counts_of(main).sum() == 0


@pytest.mark.parametrize("paired", [False, True])
def test_all_hit_path(case, paired):
    """Every read is under the screen's k: no hit pair at all, the all-hit bytes alone decide."""
    rng = np.random.default_rng(4)
    reads = [_dna(rng, int(n)) for n in rng.integers(5, KA, 600)]
    prep = prep_ref.prep_block(reads, None, paired=paired, min_length=5)
    want = case.deplete(prep, case.a_o, 1.0, paired=paired)
    assert want["units_removed"] == want["n_units"] == (300 if paired else 600) and want["leaf_counts"] == [want["n_units"]] * 4
    fresh(case.a)
    case.prepare(reads, None, paired=paired, min_length=5)
    case.check(case.main.prep_deplete(case.a, 1.0, paired=paired), want, paired)
    assert counts_of(case.a).tolist() == want["leaf_counts"]
    fresh(case.a)


@pytest.mark.parametrize("paired", [False, True])
def test_a_full_hit_buffer_is_retried(case, paired):
    """PFQ_HIT_SLOTS = 0 on the screen: the first attempt has no room for a single hit pair, and no unit may survive for it; the
    screen's counters are restored and count once."""
    main, a = case.main, case.a
    reads = fragments(case) if paired else case.prep["kept_reads"]
    prep = prep_ref.prep_block(reads, None, paired=paired, min_length=5)
    want = case.deplete(prep, case.a_o, THR, paired=paired)
    assert want["units_removed"] > 0
    fresh(a)
    a.set_option("PFQ_HIT_SLOTS", "0")
    try:
        case.prepare(reads, None, paired=paired, min_length=5)
        case.check(main.prep_deplete(a, THR, paired=paired), want, ("retry", paired))
        c = a.last_capacity()
        assert c["attempts"] == 2 and c["hit_cap"] == 0 < c["hit_cursor"], c
    finally:
        a.set_option("PFQ_HIT_SLOTS", None)
    assert counts_of(a).tolist() == want["leaf_counts"]
    fresh(a)


def test_refusals(case, tmp_path):
    main, a, L = case.main, case.a, _ffi.lib()
    fresh(main, a)
    main.query_packed(*pack_reads(case.reads[:20]), THR)
    a.query_packed(*pack_reads(case.reads[:20]), THR)
    case.prepare(case.reads[:60], case.quals[:60], **TRIM)
    state = lambda: (counts_of(main).tolist(), counts_of(a).tolist(), [x.tobytes() for x in main.prep_csr()])
    before = state()
    out = _ffi.PrepDepleted()

    def refused(code, tree, screen, flags=0):
        assert L.pfq_prep_deplete(tree, screen, THR, flags, C.byref(out)) == code
        assert state() == before

    refused(PFQ_ERR_ARG, None, a._h)
    refused(PFQ_ERR_ARG, main._h, None)
    assert L.pfq_prep_deplete(main._h, a._h, THR, 0, None) == PFQ_ERR_ARG and state() == before
    refused(PFQ_ERR_ARG, main._h, main._h)                            # screen == tree
    for flags in (_ffi.PAIR_BOTH, _ffi.WANT_HITS, _ffi.PAIRED | _ffi.WANT_LCA, 1 << 20):
        refused(PFQ_ERR_ARG, main._h, a._h, flags)
    refused(PFQ_ERR_ARG, main._h, a._h, _ffi.PAIRED)                  # PFQ_PAIRED on a block prepared unpaired
    ids = [f"A{i:02d}" for i in range(4)]
    n_dev = C.c_int(0)
    assert L.pfq_device_count(C.byref(n_dev)) == 0
    if n_dev.value > 1:                                               # trees on different devices
        far = BloomTree.build_balanced(case.a_g, ids, KA, NBITS_A, HA, *SEEDS_A, device=1)
        refused(PFQ_ERR_ARG, main._h, far._h)
        far.close()
    unprepared = BloomTree.build_balanced(case.a_g[:2], ids[:2], KA, NBITS_A, HA, *SEEDS_A)
    assert L.pfq_prep_deplete(unprepared._h, a._h, THR, 0, C.byref(out)) == PFQ_ERR_STATE and state() == before    # before any prep
    unprepared.close()
    empty = BloomTree.new(KA, 0.01, 10000, *SEEDS_A)
    refused(PFQ_ERR_STATE, main._h, empty._h)                         # an empty screen
    empty.close()
    a.save(str(tmp_path / "a"))
    shard = BloomTree.load_subtree(str(tmp_path / "a"), 1, 0)
    refused(PFQ_ERR_UNSUPPORTED, main._h, shard._h)                   # a subtree shard's rows are partial
    shard.close()
    genome = _one_child_db(tmp_path / "one_child", False)             # a sticky insertion error, on the screen and on the tree
    bad = BloomTree.load(str(tmp_path / "one_child"))
    bad.set_option("PFQ_GREEDY_HOST", "1")
    with pytest.raises(PfqError):
        bad.insert(genome, "new")
    refused(PFQ_ERR_FORMAT, main._h, bad._h)
    bad.prep_reads(*pack_reads(case.reads[:10]))
    assert L.pfq_prep_deplete(bad._h, a._h, THR, 0, C.byref(out)) == PFQ_ERR_FORMAT and state() == before
    bad.close()
    with pytest.raises(PfqError) as e:
        a.last_deplete_ms()                                           # the screen's own blocks were never depleted
    assert e.value.code == PFQ_ERR_STATE
    # after all that the call still works on the block prepared before
    want = case.deplete(prep_ref.prep_block(case.reads[:60], case.quals[:60], **TRIM), case.a_o, THR)
    case.check(main.prep_deplete(a, THR), want, "after the refusals")
    fresh(main, a)


# ---------------------------------------------------------------------------------------------------------------
# behind the other prep steps
# ---------------------------------------------------------------------------------------------------------------
STEPS = dict(O=30, E=10, high=30, low=14, par=dict(trim_quality=20, trim_window=4, min_length=K))


def worked_fragments(case):
    """150 fragments of 60 .. 200 bases as tests/test_gpu_correct.py builds them for test_with_adapters_and_quality_trimming, but
    with inserts of the screen's genomes and of the main tree's by turns: adapter read-through, a low-quality tail on some second
    mates, and in three of four overlaps one wrong base per mate, of quality 2 against 40 — at threshold 1 either hides its mate
    from the tree the insert comes from until it is corrected.  Returns reads, quals."""
    rng = np.random.default_rng(4800)
    background = np.frombuffer(b"5?IJ", dtype=np.uint8)
    reads, quals = [], []
    for n in range(150):
        L1, L2 = (int(v) for v in rng.integers(60, 200, 2))
        I = int(rng.integers(40, 230))
        g = case.a_g[n % 4] if n % 2 else case.main_g[n % 16]
        ins = piece(rng, g, I)
        a = bytearray((ins + (AD33 if n % 3 == 0 else b"") + _dna(rng, L1))[:L1])
        b = bytearray((orc.revcomp(ins) + _dna(rng, L2))[:L2])
        q1, q2 = (bytearray(rng.choice(background, L).astype(np.uint8)) for L in (L1, L2))
        lo, hi = max(0, I - L2), min(I, L1)
        if n % 4 and hi - lo >= 30:
            i1, i2 = sorted(rng.choice(hi - lo, 2, replace=False).tolist())
            a[lo + i1], q1[lo + i1], q2[I - 1 - lo - i1] = other_base(rng, a[lo + i1]), 2 + 33, 40 + 33
            b[I - 1 - lo - i2], q2[I - 1 - lo - i2], q1[lo + i2] = other_base(rng, b[I - 1 - lo - i2]), 2 + 33, 40 + 33
        if n % 7 == 2 and I > 14:
            q2[I - 6:] = b"#" * len(q2[I - 6:])
        reads += [bytes(a), bytes(b)]
        quals += [None if n % 13 == 12 else bytes(q1), bytes(q2)]
    return reads, quals


@pytest.fixture(scope="module")
def worked(case):
    """The fragments and, from the references alone, the prepared block with and without the correction."""
    reads, quals = worked_fragments(case)
    s = STEPS
    with_c = correct_ref.prep_block(reads, quals, s["O"], s["E"], s["high"], s["low"], [AD33], **s["par"])
    without = overlap_ref.prep_block(reads, quals, s["O"], s["E"], [AD33], **s["par"])
    cor = with_c["corrections"]
    assert min(cor["n_bases"]) > 40 and with_c["adapters"]["n_found"] >= 15 and with_c["n_overlapped"] > 100 and with_c["n_trimmed"] > 100
    return reads, quals, with_c, without


def same_report(got, want, tag):
    """Two read-outs of pfq_prep_last_adapters / _overlap / _corrections, field by field."""
    assert got.keys() == want.keys(), tag
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and np.array_equal(got[k], v), (tag, k)
        else:
            assert got[k] == v, (tag, k, got[k], v)


@pytest.mark.parametrize("mode", [None, "either", "both"], ids=["unpaired", "either", "both"])
@pytest.mark.parametrize("want_reads", [False, True], ids=["corrected in the overlap kernel", "corrected by the patch kernel"])
def test_behind_adapters_overlap_and_correction(case, worked, want_reads, mode):
    """The depletion re-gathers from the raw block the correction changed in place (in the overlap kernel, or with want_reads in
    the patch kernel), by begin / len that hold min(adapter cut, overlap cut): expected is deplete_ref on correct_ref's kept
    reads.  What the three steps reported and the arrays the prep handed out are after the call what they were before it."""
    main, a, L = case.main, case.a, _ffi.lib()
    reads, quals, with_c, without = worked
    kw = dict(paired=mode is not None, both=mode == "both")
    want = case.deplete(with_c, case.a_o, 1.0, **kw)
    plain = case.deplete(without, case.a_o, 1.0, **kw)
    gone = lambda prep, ref: {prep["kept"][i] // 2 for i in range(len(prep["kept"])) if ref["removed"][i // (2 if mode else 1)]}
    by_correction = gone(with_c, want) - gone(without, plain)
    assert len(by_correction) >= 10, len(by_correction)              # removed only because a correction restored a k-mer of the screen
    main_hits = lambda ref: sum(map(bool, deplete_ref.leaf_sets(case.main_o, ref["survivors"], 1.0)))
    assert main_hits(want) >= main_hits(plain) + 10                   # ... and survivors the main tree sees only corrected
    assert 0 < want["units_removed"] < want["n_units"]
    fresh(main, a)
    seq, off, qual, hq = pack_quals(reads, quals)
    s = STEPS
    par = _ffi.PrepParams(s["par"]["trim_quality"], s["par"]["trim_window"], 0, s["par"]["min_length"], _ffi.PREP_MAX_N_OFF, 0,
                          _ffi.PREP_PAIRED | (_ffi.PREP_WANT_READS if want_reads else 0))
    out = _ffi.Prep()
    n = len(reads)
    try:
        main.set_adapters([AD33])
        main.set_mate_overlap(s["O"], s["E"])
        main.set_mate_correct(s["high"], s["low"])
        # (the C call, so that the library-owned arrays it hands out can be read again after the depletion)
        _ffi.check(L.pfq_prep_reads(main._h, seq.ctypes.data, qual.ctypes.data, off.ctypes.data, hq.ctypes.data, n, C.byref(par), C.byref(out)))
        main._prep_shape, main._prep_reads = (int(out.n_kept), int(out.bases_kept)), n
        assert int(out.n_kept) == with_c["n_kept"]
        handed = lambda: {k: np.ctypeslib.as_array(getattr(out, k), shape=(m,)).copy() for k, m in
                          (("begin", n), ("len", n), ("reason", n), ("kept", with_c["n_kept"]))} if want_reads else {}
        for k, v in handed().items():
            assert v.tolist() == with_c[k], k
        reports = (main.last_adapters, main.last_overlap, main.last_corrections)
        before = [call() for call in reports]
        assert before[2]["n_bases"] == with_c["corrections"]["n_bases"] and (before[2]["patches"] is not None) == want_reads
        got = main.prep_deplete(a, 1.0, paired=mode is not None, pair_mode=mode or "either")
        case.check(got, want, (want_reads, mode), arrays=want_reads)
        assert counts_of(a).tolist() == want["leaf_counts"] and counts_of(main).sum() == 0
        for call, was in zip(reports, before):
            same_report(call(), was, call.__name__)
        for k, v in handed().items():
            assert v.tolist() == with_c[k], (k, "changed by the depletion")
        qkw = dict(want_hits=True, paired=mode is not None, pair_mode=mode or "either")
        want_off, want_leaves = main.query_packed(*pack_reads(want["survivors"]), 1.0, **qkw)
        want_counts = counts_of(main)
        assert want_counts.sum() > 0
        fresh(main)
        off_, leaves = main.query_prep(1.0, **qkw)
        assert off_.tolist() == want_off.tolist() and leaves.tolist() == want_leaves.tolist()
        assert counts_of(main).tolist() == want_counts.tolist()
    finally:
        main.set_adapters([])
        main.set_mate_correct(0)
        main.set_mate_overlap(0)
        fresh(main, a)


# ---------------------------------------------------------------------------------------------------------------
# the retry with something to lose
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_the_retry_restores_counters_that_are_not_zero(case, paired):
    """As test_a_full_hit_buffer_is_retried, but the screen's counters hold an earlier, synchronised query and a counts-only
    query_device of the screen was issued on a user stream and not waited for: afterwards they are the earlier call's plus the
    one in flight plus the depletion's, counted exactly once."""
    main, a = case.main, case.a
    reads = fragments(case) if paired else case.prep["kept_reads"]
    prep = prep_ref.prep_block(reads, None, paired=paired, min_length=5)
    want = case.deplete(prep, case.a_o, THR, paired=paired)
    assert want["units_removed"] > 0
    earlier, flying = case.reads[:60], case.reads[60:] * 4
    c_earlier, c_flying = oracle_counts(case.a_o, earlier, THR), oracle_counts(case.a_o, flying, THR)
    assert sum(c_earlier) > 0 and sum(c_flying) > 0
    fresh(a)
    a.query_packed(*pack_reads(earlier), THR)
    assert counts_of(a).tolist() == c_earlier
    seq, off = pack_reads(flying)
    d_seq, d_off, stream = DeviceBuffer.from_numpy(seq), DeviceBuffer.from_numpy(off), stream_create()
    try:
        case.prepare(reads, None, paired=paired, min_length=5)
        a.query_device(d_seq.ptr, d_off.ptr, len(flying), int(off[-1]), THR, stream=stream)       # not waited for
        a.set_option("PFQ_HIT_SLOTS", "0")
        try:
            case.check(main.prep_deplete(a, THR, paired=paired), want, ("retry with counters", paired))
            c = a.last_capacity()
            assert c["attempts"] == 2 and c["hit_cap"] == 0 < c["hit_cursor"], c
        finally:
            a.set_option("PFQ_HIT_SLOTS", None)
        stream_synchronize(stream)
        assert counts_of(a).tolist() == (np.array(c_earlier) + np.array(c_flying) + np.array(want["leaf_counts"])).tolist()
    finally:
        stream_synchronize(stream)
        stream_destroy(stream)
        fresh(a)
