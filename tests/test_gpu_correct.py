"""pfq_tree_set_mate_correct / pfq_prep_reads / pfq_prep_last_corrections on the device against tests/correct_ref.py: the totals,
the patch list exact and in order, begin, len, reason, kept and the prepared CSR byte for byte, the overlap and adapter steps
unchanged — over the mate lengths and start alignments of test_gpu_overlap, mismatches at the edges of the overlap and of the
kernel's words, quality pairs on both sides of both bounds, mates without qualities, calls with and without the patch list, split
and permuted blocks, together with adapters and quality trimming, over more fragments than a grid trip and a scan block hold; then
what the option is for: a fragment with one low-quality error in its overlap is classified like the error-free one."""
import numpy as np
import pytest

import correct_ref
import overlap_ref
from phagefilter_amd import BloomTree, PfqError, pack_reads
from test_gpu_build import SEEDS, _dna
from test_gpu_overlap import AD33, NO, Case, lengths_of, other_base, planted
from test_gpu_prep import H, K, NBITS, PFQ_ERR_ARG, PFQ_ERR_STATE, SCAN_ITEMS, TOTALS, TRIP_READS, pack_quals
from test_overlap_cpu import revcomp

pytestmark = pytest.mark.gpu

# (p1, p2) of a planted mismatch: on both sides of high = 30 and low = 14, either role, both high, both low, the extremes
QUAL_PAIRS = ((30, 14), (29, 14), (30, 15), (31, 13), (14, 30), (14, 29), (15, 30), (13, 31), (40, 40), (2, 2), (40, 2), (2, 40), (93, 0), (0, 93), (40, 20))
BACKGROUND = np.frombuffer(b"#/0>?I", dtype=np.uint8)


def planted_q(rng, I, L1, L2, pairs=(), n_random=0, kinds="ab", menu=QUAL_PAIRS, background=BACKGROUND):
    """Mates of an insert of I bases and their qualities.  Pair m of the overlap (i = lo + m) for every m of `pairs`, and n_random
    more, mismatches — a substitution in mate 1 ("a") or mate 2 ("b"), or an N ("n", "N": in mate 1 or 2) by turns through `kinds`
    — and takes its qualities from `menu` by turns."""
    a, b = (bytearray(s) for s in planted(rng, I, L1, L2))
    q1, q2 = (bytearray(rng.choice(background, L).astype(np.uint8)) for L in (L1, L2))
    lo, hi = max(0, I - L2), min(I, L1)
    ms = [m for m in pairs if m < hi - lo]
    if n_random:
        rest = [m for m in range(hi - lo) if m not in ms]
        ms += rng.choice(rest, n_random, replace=False).tolist()
    start = int(rng.integers(len(menu)))
    for t, m in enumerate(ms):
        i = lo + m
        j = I - 1 - i
        kind = kinds[t % len(kinds)]
        if kind == "a":
            a[i] = other_base(rng, a[i])
        elif kind == "b":
            b[j] = other_base(rng, b[j])
        elif kind == "n":
            a[i] = ord("Nn"[t // 2 % 2])
        else:
            b[j] = ord("nN"[t // 2 % 2])
        p1, p2 = menu[(start + t) % len(menu)]
        q1[i], q2[j] = p1 + 33, p2 + 33
    return bytes(a), bytes(b), bytes(q1), bytes(q2)


def shape_block(rng, O, E):
    """Fragments over lengths_of(O), equal and unequal mates, inserts below, at and above the mates' lengths, with mismatches at
    the first and the last pair of the overlap, at pairs 15, 16, 17 of a word, several in one word, exactly the allowed number
    and one more; every seventh fragment has a mate without qualities.  Returns reads, quals."""
    Ls = lengths_of(O)
    frags = []
    for L1, L2 in [(L, L) for L in Ls] + [(L, Ls[(i + 5) % len(Ls)]) for i, L in enumerate(Ls)]:
        lo, hi = min(L1, L2), max(L1, L2)
        for I in sorted({O + 1, lo - 3, lo, hi, hi + 2, L1 + L2 - O}):
            o = min(I, L1) - max(0, I - L2)
            if not (O <= I <= L1 + L2 - O and o >= O):
                continue
            allowed = E * o // 100
            sets = [[0, o - 1], [m for m in (15, 16, 17) if m < o], [m for m in (32, 33, 35, 38, 47) if m < o], [o - 1], []]
            for n, ms in enumerate(sets):
                ms = sorted(set(ms))[:allowed]
                frags.append(planted_q(rng, I, L1, L2, ms, kinds=("ab", "ba", "abnN", "b", "a")[n]))
            several = [m for m in (33, 34, 36, 39, 46, 47) if m < o][:allowed]                # ... of one word, all corrected in one mate
            frags.append(planted_q(rng, I, L1, L2, several, kinds="b", menu=((40, 2), (93, 14), (30, 0))))
            frags.append(planted_q(rng, I, L1, L2, several, kinds="a", menu=((2, 40), (14, 93), (0, 30))))
            if allowed <= o:
                frags.append(planted_q(rng, I, L1, L2, (), allowed, kinds="abNn"))          # mm exactly at the bound
            if allowed + 1 <= o:
                frags.append(planted_q(rng, I, L1, L2, (), allowed + 1))                    # one more: this I does not match
        a, b, q1, q2 = planted_q(rng, max(O, lo - 1), L1, L2, [0] if E else [])
        frags.append((a.lower(), b[:L2 // 2] + b[L2 // 2:].lower(), q1, q2))
    reads, quals = [], []
    for n, i in enumerate(rng.permutation(len(frags)).tolist()):
        a, b, q1, q2 = frags[i]
        reads += [a, b]
        quals += [None if n % 7 == 3 else q1, None if n % 7 == 6 and n % 2 else q2]
    return reads, quals


PATCH_FIELDS = ("read", "pos", "base", "qual", "old_base", "old_qual")


def check(case, reads, quals, O, E, high=30, low=14, set1=(), set2=(), adapter_O=5, adapter_E=10, want_reads=True, packed=None, want=None, **params):
    """One paired device call with the correction against the reference: the correction's totals and patches, what the overlap
    step, the adapter step and the prep report, and the CSR."""
    gt = case.gt
    want = want or correct_ref.prep_block(reads, quals, O, E, high, low, set1, set2, adapter_O, adapter_E, **params)
    if quals is None:
        (seq, off), qual, hq = packed or pack_reads(reads), None, None
    else:
        seq, off, qual, hq = packed or pack_quals(reads, quals)
    gt.set_adapters(set1, set2, min_overlap=adapter_O, max_error_percent=adapter_E)
    gt.set_mate_overlap(O, E)
    gt.set_mate_correct(high, low)
    got = gt.prep_reads(seq, off, qual, hq, paired=True, want_reads=want_reads, **params)
    cor, ov = gt.last_corrections(), gt.last_overlap()
    tag = (len(reads), O, E, high, low, [len(a) for a in set1], params)
    for k in correct_ref.TOTALS:
        assert cor[k] == want["corrections"][k], (tag, k, cor[k], want["corrections"][k])
    if want_reads:
        w = want["corrections"]["patches"]
        g = cor["patches"]
        assert g.dtype == BloomTree.PATCH_DTYPE and g.dtype.itemsize == 12 and g.shape == (len(w),), (tag, g.shape, len(w))
        got_list = list(zip(*(g[k].tolist() for k in PATCH_FIELDS)))
        bad = [n for n, (x, y) in enumerate(zip(got_list, w)) if x != y][:4]
        assert not bad, (tag, [(got_list[n], w[n], len(reads[w[n][0]]), int(off[w[n][0]]) & 15) for n in bad])
    else:
        assert cor["patches"] is None, tag
    for k in overlap_ref.TOTALS:
        assert ov[k] == want[k], (tag, k, ov[k], want[k])
    assert ov["hist"].tolist() == want["hist"], tag
    for k in TOTALS:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    checks = [("insert", ov, np.uint32, want), ("mismatches", ov, np.uint32, want), ("begin", got, np.uint32, want), ("len", got, np.uint32, want),
              ("reason", got, np.uint32, want), ("kept", got, np.uint32, want)]
    if len(set1):
        ad = gt.last_adapters()
        for k in ("n_reads", "n_found", "bases_cut", "found"):
            assert ad[k] == want["adapters"][k], (tag, k)
        checks += [("cut", ad, np.uint32, want["adapters"]), ("which", ad, np.uint8, want["adapters"])]
    if want_reads:
        for k, src, dtype, ref in checks:
            g, w = src[k], np.array(ref[k], dtype=dtype)
            assert g.dtype == dtype and g.shape == w.shape, (tag, k)
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, (tag, k, bad[:8], g[bad[:8]], w[bad[:8]])
    else:
        assert all(got[k] is None for k in ("begin", "len", "reason", "kept")) and ov["insert"] is None, tag
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
    x.gt.set_mate_correct(0)
    x.gt.set_mate_overlap(0)
    x.gt.close()


@pytest.fixture(scope="module")
def shapes():
    rng = np.random.default_rng(4100)
    reads, quals = shape_block(rng, 30, 10)
    return reads, quals, correct_ref.prep_block(reads, quals, 30, 10, min_length=K)


def test_lengths_alignments_words_and_bounds(case, shapes):
    reads, quals, want = shapes
    check(case, reads, quals, 30, 10, want=want, min_length=K)
    off = want["off"].astype(np.int64)
    assert {int(o) & 15 for o in off[:-1:2]} == set(range(16)) and {int(o) & 15 for o in off[1:-1:2]} == set(range(16))
    cor = want["corrections"]
    assert cor["n_fragments_corrected"] > 150 and min(cor["n_bases"]) > 100 and cor["n_unresolved"] > 150 and cor["n_no_quality"] > 30
    ins, L = want["insert"], [len(s) for s in reads]
    found = [f for f in range(len(ins)) if ins[f] != NO and want["mismatches"][f]]
    assert any(ins[f] < L[2 * f + 1] for f in found) and any(ins[f] == L[2 * f + 1] for f in found) and any(ins[f] > max(L[2 * f], L[2 * f + 1]) for f in found)
    at_bound = [f for f in found if want["mismatches"][f] == 10 * (min(ins[f], L[2 * f]) - max(0, ins[f] - L[2 * f + 1])) // 100]
    assert len(at_bound) > 20
    in_word = {}                                                      # several corrections of one mate in one 16-base word
    for p in cor["patches"]:
        in_word[(p[0], p[1] // 16)] = in_word.get((p[0], p[1] // 16), 0) + 1
    assert max(in_word.values()) >= 3
    assert {p[1] % 16 for p in cor["patches"]} == set(range(16)) and max(p[1] for p in cor["patches"]) >= 500
    # the same block without the list: the same totals and CSR, and no list
    check(case, reads, quals, 30, 10, want=want, want_reads=False, min_length=K)
    # the overlap and adapter steps report what they report without the option
    plain = overlap_ref.prep_block(reads, quals, 30, 10, min_length=K)
    assert all(want[k] == plain[k] for k in (*overlap_ref.TOTALS, "insert", "mismatches", "hist", "cut")) and want["kept_reads"] != plain["kept_reads"]


@pytest.mark.parametrize("O,E,high,low", [(12, 50, 30, 14), (8, 4, 93, 0), (100, 10, 1, 0), (16, 20, 20, 19)])
def test_other_parameters(case, O, E, high, low):
    rng = np.random.default_rng(4200 + O)
    frags = []
    for n in range(90):
        L1, L2 = (int(v) for v in rng.choice([37, 64, 100, 150, 151, 256, 300], 2))
        I = int(rng.integers(max(O, 20), max(L1 + L2 - max(O, 20), max(O, 20) + 1)))
        o = max(min(I, L1) - max(0, I - L2), 0)
        n_mm = int(rng.integers(0, max(1, min(E * o // 100, 12) + 1))) if o >= O else 0
        menu = QUAL_PAIRS + ((high, low), (max(high - 1, 0), low), (high, low + 1), (low, high), (low + 1, high), (low, max(high - 1, 0)))
        frags.append(planted_q(rng, I, L1, L2, (), n_mm, kinds="abnN", menu=menu))
    reads = [s for f in frags for s in f[:2]]
    quals = [q for f in frags for q in f[2:]]
    want = check(case, reads, quals, O, E, high, low, min_length=K)
    assert want["corrections"]["n_unresolved"] > 10 and (sum(want["corrections"]["n_bases"]) > 10 or high == 93)


def test_without_qualities_for_the_call(case, shapes):
    reads, _, with_q = shapes
    want = check(case, reads, None, 30, 10, min_length=K)
    cor = want["corrections"]
    assert cor["patches"] == [] and cor["n_no_quality"] == sum(1 for m in want["mismatches"] if m) > 300 and cor["n_unresolved"] == 0
    assert want["kept_reads"] == overlap_ref.prep_block(reads, None, 30, 10, min_length=K)["kept_reads"]
    check(case, reads, None, 30, 10, want=want, want_reads=False, min_length=K)


def test_split_and_permuted_blocks(case, shapes):
    reads, quals, whole = shapes
    rng = np.random.default_rng(4300)
    n_frag = len(reads) // 2
    order = rng.permutation(n_frag).tolist()
    per_fragment = {}
    for read, pos, *rest in whole["corrections"]["patches"]:
        per_fragment.setdefault(read // 2, []).append((read % 2, pos, *rest))
    for part in (order[:n_frag // 3], order[n_frag // 3:]):
        rs = [reads[2 * f + m] for f in part for m in (0, 1)]
        qs = [quals[2 * f + m] for f in part for m in (0, 1)]
        got = check(case, rs, qs, 30, 10, min_length=K)
        for k in ("begin", "len", "reason"):
            assert got[k] == [whole[k][2 * f + m] for f in part for m in (0, 1)], k
        mine = {}
        for read, pos, *rest in got["corrections"]["patches"]:
            mine.setdefault(part[read // 2], []).append((read % 2, pos, *rest))
        assert mine == {f: v for f, v in per_fragment.items() if f in set(part)}
        assert got["insert"] == [whole["insert"][f] for f in part]


def test_with_adapters_and_quality_trimming(case):
    rng = np.random.default_rng(4400)
    reads, quals, planted_at = [], [], []
    for n in range(150):
        L1, L2 = (int(v) for v in rng.integers(60, 200, 2))
        I = int(rng.integers(40, 230))
        lo, hi = max(0, I - L2), min(I, L1)
        ms = sorted(rng.choice(hi - lo, 3, replace=False).tolist()) if n % 4 and hi - lo >= 30 else []
        # the wrong base has quality 2 and its mate's 40: after the correction the position carries 40 and no longer ends the read
        a, b, q1, q2 = planted_q(rng, I, L1, L2, ms, kinds="ab", menu=((40, 2), (2, 40)) if n % 5 else QUAL_PAIRS, background=np.frombuffer(b"5?IJ", dtype=np.uint8))
        if n % 3 == 0 and I < L1:
            a = (a[:I] + AD33 + _dna(rng, L1))[:L1]
        if n % 7 == 2 and I > 14:
            q2 = q2[:I - 6] + b"#" * len(q2[I - 6:])
        reads += [a, b]
        quals += [None if n % 13 == 12 else q1, q2]
    a, b, q1, q2 = planted_q(rng, 120, 150, 150, [100], kinds="a", menu=((2, 40),))
    reads += [a, b]
    quals += [q1, q2]
    inside = a[60:80]                                                 # an "adapter" inside this insert: the correction at 100 lies behind the cut
    packed = pack_quals(reads, quals)
    for par in (dict(trim_quality=20, trim_window=1), dict(trim_quality=20, trim_window=4, min_length=K), dict(trim_quality=25, trim_window=50, poly_x=10, max_n=3, min_complexity=30)):
        want = check(case, reads, quals, 30, 10, set1=[AD33, inside], packed=packed, **par)
        plain = overlap_ref.prep_block(reads, quals, 30, 10, [AD33, inside], **par)
        longer = sum(1 for x, y in zip(want["len"], plain["len"]) if x > y)
        # trimming saw the corrected qualities: in a window of 1 or 4 a base of quality 2 ends the read, in one of 50 it does not
        assert want["len"] != plain["len"] and (longer > 40 or par["trim_window"] > 4), (par, longer)
        assert any(pos >= want["cut"][read] for read, pos, *_ in want["corrections"]["patches"])   # behind a cut, still reported
        check(case, reads, quals, 30, 10, set1=[AD33], set2=[AD33[:20]], adapter_O=8, adapter_E=20, packed=packed, want_reads=False, **par)


def test_more_fragments_than_a_grid_trip_and_a_scan_block(case):
    rng = np.random.default_rng(4500)
    hi_q = np.frombuffer(b"I", dtype=np.uint8)
    base = [planted_q(rng, I, L1, L2, ms, kinds="ab", menu=((40, 2), (2, 40), (40, 40)), background=hi_q)
            for I, L1, L2, ms in ((30, 150, 150, []), (100, 150, 150, []), (149, 150, 151, []), (150, 150, 150, []), (220, 150, 150, []), (271, 150, 150, []),
                                  (400, 150, 150, []), (60, 100, 64, []), (90, 150, 150, []), (120, 150, 150, []), (200, 150, 150, []), (31, 150, 150, []),
                                  (90, 150, 150, [0, 17, 89]), (220, 150, 150, [3, 4, 5, 79]))]
    long_frag = planted_q(rng, 100, 600, 150, [5], menu=((40, 2),), background=hi_q)
    n_frag = (TRIP_READS + 2 * SCAN_ITEMS + 78) // 2
    frags = [base[i] for i in rng.integers(0, len(base), n_frag).tolist()]
    for j in range(30):
        frags[n_frag - 1 - 50 * j] = long_frag
    frags[0], frags[-1] = base[-1], base[-2]
    reads = [s for f in frags for s in f[:2]]
    quals = [q for f in frags for q in f[2:]]
    packed = pack_quals(reads, quals)
    want = check(case, reads, quals, 30, 10, packed=packed, min_length=K)
    cor = want["corrections"]
    assert len(cor["patches"]) > 2 * SCAN_ITEMS and cor["n_fragments_corrected"] > SCAN_ITEMS and cor["n_unresolved"] > 1000
    assert cor["patches"][0][0] < 2 and cor["patches"][-1][0] >= len(reads) - 2      # the first and the last fragment
    assert cor["n_fragments_corrected"] < n_frag // 5                  # sparse
    check(case, reads, quals, 30, 10, packed=packed, want=want, want_reads=False, min_length=K)


def test_option_off_state_and_setter_errors(case):
    gt = case.gt
    rng = np.random.default_rng(4600)
    frags = [planted_q(rng, I, 150, 150, [2, 40], kinds="ab", menu=((40, 2), (2, 40))) for I in (60, 100, 149, 200)]
    reads = [s for f in frags for s in f[:2]]
    quals = [q for f in frags for q in f[2:]]
    seq, off, qual, hq = pack_quals(reads, quals)
    want = check(case, reads, quals, 30, 10, min_length=K)
    assert want["corrections"]["n_fragments_corrected"] == 4 and gt.last_corrections_ms() >= 0.0 and gt.last_overlap_ms() >= 0.0
    for bad, named in ((dict(high=94), "high"), (dict(high=1 << 31), "high"), (dict(high=30, low=30), "low"), (dict(high=30, low=31), "low"), (dict(high=1, low=1), "low")):
        with pytest.raises(PfqError) as e:
            gt.set_mate_correct(**bad)
        assert e.value.code == PFQ_ERR_ARG and named in str(e.value), (bad, str(e.value))
    check(case, reads, quals, 30, 10, want=want, min_length=K)        # refused calls set nothing
    # kept over a prune (on a tree of its own), not run without mates or without the overlap
    fresh = BloomTree.build_balanced(case.genomes[:4], case.ids[:4], K, NBITS, H, *SEEDS)
    with pytest.raises(PfqError) as e:
        fresh.last_corrections()                                      # no prep yet
    assert e.value.code == PFQ_ERR_STATE
    fresh.set_mate_correct()                                          # 30, 14
    fresh.prep_reads(seq, off, qual, hq, paired=True, want_reads=True)
    for call in (fresh.last_corrections, fresh.last_corrections_ms):
        with pytest.raises(PfqError) as e:
            call()                                                    # no overlap set: the step did not run
        assert e.value.code == PFQ_ERR_STATE
    fresh.set_mate_overlap(30, 10)
    fresh.prune_tree(1)
    fresh.prep_reads(seq, off, qual, hq, paired=True)
    cor = fresh.last_corrections()
    assert cor["n_fragments_corrected"] == 4 and cor["n_bases"] == want["corrections"]["n_bases"] and cor["patches"] is None
    with pytest.raises(PfqError) as e:
        fresh.last_corrections_ms()                                   # no list, no second kernel
    assert e.value.code == PFQ_ERR_STATE
    fresh.prep_reads(seq, off, qual, hq, want_reads=True)             # unpaired
    with pytest.raises(PfqError) as e:
        fresh.last_corrections()
    assert e.value.code == PFQ_ERR_STATE
    fresh.close()
    # off again: the overlap step alone, as test_gpu_overlap checks it
    gt.set_mate_correct(0)
    Case.check(case, reads, quals, 30, 10, min_length=K)
    with pytest.raises(PfqError) as e:
        gt.last_corrections()
    assert e.value.code == PFQ_ERR_STATE
    # no reads: an empty report
    gt.set_mate_correct(30, 14)
    assert gt.prep_reads(*pack_reads([]), paired=True, want_reads=True)["n_reads"] == 0
    cor = gt.last_corrections()
    assert [cor[k] for k in correct_ref.TOTALS] == [0, [0, 0], 0, 0] and cor["patches"].size == 0


def test_a_low_quality_error_in_the_overlap_no_longer_hides_the_fragment(case):
    gt, g = case.gt, case.genomes
    rng = np.random.default_rng(4700)
    clean, noisy, quals, origin = [], [], [], []
    for at, n, leaf in zip(rng.integers(0, 1700, 200).tolist(), rng.integers(40, 141, 200).tolist(), rng.integers(0, 16, 200).tolist()):
        ins = g[leaf][at:at + n]
        x = int(rng.integers(0, n))                                   # the error, on the forward strand; in mate 2 it is base n - 1 - x
        for _ in range(8):
            wrong = ins[:x] + bytes([other_base(rng, ins[x])]) + ins[x + 1:]
            if not any(wrong[max(0, x - K + 1):x + K] in s or revcomp(wrong[max(0, x - K + 1):x + K]) in s for s in g):
                break                                                 # (not another strain's base)
        else:
            continue
        tail1, tail2 = _dna(rng, 150), _dna(rng, 150)
        clean += [(ins + tail1)[:150], (revcomp(ins) + tail2)[:150]]
        noisy += [(ins + tail1)[:150], (revcomp(wrong) + tail2)[:150]]
        q2 = bytearray(b"I" * 150)
        q2[n - 1 - x] = ord("#")
        quals += [b"I" * 150, bytes(q2)]
        origin.append(leaf)
    assert len(origin) > 190
    kw = dict(want_hits=True, paired=True, pair_mode="both")
    gt.set_adapters([])
    gt.set_mate_overlap(30, 10)
    gt.set_mate_correct(0)
    gt.prep_reads(*pack_quals(clean, quals), paired=True, min_length=K)
    want_off, want_leaves = gt.query_prep(1.0, **kw)
    rows = [want_leaves[int(a):int(b)].tolist() for a, b in zip(want_off, want_off[1:])]
    assert len(rows) == len(origin) and all(leaf in row for leaf, row in zip(origin, rows))
    gt.prep_reads(*pack_quals(noisy, quals), paired=True, min_length=K)
    off, _ = gt.query_prep(1.0, **kw)
    assert np.diff(off.astype(np.int64)).tolist() == [0] * len(origin)          # one wrong base: every fragment is lost
    gt.set_mate_correct(30, 14)
    gt.prep_reads(*pack_quals(noisy, quals), paired=True, min_length=K)
    cor = gt.last_corrections()
    assert cor["n_fragments_corrected"] == len(origin) and cor["n_bases"] == [0, len(origin)] and cor["n_unresolved"] == 0
    off, leaves = gt.query_prep(1.0, **kw)
    assert off.tolist() == want_off.tolist() and leaves.tolist() == want_leaves.tolist()
    gt.reset_counts()
