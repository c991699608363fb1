"""tests/correct_ref.py against hand-written cases of the rule of pfq.h "mate correction" — each branch, the bounds, N on either
side, lower case, a mate without qualities, a pair behind the adapter cut, no mismatch — and against its own properties: the patch
list applied to the originals gives the corrected reads, the mismatches left are the unresolved pairs, correcting twice changes
nothing more."""
import numpy as np

import correct_ref
import overlap_ref
import prep_ref
from test_overlap_cpu import AD33, dna, fragment, revcomp

INS = b"ACGTTGCAAGGCTTAGCCATGCAAGTCTGACC"                             # 32 bases
O, E = 8, 20


def q_of(p):
    return p + 33


def one(i, wrong, p1, p2, side=1, L=32, base=None):
    """Mates of L bases of INS (the whole insert: pair (i, j = 31 - i)), all qualities 40, with `wrong` written at pair i into mate
    `side` (1: b[j], 0: a[i]) and the qualities p1, p2 at that pair.  Returns a, b, q1, q2, i, j."""
    a, b = bytearray(INS[:L] + b"T" * (L - 32)), bytearray(revcomp(INS)[:L] + b"G" * (L - 32))
    j = len(INS) - 1 - i
    q1, q2 = bytearray(b"I" * L), bytearray(b"I" * L)
    if side == 1:
        b[j] = wrong
    else:
        a[i] = wrong
    if base is not None:
        (a if side == 1 else b)[i if side == 1 else j] = base
    q1[i], q2[j] = q_of(p1), q_of(p2)
    return bytes(a), bytes(b), bytes(q1), bytes(q2), i, j


def run(a, b, q1, q2, **kw):
    return correct_ref.correct_fragment(a, b, q1, q2, O, E, **kw)


def test_each_branch_of_the_rule():
    # mate 1 high, mate 2 low: mate 2 takes comp(a[i]) and a's raw quality byte
    a, b, q1, q2, i, j = one(5, ord("A") if revcomp(INS)[26:27] != b"A" else ord("C"), 40, 2)
    assert overlap_ref.find_insert(a, b, O, E) == (32, 1)
    na, nb, nq1, nq2, pt, un, noq = run(a, b, q1, q2)
    assert (na, nq1) == (a, q1) and nb == revcomp(INS) and nq2 == q2[:j] + b"I" + q2[j + 1:]
    assert pt == [(1, j, revcomp(INS)[j], q_of(40), b[j], q_of(2))] and un == 0 and not noq
    # the roles swapped
    a, b, q1, q2, i, j = one(9, ord("A") if INS[9:10] != b"A" else ord("C"), 3, 35, side=0)
    na, nb, nq1, nq2, pt, un, noq = run(a, b, q1, q2)
    assert (nb, nq2) == (b, q2) and na == INS and nq1[i] == q_of(35) and pt == [(0, i, INS[i], q_of(35), a[i], q_of(3))] and un == 0
    # neither: both high, both low, high against middling
    for p1, p2 in ((40, 40), (2, 2), (40, 20), (20, 2), (29, 2), (40, 15)):
        a, b, q1, q2, i, j = one(5, ord("A") if revcomp(INS)[26:27] != b"A" else ord("C"), p1, p2)
        assert run(a, b, q1, q2) == (a, b, q1, q2, [], 1, False), (p1, p2)


def test_the_bounds_exactly_and_one_off():
    wrong = ord("A") if revcomp(INS)[26:27] != b"A" else ord("C")
    for p1, p2, fixed in ((30, 14, True), (29, 14, False), (31, 14, True), (30, 15, False), (30, 13, True), (93, 0, True)):
        a, b, q1, q2, i, j = one(5, wrong, p1, p2)
        got = run(a, b, q1, q2)
        assert (len(got[4]), got[5]) == ((1, 0) if fixed else (0, 1)), (p1, p2)
    # a quality byte below '!' counts as 0; other bounds by the arguments
    a, b, q1, q2, i, j = one(5, wrong, 40, 2)
    q2 = q2[:j] + b"\x1f" + q2[j + 1:]
    assert len(run(a, b, q1, q2)[4]) == 1
    assert len(run(a, b, q1, q2, high=41, low=14)[4]) == 0 and len(run(a, b, q1, q2, high=40, low=0)[4]) == 1
    a, b, q1, q2, i, j = one(5, wrong, 40, 2)
    assert len(run(a, b, q1, q2, high=40, low=1)[4]) == 0 and len(run(a, b, q1, q2, high=3, low=2)[4]) == 1


def test_n_and_lower_case():
    # N on the low side is repaired; the written base is upper case whatever the mate's case
    a, b, q1, q2, i, j = one(5, ord("N"), 40, 2)
    got = run(a, b, q1, q2)
    assert got[1] == revcomp(INS) and got[4][0][2:] == (revcomp(INS)[j], q_of(40), ord("N"), q_of(2))
    got = run(a.lower(), b, q1, q2)
    assert got[0] == a.lower() and got[1] == revcomp(INS) and len(got[4]) == 1
    got = run(a, b.lower(), q1, q2)                                   # the corrected base alone becomes upper case
    assert got[1] == b.lower()[:j] + revcomp(INS)[j:j + 1] + b.lower()[j + 1:]
    # N on the high side never corrects: not the N's mate, and not the N (the mate's quality is low)
    a, b, q1, q2, i, j = one(5, ord("N"), 2, 40)                      # b[j] = N with quality 40, a[i] good with quality 2
    assert run(a, b, q1, q2) == (a, b, q1, q2, [], 1, False)
    a, b, q1, q2, i, j = one(5, ord("n"), 40, 2, side=0)              # a[i] = n with quality 40
    assert run(a, b, q1, q2) == (a, b, q1, q2, [], 1, False)
    a, b, q1, q2, i, j = one(5, ord("n"), 2, 40, side=0)              # a[i] = n with quality 2: repaired from b
    assert run(a, b, q1, q2)[0] == INS
    # lower case that matches is no mismatch
    a, b, q1, q2, i, j = one(5, revcomp(INS).lower()[26], 40, 2)
    assert overlap_ref.find_insert(a, b, O, E) == (32, 0) and run(a, b, q1, q2) == (a, b, q1, q2, [], 0, False)


def test_qualities_missing_no_mismatch_no_insert():
    wrong = ord("A") if revcomp(INS)[26:27] != b"A" else ord("C")
    a, b, q1, q2, i, j = one(5, wrong, 40, 2)
    assert run(a, b, None, q2) == (a, b, None, q2, [], 0, True) and run(a, b, q1, None) == (a, b, q1, None, [], 0, True)
    assert run(INS, revcomp(INS), q1, None) == (INS, revcomp(INS), q1, None, [], 0, False)      # mm == 0: nothing, and not counted
    assert run(INS, revcomp(INS), q1, q2) == (INS, revcomp(INS), q1, q2, [], 0, False)
    rng = np.random.default_rng(1)
    x, y = dna(rng, 40), dna(rng, 40)
    assert overlap_ref.find_insert(x, y, O, E)[0] == overlap_ref.NO_INSERT
    assert correct_ref.correct_fragment(x, y, b"#" * 40, b"I" * 40, O, E)[4:] == ([], 0, False)
    long_a = INS * 17                                                 # 544 bases: not analysed
    assert correct_ref.correct_fragment(long_a, revcomp(long_a), b"#" * 544, b"I" * 544, O, E)[4:] == ([], 0, False)
    res = correct_ref.correct_block([a, b, a, b, INS, revcomp(INS)], [q1, q2, None, q2, q1, None], O, E)
    assert [res[k] for k in correct_ref.TOTALS] == [1, [0, 1], 0, 1] and res["patches"] == [(1, j, revcomp(INS)[j], q_of(40), wrong, q_of(2))]
    res = correct_ref.correct_block([a, b], None, O, E)
    assert [res[k] for k in correct_ref.TOTALS] == [0, [0, 0], 0, 1] and res["quals"] is None and res["reads"] == [a, b]


def test_a_pair_behind_the_adapter_cut_and_trimming_on_corrected_qualities():
    # insert of 32 in mates of 60: the adapter follows the insert.  A correction at a[30] lies in front of the cuts; one planted
    # behind an adapter cut that comes earlier is still reported
    rng = np.random.default_rng(2)
    a = INS + AD33[:28]
    b = revcomp(INS) + dna(rng, 28)
    q1, q2 = bytearray(b"I" * 60), bytearray(b"I" * 60)
    a = bytearray(a)
    a[30] = ord("A") if INS[30:31] != b"A" else ord("C")
    q1[30] = q_of(2)
    a, q1, q2 = bytes(a), bytes(q1), bytes(q2)
    res = correct_ref.prep_block([a, b], [q1, q2], O, E, set1=[AD33], trim_quality=20, trim_window=1)
    assert res["insert"] == [32] and res["mismatches"] == [1] and res["cut"] == [32, 32]
    assert res["corrections"]["patches"] == [(0, 30, INS[30], q_of(40), a[30], q_of(2))]
    assert res["len"] == [32, 32] and res["kept_reads"] == [INS, revcomp(INS)]                  # the old quality would have ended mate 1 at 30
    plain = overlap_ref.prep_block([a, b], [q1, q2], O, E, [AD33], trim_quality=20, trim_window=1)
    assert plain["len"] == [30, 32]
    # an "adapter" that matches at 20: pair (30, 1) is behind mate 1's cut
    res = correct_ref.prep_block([a, b], [q1, q2], O, E, set1=[a[20:32] + AD33[:10]], adapter_O=12, adapter_E=0)
    assert res["adapters"]["cut"][0] == 20 and res["cut"][0] == 20 and res["len"][0] == 20
    assert res["corrections"]["patches"] == [(0, 30, INS[30], q_of(40), a[30], q_of(2))]        # behind the cut, still reported


def noisy_block(rng, n_frag, with_quals=True):
    reads, quals = [], []
    for n in range(n_frag):
        L1, L2 = (int(v) for v in rng.integers(20, 90, 2))
        I = int(rng.integers(10, 140))
        a, b = (bytearray(s) for s in fragment(rng, I, L1, L2))
        qs = [bytearray(rng.choice(np.frombuffer(b"#/0>?I", dtype=np.uint8), len(s), p=[.2, .1, .1, .1, .1, .4]).astype(np.uint8)) for s in (a, b)]
        for s in (a, b):
            for j in np.flatnonzero(rng.random(len(s)) < 0.04).tolist():
                s[j] = ord("ACGTNacgtn"[int(rng.integers(10))])
        reads += [bytes(a), bytes(b)]
        quals += [None if n % 11 == 3 else bytes(qs[0]), None if n % 13 == 5 else bytes(qs[1])]
    return reads, quals


def test_properties():
    rng = np.random.default_rng(8)
    reads, quals = noisy_block(rng, 300)
    res = correct_ref.correct_block(reads, quals, 12, 20)
    assert res["n_fragments_corrected"] > 40 and min(res["n_bases"]) > 20 and res["n_unresolved"] > 40 and res["n_no_quality"] > 5
    assert res["patches"] == sorted(res["patches"]) and len(res["patches"]) == sum(res["n_bases"])
    assert len({p[:2] for p in res["patches"]}) == len(res["patches"])
    # the patches applied to the originals give the corrected reads
    assert correct_ref.apply_patches(reads, quals, res["patches"]) == (res["reads"], res["quals"])
    # at the same insert the corrected pair mismatches exactly where pairs were unresolved
    unresolved = 0
    for f in range(len(reads) // 2):
        a, b, q1, q2 = reads[2 * f], reads[2 * f + 1], quals[2 * f], quals[2 * f + 1]
        I, mm = overlap_ref.find_insert(a, b, 12, 20)
        na, nb, _, _, pt, un, noq = correct_ref.correct_fragment(a, b, q1, q2, 12, 20)
        if I == overlap_ref.NO_INSERT:
            assert not pt and not un
            continue
        left = 0
        for i in range(max(0, I - len(b)), min(I, len(a))):
            ua, ub = prep_ref.up(na[i]), prep_ref.up(nb[I - 1 - i])
            left += not (ua in overlap_ref.COMP and ub in overlap_ref.COMP and ua == overlap_ref.COMP[ub])
        assert left == (mm if noq else un) and len(pt) + un == (0 if noq else mm), f
        unresolved += un
    assert unresolved == res["n_unresolved"]
    # correcting twice changes nothing more (a corrected pair agrees; an unresolved one stays unresolved)
    for f in range(len(reads) // 2):
        first = correct_ref.correct_fragment(reads[2 * f], reads[2 * f + 1], quals[2 * f], quals[2 * f + 1], 12, 20)
        if overlap_ref.find_insert(first[0], first[1], 12, 20)[0] != overlap_ref.find_insert(reads[2 * f], reads[2 * f + 1], 12, 20)[0]:
            continue                                                  # (the corrected mates may match at a larger insert: another hypothesis)
        again = correct_ref.correct_fragment(*first[:4], 12, 20)
        assert again[:4] == first[:4] and again[4] == [], f


def test_prep_block_equals_the_overlap_reference_on_the_corrected_mates():
    rng = np.random.default_rng(9)
    reads, quals = noisy_block(rng, 120)
    params = dict(trim_quality=20, trim_window=4, min_length=15, max_n=2)
    got = correct_ref.prep_block(reads, quals, 12, 20, set1=[AD33], **params)
    orig = overlap_ref.prep_block(reads, quals, 12, 20, [AD33], **params)
    for k in (*overlap_ref.TOTALS, "insert", "mismatches", "ocut", "cut", "hist", "adapters"):
        assert got[k] == orig[k], k
    cor = got["corrections"]
    cut_reads = [s[:c] for s, c in zip(cor["reads"], orig["cut"])]
    cut_quals = [None if q is None else q[:c] for q, c in zip(cor["quals"], orig["cut"])]
    want = prep_ref.prep_block(cut_reads, cut_quals, paired=True, **params)
    for k in ("n_reads", "n_kept", "bases_kept", "n_reason", "begin", "len", "reason", "kept", "kept_reads"):
        assert got[k] == want[k], k
    assert got["bases_in"] == orig["bases_in"] and len(cor["patches"]) > 20
    untrimmed = correct_ref.prep_block(reads, quals, 12, 20)          # no trim step: the corrected mates, cut at ocut
    assert untrimmed["kept_reads"] == [s[:c] for s, c in zip(cor["reads"], orig["ocut"])] != [s[:c] for s, c in zip(reads, orig["ocut"])]
    off = correct_ref.prep_block(reads, quals, 12, 20, high=93, low=0, set1=[AD33], **params)  # nothing qualifies: the plain result
    assert off["corrections"]["patches"] == [] and all(off[k] == orig[k] for k in ("begin", "len", "reason", "kept", "kept_reads"))
