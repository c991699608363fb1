"""CPU only: tests/prep_ref.py against the worked examples of the contract (pfq.h "read preprocessing"), against an independent
brute-force statement of every step on random short reads, the pair rule and the totals, and purity."""
import numpy as np
import pytest

import prep_ref

# quality letters of the examples: I = 40, 5 = 20, + = 10, # = 2
EXAMPLES = [
    (b"ACGTACGTACGT", b"##IIIIIIII#I", dict(trim_quality=20, trim_window=4), (2, 10, 0)),
    (b"ACGTACGTACGT", b"IIII#I#IIIII", dict(trim_quality=20, trim_window=4), (0, 12, 0)),
    (b"ACGTACGTACGT", b"IIII5555++++", dict(trim_quality=20, trim_window=4), (0, 5, 0)),
    (b"ACG", b"I5I", dict(trim_quality=20, trim_window=4), (0, 3, 0)),
    (b"ACGTACGTAC", b"##########", dict(trim_quality=20, min_length=0), (0, 0, 0)),
    (b"ACGTACGGGGGG", None, dict(poly_x=5), (0, 6, 0)),
    (b"ACGTACGgGGnN", None, dict(poly_x=2), (0, 10, 0)),
    (b"AAAAAAAAAA", None, dict(poly_x=10, min_length=1), (0, 0, 1)),
    (b"AAAAAAAAAAAAAAAAAAAAC", None, dict(min_complexity=30), (0, 21, 3)),
    (b"ACACACACAC", None, dict(min_complexity=30), (0, 10, 0)),
    (b"ACNNGT", None, dict(max_n=1), (0, 6, 2)),
]


@pytest.mark.parametrize("s,q,params,want", EXAMPLES, ids=[f"example{i}" for i in range(len(EXAMPLES))])
def test_worked_examples(s, q, params, want):
    assert prep_ref.prep_read(s, q, **params) == want
    assert [ord(c) - 33 for c in "I5+#"] == [40, 20, 10, 2]


def random_read(rng, L):
    s = bytes(rng.choice(np.frombuffer(b"ACGTacgtNn", dtype=np.uint8), L, p=[.2, .2, .2, .2, .03, .03, .03, .03, .04, .04]).astype(np.uint8))
    if L and rng.random() < 0.4:                                     # a homopolymer tail
        t = int(rng.integers(1, L + 1))
        s = s[:L - t] + bytes([int(rng.choice(np.frombuffer(b"GgNA", dtype=np.uint8)))]) * t
    q = bytes(rng.choice(np.frombuffer(b"!#+5I5", dtype=np.uint8), L).astype(np.uint8))
    return s, q


def brute(s, q, Q, W, P, min_length, max_n, C):
    """Every window summed naively, every suffix tried: the contract read literally, sharing no code with prep_ref."""
    L = len(s)
    b, e, empty = 0, L, False
    if Q > 0 and q is not None:
        p = [max(c - 33, 0) for c in q]
        firsts = [j for j in range(L) if p[j] >= Q]
        if not firsts:
            empty = True
        else:
            b = min(firsts)
            w = min(W, L - b)
            bad = [i for i in range(b, L - w + 1) if sum(p[i + t] for t in range(w)) < Q * w]
            e = min(bad) if bad else L
            lasts = [j for j in range(b, e) if p[j] >= Q]
            if not lasts:
                empty = True
            else:
                e = 1 + max(lasts)
    if P > 0 and not empty and e > b:
        c = s[e - 1] & 0xDF
        r = max(t for t in range(0, e - b + 1) if all((x & 0xDF) == c for x in s[e - t:e]))
        if r >= P:
            e -= r
    if empty or e <= b:
        b = e = 0
    n = e - b
    n_bases = sum(1 for x in s[b:e] if chr(x & 0xDF) not in "ACGT")
    d = len([j for j in range(b, e - 1) if (s[j] & 0xDF) != (s[j + 1] & 0xDF)])
    if n < min_length:
        why = 1
    elif max_n is not None and n_bases > max_n:
        why = 2
    elif C > 0 and 100 * d < C * max(n - 1, 0):
        why = 3
    else:
        why = 0
    return b, n, why


def test_every_step_against_brute_force():
    rng = np.random.default_rng(777)
    seen = set()
    for it in range(400):
        s, q = random_read(rng, int(rng.integers(0, 40)))
        if it % 5 == 0:
            q = None
        Q, W, P = int(rng.choice([0, 2, 10, 20, 41])), int(rng.choice([1, 2, 4, 7, 50])), int(rng.choice([0, 1, 3, 10]))
        ml, mn, C = int(rng.choice([0, 1, 5, 21])), rng.choice([None, 0, 1, 3]), int(rng.choice([0, 30, 60, 100]))
        mn = None if mn is None else int(mn)
        got = prep_ref.prep_read(s, q, trim_quality=Q, trim_window=W, poly_x=P, min_length=ml, max_n=mn, min_complexity=C)
        assert got == brute(s, q, Q, W, P, ml, mn, C), (s, q, Q, W, P, ml, mn, C)
        seen.add(got[2])
        assert got[1] > 0 or got[0] == 0                              # an empty interval is (0, 0)
    assert seen == {0, 1, 2, 3}


def test_pair_rule_and_totals():
    good, short, poly = b"ACGTTGCAACGT", b"ACG", b"AAAAAAAAAAAA"
    reads = [good, good, good, short, short, good, poly, short, good, poly]
    got = prep_ref.prep_block(reads, None, paired=True, min_length=5, min_complexity=30)
    assert got["reason"] == [0, 0, prep_ref.MATE, prep_ref.SHORT, prep_ref.SHORT, prep_ref.MATE, prep_ref.COMPLEXITY, prep_ref.SHORT,
                             prep_ref.MATE, prep_ref.COMPLEXITY]
    assert got["kept"] == [0, 1] and got["kept_reads"] == [good, good]
    assert got["n_reason"] == {"kept": 2, "short": 3, "n": 0, "complexity": 2, "mate": 3}
    assert (got["n_reads"], got["n_kept"], got["bases_in"], got["bases_kept"], got["n_trimmed"]) == (10, 2, sum(map(len, reads)), 24, 0)
    alone = prep_ref.prep_block(reads, None, paired=False, min_length=5, min_complexity=30)
    assert alone["reason"] == [0, 0, 0, 1, 1, 0, 3, 1, 0, 3] and alone["n_kept"] == 5
    quals = [b"I" * 9 + b"###", None] + [None] * 8
    cut = prep_ref.prep_block(reads, quals, paired=True, trim_quality=20, min_length=5, min_complexity=30)
    # (windows 6 and 7 hold 122 and 84 >= 80, window 8 holds 46: cut at 8, whose last good base is 7)
    assert cut["len"][:2] == [8, 12] and cut["n_trimmed"] == 1 and cut["bases_kept"] == 20 and cut["kept_reads"][0] == good[:8]
    parts = [prep_ref.prep_block(reads[a:b], None, paired=True, min_length=5, min_complexity=30) for a, b in ((0, 4), (4, 10))]
    assert prep_ref.add_totals(parts) == {k: got[k] for k in ("n_reads", "n_kept", "bases_in", "bases_kept", "n_trimmed", "n_reason")}
    with pytest.raises(AssertionError):
        prep_ref.prep_block(reads[:3], None, paired=True)


def test_a_read_does_not_depend_on_its_neighbours():
    rng = np.random.default_rng(4242)
    pairs = [random_read(rng, int(rng.integers(0, 60))) for _ in range(120)]
    params = dict(trim_quality=20, trim_window=4, poly_x=3, min_length=8, max_n=2, min_complexity=30)
    alone = [prep_ref.prep_read(s, q, **params) for s, q in pairs]
    order = rng.permutation(len(pairs))
    block = prep_ref.prep_block([pairs[i][0] for i in order], [pairs[i][1] for i in order], **params)
    assert [(block["begin"][j], block["len"][j], block["reason"][j]) for j in range(len(order))] == [alone[i] for i in order]
