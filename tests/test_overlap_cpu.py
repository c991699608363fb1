"""tests/overlap_ref.py against the rule of pfq.h "mate overlap" written out once more, literally, and against its own edge
cases: planted inserts over the whole range, nothing outside it, poly-A mates, and the equality with adapter_ref.prep_block on
hand-cut reads."""
import numpy as np

import adapter_ref
import overlap_ref
import prep_ref

NO = overlap_ref.NO_INSERT
AD33 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def dna(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), n).astype(np.uint8))


def revcomp(s):
    return s.translate(COMPLEMENT)[::-1]


def fragment(rng, I, L1, L2):
    """Mates of L1 and L2 bases of an insert of I random bases, each followed by random bases of its own."""
    ins = dna(rng, I)
    return (ins + dna(rng, L1))[:L1], (revcomp(ins) + dna(rng, L2))[:L2]


def brute(a, b, O, E):
    """Every I, every pair (i, j), as the definitions read."""
    comp = {"A": "T", "T": "A", "C": "G", "G": "C"}
    best = (NO, 0)
    for I in range(0, len(a) + len(b) + 2):
        pairs = [(i, I - 1 - i) for i in range(len(a)) if 0 <= I - 1 - i < len(b)]
        mm = 0
        for i, j in pairs:
            p, q = chr(a[i] & 0xDF), chr(b[j] & 0xDF)
            if p not in comp or q not in comp or p != comp[q]:
                mm += 1
        if O <= I <= len(a) + len(b) - O and len(pairs) >= O and 100 * mm <= E * len(pairs):
            best = (I, mm)
    return best


def test_against_the_brute_force():
    rng = np.random.default_rng(5)
    found = 0
    for n in range(400):
        L1, L2 = (int(v) for v in rng.integers(0, 24, 2))
        letters = (b"ACGT", b"AC", b"ACGTNacgtn", b"A")[n % 4]          # few letters: many hypotheses match
        a, b = dna(rng, L1, letters), dna(rng, L2, letters)
        if n % 3 == 0 and L1 and L2:
            a, b = fragment(rng, int(rng.integers(0, L1 + L2 + 1)), L1, L2)
        for O, E in ((1, 0), (3, 10), (5, 34), (8, 50)):
            got = overlap_ref.find_insert(a, b, O, E)
            assert got == brute(a, b, O, E), (a, b, O, E)
            found += got[0] != NO
    assert 300 < found < 1500


def test_a_planted_insert_is_recovered_over_the_whole_range():
    rng = np.random.default_rng(6)
    # (O of 12 and more: a longer insert matches random bases by chance once in 4^12 hypotheses)
    for L1, L2, O in ((40, 40, 12), (50, 31, 12), (31, 50, 12), (33, 33, 16), (64, 20, 20)):
        for I in range(0, L1 + L2 + 3):
            a, b = fragment(rng, I, L1, L2)
            got = overlap_ref.find_insert(a, b, O, 0)
            o = min(I, L1) - max(0, I - L2)
            if O <= I <= L1 + L2 - O and o >= O:
                assert got == (I, 0), (L1, L2, O, I)
                cut = overlap_ref.fragment(a, b, O, 0)
                assert cut == (True, I, 0, min(L1, I), min(L2, I))
            else:                                                     # outside the range random mates match nowhere
                assert got == (NO, 0), (L1, L2, O, I, got)


def test_poly_a_mates_get_the_longest_insert_and_no_cut():
    for L1, L2, O in ((150, 150, 30), (100, 151, 30), (20, 20, 1)):
        a, b = b"A" * L1, b"T" * L2
        assert overlap_ref.fragment(a, b, O, 10) == (True, L1 + L2 - O, 0, L1, L2)
    unit = b"ACGGTCATTG"                                              # a tandem repeat matches every 10 bases: the largest wins
    a = unit * 6
    assert overlap_ref.find_insert(a, revcomp(a), 30, 0) == (90, 0)
    assert overlap_ref.fragment(b"A" * 513, b"T" * 100, 30, 10) == (False, NO, 0, 513, 100)


def test_equal_to_the_adapter_reference_on_hand_cut_reads():
    rng = np.random.default_rng(7)
    reads, quals = [], []
    for n in range(60):
        L1, L2 = (int(v) for v in rng.integers(20, 90, 2))
        I = int(rng.integers(0, 140))
        a, b = fragment(rng, I, L1, L2)
        if n % 4 == 0 and I < L1:
            a = (a[:I] + AD33 + dna(rng, L1))[:L1]                    # the adapter step sees the same read-through
        if n % 5 == 0:
            a = (a[:7] + AD33 + dna(rng, L1))[:L1]                    # ... or an adapter in front of the insert's end
        reads += [a, b]
        quals += [bytes(rng.choice(np.frombuffer(b"#5I", dtype=np.uint8), len(s), p=[.1, .2, .7]).astype(np.uint8)) for s in (a, b)]
    params = dict(trim_quality=20, trim_window=4, poly_x=8, min_length=15, max_n=2, min_complexity=20)
    keys = ("n_reads", "n_kept", "bases_kept", "n_reason", "begin", "len", "reason", "kept", "kept_reads")
    for sets in ((), ([AD33],)):
        got = overlap_ref.prep_block(reads, quals, 12, 10, *sets, **params)
        cut_reads = [s[:c] for s, c in zip(reads, got["cut"])]
        cut_quals = [q[:c] for q, c in zip(quals, got["cut"])]
        assert cut_reads == got["cut_reads"]
        want = adapter_ref.prep_block(cut_reads, cut_quals, [], paired=True, **params)
        assert want["n_found"] == 0
        for k in keys:
            assert got[k] == want[k], k
        assert got["bases_in"] == sum(map(len, reads)) and got["n_trimmed"] == sum(1 for i in got["kept"] if got["len"][i] < len(reads[i]))
        assert got["n_trimmed"] > want["n_trimmed"]
        assert got["reads_cut"] == sum(1 for s, c in zip(reads, got["ocut"]) if c < len(s)) > 20
        assert got["bases_cut"] == sum(len(s) - c for s, c in zip(reads, got["ocut"]))
        assert sum(got["hist"]) == got["n_overlapped"] == sum(1 for i in got["insert"] if i != NO) and got["n_skipped"] == 0
        if sets:
            ad = got["adapters"]
            assert ad["cut"] == adapter_ref.prep_block(reads, None, [AD33], paired=True)["cut"]
            assert any(c < o for c, o in zip(ad["cut"], got["ocut"])) and any(c > o for c, o in zip(ad["cut"], got["ocut"]))
            assert got["cut"] == [min(c, o) for c, o in zip(ad["cut"], got["ocut"])]
        else:
            assert got["adapters"] is None and got["cut"] == got["ocut"]
