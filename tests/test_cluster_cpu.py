"""CPU only: tests/cluster_ref.py itself, the restatement of pfq_tree_recluster's rule (include/pfq.h "re-clustering") — the
scores and the merge log of hand-made filters worked out by hand, its vectorised order against plain fractions on matrices full
of ties, and what the rule makes of strain families put into the oracle's filters."""
import math
from fractions import Fraction

import numpy as np

import cluster_ref as cr
import sim_ref
from oracle import pfq_oracle as orc
from test_sim_cpu import strain_families, tree_of


def bits(*idx):
    return sum(1 << i for i in idx)


def test_hand_made_filters():
    # m = 64.  f0 = f1 = bits 0..7, f2 = bits 4..11, f3 = bits 32..39: A = B = 8 everywhere, A B = 64.
    #   (f0, f1): I = 8, U = 8:  num = 8 * 64 - 64 = 448 = den                          -> q = 2^20
    #   (f0, f2), (f1, f2): I = 4, U = 12: num = 256 - 64 = 192, den = 768 - 64 = 704   -> q = floor(192 * 2^20 / 704) = floor(3 * 2^20 / 11) = 285975
    #   (.., f3): I = 0: num = max(0, -64) = 0                                          -> q = 0
    rows = np.array([[bits(*range(8))], [bits(*range(8))], [bits(*range(4, 12))], [bits(*range(32, 40))]], dtype=np.uint64)
    q = cr.leaf_scores(rows, 64)
    assert 3 * (1 << 20) // 11 == 285975
    assert q.tolist() == [[0, 1 << 20, 285975, 0], [1 << 20, 0, 285975, 0], [285975, 285975, 0, 0], [0, 0, 0, 0]]
    # round 0: best(0) = 1, best(1) = 0, best(2) = 0 (0 and 1 tie: the smaller index), best(3) = 0 (all zero: the smallest index):
    #          only (0, 1) is mutual -> node 4.
    # round 1: S(4, 2) = 571950 over 2 pairs, S(4, 3) = S(2, 3) = 0: best(4) = 2, best(2) = 4, best(3) = 2 -> (2, 4) -> node 5
    # round 2: (3, 5) -> node 6, the root
    log, rounds = cr.cluster(q)
    assert rounds == 3
    assert log == [(4, 0, 1, 0, 2, 1 << 20, 1), (5, 2, 4, 1, 3, 571950, 2), (6, 3, 5, 2, 4, 0, 3)]
    assert cr.height(log, 4) == 3 and cr.leaf_sets(log, 4)[5] == frozenset([0, 1, 2])
    assert cr.merges_tsv(log, ["a", "b", "c", "d", "I0", "I1", "I2"]) == (
        cr.HEADER + "\nI0\ta\tb\t2\t0\t1048576\t1\t1.000000\nI1\tc\tI0\t3\t1\t571950\t2\t0.272727\nI2\td\tI1\t4\t2\t0\t3\t0.000000\n")


def test_scores_at_the_edges():
    # empty filters: den = 0 -> 0; an empty one against a full one: I = 0, A B = 0, num = 0; two full ones: U m - A B = 0 -> 0
    assert cr.q_of(0, 0, 0, 64) == 0 and cr.q_of(0, 0, 64, 64) == 0 and cr.q_of(64, 64, 64, 64) == 0
    # below the chance overlap: clamped to 0
    assert cr.q_of(1, 32, 32, 64) == 0 and cr.q_of(16, 32, 32, 64) == 0 and cr.q_of(17, 32, 32, 64) == (64 << 20) // (47 * 64 - 1024)
    # nbits 70: the padding above bit 69 does not count; the two ways of computing q agree
    rows = np.array([[0b1011, 0b100001 | (1 << 63)], [0b0011, 0b100000 | (1 << 6)], [0, 1 << 40]], dtype=np.uint64)
    q = cr.leaf_scores(rows, 70)
    assert q[0, 1] == cr.q_of(3, 5, 3, 70) == ((3 * 70 - 15) << 20) // (5 * 70 - 15) and q[0, 2] == 0 and q[2, 1] == 0
    # a filter size at which num * 2^20 does not fit 64 bits: Python integers
    big = (1 << 31) + 11
    assert cr.q_of(1 << 20, 1 << 21, 1 << 21, big) == (((1 << 20) * big - (1 << 42)) << 20) // (3 * (1 << 20) * big - (1 << 42))


def brute_force(q):
    """The rule with fractions and loops."""
    L = len(q)
    S = {(i, j): int(q[i][j]) for i in range(L) for j in range(L) if i != j}
    size = {i: 1 for i in range(L)}
    live, log, rnd, made = list(range(L)), [], 0, L
    while len(live) > 1:
        best = {}
        for i in live:
            best[i] = min((j for j in live if j != i), key=lambda j: (-Fraction(S[i, j], size[i] * size[j]), j))
        pairs = [(i, best[i]) for i in live if best[best[i]] == i and i < best[i]]
        assert pairs
        for i, j in pairs:
            log.append((made, i, j, rnd, size[i] + size[j], S[i, j], size[i] * size[j]))
            made += 1
        for k, (i, j) in enumerate(pairs):
            z = made - len(pairs) + k
            others = [w for w in live if w not in (i, j)]
            for w in others:
                S[z, w] = S[w, z] = S[i, w] + S[j, w]
            for w in (i, j):
                live.remove(w)
            live.append(z)
            size[z] = size[i] + size[j]
        rnd += 1
    return log, rnd


def test_ties_every_round_has_a_mutual_pair():
    rng = np.random.default_rng(20)
    for case in range(1000):
        L = int(rng.integers(2, 10))
        top = (1, 2, 3, 1 << 20)[case % 4]
        q = rng.integers(0, top + 1, (L, L))
        if case % 4 == 3:
            q = (q >> 18) << 18                                              # few distinct large values
        q = np.triu(q, 1)
        q = q + q.T
        log, rounds = cr.cluster(q)                                          # (asserts a mutual pair in every round)
        assert len(log) == L - 1 and log[-1][0] == 2 * L - 2 and log[-1][4] == L and 1 <= rounds <= L - 1
        assert (log, rounds) == cr.cluster(q.copy())
        assert (log, rounds) == brute_force(q.tolist()), (case, q.tolist())


def test_strain_families_become_clades():
    rng = np.random.default_rng(2718)
    ot = tree_of(strain_families(rng, 10, 3, 2000, 0.006, 100))
    L = 130
    nt, log, rounds, names = cr.recluster(ot)
    sets = cr.leaf_sets(log, L)
    for f in range(10):
        assert frozenset(range(3 * f, 3 * f + 3)) in sets, f
    assert cr.height(log, L) < 2 * math.ceil(math.log2(L)) + 8, (cr.height(log, L), rounds)
    assert rounds < L // 2
    # the new tree: the same leaves with the same words, every internal filter the OR of its children, names unique
    old = {ot.tax_id[v]: ot.bits[ot.filter_of[v]] for v in ot.leaves_dfs()}
    new_leaves = nt.leaves_dfs()
    assert nt.n_nodes == 2 * L - 1 and sorted(nt.tax_id[v] for v in new_leaves) == sorted(old)
    assert all(np.array_equal(nt.bits[nt.filter_of[v]], old[nt.tax_id[v]]) for v in new_leaves)
    for v in range(nt.n_nodes):
        if not nt.is_leaf(v):
            assert np.array_equal(nt.bits[nt.filter_of[v]], nt.bits[nt.filter_of[nt.left[v]]] | nt.bits[nt.filter_of[nt.right[v]]])
    assert len(set(nt.bf_path)) == nt.n_nodes and names[L] == "Internal_Node_0" and names[:L] == [ot.tax_id[v] for v in ot.leaves_dfs()]
    table = cr.clade_table(nt)
    assert table[0][:4] == (-1, 0, 0, L) and len(table) == 2 * L - 1
    # a leaf called like an internal node: the running number skips it
    ot2 = tree_of([b"ACGT" * 100, b"ACGT" * 100, b"GATTACA" * 60])
    ot2.tax_id[ot2.leaves_dfs()[2]] = "Internal_Node_0"
    ot2.bf_path[ot2.leaves_dfs()[2]] = "Internal_Node_0.bf"
    _, log2, _, names2 = cr.recluster(ot2)
    assert names2[3:] == ["Internal_Node_1", "Internal_Node_2"] and log2[0][:3] == (3, 0, 1)


def test_one_and_two_leaves():
    assert cr.cluster(np.zeros((1, 1), dtype=np.int64)) == ([], 0)
    assert cr.cluster(np.array([[0, 7], [7, 0]])) == ([(2, 0, 1, 0, 2, 7, 1)], 1)
    t, log, rounds, names = cr.recluster(tree_of([b"ACGTTGCA" * 30]))
    assert t.n_nodes == 1 and t.root == 0 and log == [] and rounds == 0 and names == ["G000"]
