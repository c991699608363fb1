"""pfq_tree_recluster restated over an oracle tree (include/pfq.h "re-clustering"), in exact arithmetic: the scores of the leaf
pairs, the rounds of mutual best pairs under average linkage, the merge log, the new tree and the lines of MERGES.tsv.  Nothing
here knows how the library computes any of it.

Exactness.  q is computed in Python integers unless num * 2^20 fits 64 bits for every pair (nbits below 2^22), where numpy's
unsigned integers give the same.  The order of the rule compares S1 / w1 with S2 / w2 for one row X, where w = |X| |Y|: |X| is
common, so the key of column Y is S / |Y|, kept as the pair (S // |Y|, (S % |Y|) / |Y|).  The first is an exact integer; the
second a correctly rounded quotient of two integers below 2^15 — equal fractions give equal doubles and different ones differ by
at least 2^-30, far above a double's spacing — so comparing the pairs compares the fractions exactly."""
import numpy as np

import sim_ref
from oracle import pfq_oracle as orc

Q = 20
HEADER = "#node\tleft\tright\tleaves\tround\tscore_sum\tpairs\tsimilarity"
MAX_LEAVES = 16384


def q_of(shared, a, b, m):
    """One leaf pair, in Python integers."""
    shared, a, b, m = int(shared), int(a), int(b), int(m)
    u = a + b - shared
    num, den = max(0, shared * m - a * b), u * m - a * b
    return (num << Q) // den if den else 0


def leaf_scores(rows, nbits):
    """q for all pairs of filter rows [L, n_words] of nbits bits: int64 [L, L], symmetric; the diagonal is not used (0)."""
    r = sim_ref.below(rows, nbits)
    shared = sim_ref.shared_bits(r, r).astype(np.uint64)
    pop = sim_ref.popcount(r)
    n = len(r)
    if nbits < (1 << 22):
        m = np.uint64(nbits)
        a, b = pop[:, None], pop[None, :]
        ab, im = a * b, shared * m
        num = np.where(im > ab, im - ab, np.uint64(0))
        den = (a + b - shared) * m - ab
        q = np.where(den > 0, (num << np.uint64(Q)) // np.maximum(den, np.uint64(1)), np.uint64(0)).astype(np.int64)
    else:
        q = np.zeros((n, n), dtype=np.int64)
        for i in range(n):
            for j in range(i + 1, n):
                q[i, j] = q[j, i] = q_of(shared[i, j], pop[i], pop[j], nbits)
    q[np.arange(n), np.arange(n)] = 0
    assert np.array_equal(q, q.T) and q.min(initial=0) >= 0 and q.max(initial=0) <= 1 << Q
    return q


def best_columns(S, sizes):
    """Per row of the live score matrix S (int64, rows and columns in ascending node index) the position of the best other
    column: S / size descending — exactly, see the module text — then the first, which is the smallest node index."""
    n = len(S)
    assert n >= 2 and int(S.max()) < (1 << 46) and int(sizes.max()) < (1 << 15)
    fl = S // sizes[None, :]
    frac = (S - fl * sizes[None, :]) / sizes[None, :]
    fl[np.arange(n), np.arange(n)] = -1
    c1 = fl == fl.max(axis=1)[:, None]
    fr = np.where(c1, frac, -1.0)
    c2 = fr == fr.max(axis=1)[:, None]
    return c2.argmax(axis=1)


def cluster(q):
    """The merge log for the leaf scores q [L, L]: a list of (node, left, right, round, n_leaves, score_sum, pairs), and the
    number of rounds."""
    L = len(q)
    assert 1 <= L <= MAX_LEAVES
    nodes = np.arange(L, dtype=np.int64)                 # live nodes, ascending
    sizes = np.ones(L, dtype=np.int64)
    S = np.array(q, dtype=np.int64, copy=True)
    log, rnd, made = [], 0, L
    while len(nodes) > 1:
        best = best_columns(S, sizes)
        pos = np.arange(len(nodes))
        left = pos[(best[best] == pos) & (pos < best)]   # mutual pairs, by their smaller position = smaller node index, ascending
        assert len(left) >= 1, "a round without a mutual pair"
        right = best[left]
        for a, b in zip(left.tolist(), right.tolist()):
            log.append((made, int(nodes[a]), int(nodes[b]), rnd, int(sizes[a] + sizes[b]), int(S[a, b]), int(sizes[a] * sizes[b])))
            made += 1
        gone = np.zeros(len(nodes), dtype=bool)
        gone[left] = gone[right] = True
        keep = pos[~gone]
        rows = np.concatenate([S[keep], S[left] + S[right]])
        S = np.concatenate([rows[:, keep], rows[:, left] + rows[:, right]], axis=1)
        sizes = np.concatenate([sizes[keep], sizes[left] + sizes[right]])
        nodes = np.concatenate([nodes[keep], np.arange(made - len(left), made, dtype=np.int64)])
        rnd += 1
    return log, rnd


def log_of(ot):
    """(merge log, rounds) of an oracle tree's current leaves."""
    return cluster(leaf_scores(sim_ref.leaf_rows(ot), ot.nbits))


def leaf_sets(log, n_leaves):
    """Per node of the log's numbering the frozenset of leaves (0 .. n_leaves - 1) below it."""
    sets = [frozenset([i]) for i in range(n_leaves)]
    for node, left, right, *_ in log:
        assert node == len(sets)
        sets.append(sets[left] | sets[right])
    return sets


def height(log, n_leaves):
    """Edges from the root to the deepest leaf."""
    h = [0] * n_leaves
    for _, left, right, *_ in log:
        h.append(1 + max(h[left], h[right]))
    return h[-1]


def recluster(ot):
    """(new oracle tree, merge log, rounds, names): the tree pfq_tree_recluster makes of `ot`, nodes in pre-order; names[n] is
    the name of node n of the log's numbering."""
    leaves = ot.leaves_dfs()
    L = len(leaves)
    assert L >= 1 and len({ot.bf_path[v] for v in leaves}) == L
    log, rounds = log_of(ot)
    t = orc.OracleTree(ot.kmer_size, ot.nbits, ot.num_hashes, ot.seed1, ot.seed2, ot.false_pos_rate, ot.largest_expected_genome)
    t.bits = np.zeros((2 * L - 1, ot.n_words), dtype=np.uint64)
    for i, v in enumerate(leaves):
        t.add_node(ot.tax_id[v], ot.bf_path[v], i)
        t.bits[i] = ot.bits[ot.filter_of[v]]
    n = 0
    for node, left, right, *_ in log:
        while f"Internal_Node_{n}.bf" in t.bf_path:
            n += 1
        assert t.add_node(f"Internal_Node_{n}", f"Internal_Node_{n}.bf", node, left, right) == node
        n += 1
        t.bits[node] = t.bits[left] | t.bits[right]
    names = list(t.tax_id)
    t.root = 2 * L - 2
    orc.renumber_preorder(t)
    return t, log, rounds, names


def clade_table(ot):
    """tree.clades() over an oracle tree: (parent, depth, first_leaf, n_leaves, name) per reachable node in pre-order."""
    out, st, col = [], [(ot.root, -1, 0)] if ot.root >= 0 else [], 0
    while st:
        v, p, d = st.pop()
        c = len(out)
        out.append([p, d, col, 0, ot.tax_id[v] if ot.tax_id[v] is not None else ot.bf_path[v][:-len(".bf")]])
        if ot.is_leaf(v):
            col += 1
            a = c
            while a >= 0:
                out[a][3] += 1
                a = out[a][0]
        else:
            if ot.right[v] >= 0:
                st.append((ot.right[v], c, d + 1))
            if ot.left[v] >= 0:
                st.append((ot.left[v], c, d + 1))
    return [tuple(r) for r in out]


def same_log(got, log, rounds, got_rounds, tag=None):
    """tree.merges() (the structured array) against a log of this module."""
    assert got_rounds == rounds, (tag, got_rounds, rounds)
    have = [(int(g["node"]), int(g["left"]), int(g["right"]), int(g["round"]), int(g["n_leaves"]), int(g["score_sum"]), int(g["pairs"])) for g in got]
    assert len(have) == len(log), (tag, len(have), len(log))
    for i, (h, w) in enumerate(zip(have, log)):
        assert h == w, (tag, i, h, w)


def merges_tsv(log, names):
    """MERGES.tsv: the header and one line per internal node in creation order."""
    lines = [HEADER]
    for node, left, right, rnd, n_leaves, score, pairs in log:
        lines.append("\t".join([names[node], names[left], names[right], str(n_leaves), str(rnd), str(score), str(pairs),
                                f"{score / (pairs * (1 << Q)):.6f}"]))
    return "\n".join(lines) + "\n"
