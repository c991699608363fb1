"""What a large call must give, worked out from a small reference.

A large call is made of copies of a small base of distinct units (reads, or fragments of two mates): unit u of the call is
base unit idx[u], idx a fixed index array in which every base unit occurs (m = bincount(idx) >= 1).  The plain references
(the oracle's rows, the k-mer by k-mer scores, best_sets, Clades, tax_ref, abund_ref, cover_ref) are run on the base alone,
and every expectation for the call follows from its definition: what is kept per unit is gathered through idx, what is
counted is counted m times, and a maximum does not care how often it saw a value.  Nothing here knows the library, and
nothing loops over the units of the call in Python.  tests/test_tiled_ref_cpu.py checks every builder against the plain
references run on the expanded list of units."""
import numpy as np

import abund_ref

NO = 0xFFFFFFFF
GATHER_CHUNK = 1 << 24                                               # entries gathered at a time (bounds the index arrays)


def tile_index(n_base, n, seed):
    """idx[n] over base units 0 .. n_base - 1, seeded: every unit once, and the rest drawn at random from a random half of
    them (so the other half keeps m = 1), in shuffled order."""
    assert n >= n_base >= 1
    rng = np.random.default_rng(seed)
    heavy = rng.permutation(n_base)[:max(1, n_base // 2)].astype(np.int64)
    idx = np.concatenate([np.arange(n_base, dtype=np.int64), heavy[rng.integers(0, len(heavy), n - n_base)]])
    rng.shuffle(idx)
    return idx


def multiplicity(idx, n_base):
    m = np.bincount(idx, minlength=n_base).astype(np.int64)
    assert len(m) == n_base and int(m.min()) >= 1 and int(m.sum()) == len(idx)
    return m


def csr_of(sets):
    """(offsets u64, leaves u32) of per-unit sets of leaf columns, every row ascending."""
    offs = np.zeros(len(sets) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64)
    return offs, np.array([c for s in sets for c in sorted(s)], dtype=np.uint32)


def gather_rows(offs, values, idx):
    """The ragged gather: rows idx[0], idx[1], ... of the CSR (offs, values), one after the other, as (new offsets u64, new
    values).  `values` may be several aligned arrays (a tuple comes back)."""
    many = isinstance(values, (tuple, list))
    vals = [np.asarray(v) for v in (values if many else (values,))]
    offs = np.asarray(offs).astype(np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    lens = (offs[1:] - offs[:-1])[idx]
    new = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(lens, out=new[1:])
    total = int(new[-1])
    out = [np.empty(total, dtype=v.dtype) for v in vals]
    lo = 0
    while lo < len(idx):                                              # (chunks of entries, not units: one pass for a small call)
        hi = max(lo + 1, int(np.searchsorted(new, new[lo] + GATHER_CHUNK, side="right")) - 1)
        a, b = int(new[lo]), int(new[hi])
        src = np.repeat(offs[idx[lo:hi]] - new[lo:hi], lens[lo:hi]) + np.arange(a, b, dtype=np.int64)
        for o, v in zip(out, vals):
            o[a:b] = v[src]
        lo = hi
    return new.astype(np.uint64), (tuple(out) if many else out[0])


def pack_units(seq, off, idx, per_unit=1):
    """The packed block (sequence bytes with 16 bytes of padding, offsets u64) of the call, from the base's packed block: base
    unit i is reads per_unit * i .. per_unit * i + per_unit - 1 of it (2: the mates of a fragment)."""
    idx = np.asarray(idx, dtype=np.int64)
    reads = (idx[:, None] * per_unit + np.arange(per_unit, dtype=np.int64)[None, :]).reshape(-1)
    new_off, body = gather_rows(off, np.asarray(seq)[:int(off[-1])], reads)
    return np.concatenate([body, np.zeros(16, dtype=np.uint8)]), new_off


def expand(items, idx, per_unit=1):
    """The call's units spelled out as a Python list (for the plain references on a small call)."""
    return [items[int(i) * per_unit + j] for i in idx for j in range(per_unit)]


def per_unit(base_values, idx):
    """A per-unit result (an LCA, a taxon): the base's, through idx."""
    return np.asarray(base_values)[np.asarray(idx, dtype=np.int64)]


def here_below(base_nodes, m, parents):
    """(here, below) over the nodes whose parents are `parents` (a parent comes before its children; the root's is negative):
    here[v] = the units assigned to v — base unit i, m[i] times, to base_nodes[i] (NO: to none) — and below = its subtree sums."""
    base_nodes = np.asarray(base_nodes, dtype=np.int64)
    hit = base_nodes != NO
    here = np.zeros(len(parents), dtype=np.uint64)
    np.add.at(here, base_nodes[hit], np.asarray(m, dtype=np.uint64)[hit])
    below = here.copy()
    for v in range(len(parents) - 1, 0, -1):
        below[parents[v]] += below[v]
    return here, below


def leaf_counts(sets, m, n_leaves):
    """Per leaf the units that list it."""
    out = np.zeros(n_leaves, dtype=np.int64)
    for s, k in zip(sets, m):
        if s:
            out[sorted(s)] += int(k)
    return out


def taxa(nodes, sets, idx, m):
    """(last, here, below, any) as tax_ref.Nodes.counts gives them for the call: every base unit's taxon and touched set
    (nodes.unit), the taxon through idx, the counts m times."""
    base_last = np.array([nodes.unit(s)[0] for s in sets], dtype=np.uint32)
    here, below = here_below(base_last, m, nodes.par)
    any_ = np.zeros(nodes.n, dtype=np.uint64)
    for s, k in zip(sets, m):
        touched = nodes.unit(s)[1]
        if touched:
            any_[np.fromiter(touched, dtype=np.int64)] += np.uint64(k)
    return per_unit(base_last, idx), here, below, any_


def abundance_log(sets, m, n_leaves):
    """abund_ref's log of the call: the base rows, each m times."""
    return abund_ref.classify([sorted(s) for s in sets], n_leaves, mult=m)


def sketch(sketcher, sets, m, reads=None, pairs=None):
    """cover_ref's sketch of the call into `sketcher` (a fresh cover_ref.TreeSketcher): every base unit once for the registers,
    counted m times in units, matched and n_units."""
    rows = [sorted(s) for s in sets]
    return sketcher.add_pairs(rows, pairs, mult=m) if pairs is not None else sketcher.add_reads(rows, reads, mult=m)


class Expect:
    """Everything one call of the units `idx` must give, from the base's references: `sets` (the rows), `scores` (aligned with
    the CSR of `sets`) and `best` (the rows the consumers read: the best-scoring entries, or `sets` again).

    offs / leaves / scores   the call's CSR and scores
    counts                   its leaf counts
    csr                      the CSR of the consumers' rows (last_best_rows)
    lca[kind], clades[kind]  last_lca and (here, below) for kind "all" (over `sets`) and "best" (over `best`); cm: a Clades
    taxa                     (last, here, below, any); nodes: a tax_ref.Nodes
    log, est                 abund_ref's log and its estimate(200, 0)
    sketch                   cover_ref's sketch (sketcher: a fresh TreeSketcher; None: left out)"""

    def __init__(self, idx, sets, scores, best, *, n_leaves, cm=None, nodes=None, sketcher=None, reads=None, pairs=None):
        n_base = len(sets)
        assert len(best) == n_base and n_base == (len(pairs) if pairs is not None else len(reads))
        self.idx = np.asarray(idx, dtype=np.int64)
        self.n = len(self.idx)
        self.m = m = multiplicity(self.idx, n_base)
        offs, leaves = csr_of(sets)
        assert len(scores) == len(leaves)
        self.offs, (self.leaves, self.scores) = gather_rows(offs, (leaves, np.asarray(scores)), self.idx)
        self.counts = leaf_counts(sets, m, n_leaves)
        self.csr = gather_rows(*csr_of(best), self.idx)
        self.lca, self.clades = {}, {}
        if cm is not None:
            for kind, rows in (("all", sets), ("best", best)):
                base = cm.expected(rows)
                self.lca[kind] = per_unit(base, self.idx)
                self.clades[kind] = here_below(base, m, cm.par)
        if nodes is not None:
            self.taxa = taxa(nodes, best, self.idx, m)
        self.log = abundance_log(best, m, n_leaves)
        self.est = abund_ref.estimate(self.log, 200, 0)
        self.sketch = sketch(sketcher, best, m, reads=reads, pairs=pairs) if sketcher is not None else None
