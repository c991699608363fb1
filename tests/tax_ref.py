"""The taxonomy model (include/pfq.h "taxonomy", DESIGN.md §5 "Taxonomy") in plain Python: the file grammar, the node numbering,
taxon(unit) by walking parents until the set meets, and `any` as the union of the ancestor sets.  Nothing here comes from the
library.

A taxonomy of a tree with L current leaves is given as n_taxa >= 1 taxa.
  - Taxon 0 is the root, with parent PFQ_NO_CLADE.
  - taxon_parent[i] < i for i > 0.
  - Every taxon has a name.
  - leaf_taxon[l] < n_taxa is the taxon that genome l sits directly under.
  - l is a leaf index in pfq_leaf_counts order.
The library derives the nodes:
  - Every genome is a node of its own, under its taxon.
  - A taxon with no genome anywhere below it is dropped.  The root is kept.
  - Nodes are numbered in pre-order: first a taxon, then the genomes directly under it in ascending leaf index, then its
    remaining child taxa in ascending input index, each with its subtree.
  - rank[l] is the position of genome l among the genomes in that order (0 .. L - 1).  So every node covers a contiguous
    range of ranks.
A unit is a read, or with PFQ_PAIRED a fragment.  Its hit set H is exactly the row pfq_hits gives for it in that call; nothing
is decided again.  With PFQ_WANT_HITS an all-leaf unit's row lists all L leaves.  Per unit with H non-empty:
  - taxon(unit) is the deepest node that is an ancestor-or-self of every genome of H.  With H empty it is PFQ_NO_CLADE.
  - here[taxon(unit)] += 1.
  - any[t] += 1 for every node t that is an ancestor-or-self of at least one genome of H, once per unit however many genomes
    of H lie below t.
  - below[t] is the sum of here over t's subtree.
Consequences: a call's increase of any[genome node of l] equals the increase of leaf counter l; any[root] = below[root] is the
number of units that hit anything; any[t] >= below[t] for every t.

The file: lines end with '\\n', a trailing '\\r' is dropped; empty lines and lines beginning with '#' are skipped.  A line is
genome<TAB>lineage[<TAB>ignored...]; fewer than two fields is an error that names the line.  lineage is a ';'-separated list of
names from the top rank down, each trimmed of spaces; an empty lineage means directly under the root, an empty name inside a
non-empty lineage is an error.  A taxon is identified by its whole path.  Only lines whose genome equals the tax_id of a leaf are
considered, and every leaf with that tax_id gets the lineage; two considered lines for one genome with different lineages is an
error.  Taxon indices are assigned in order of first appearance over the considered lines, prefixes left to right; the root is
taxon 0, named "root".  Leaves without a line sit under the root."""
import numpy as np

NO = 0xFFFFFFFF


class TaxFileError(Exception):
    def __init__(self, line, msg):
        super().__init__(f"line {line}: {msg}")
        self.line = line


def parse(data: bytes, leaf_ids):
    """(taxon_parent, taxon_names, leaf_taxon, info) of the file's bytes for leaves named leaf_ids; the root's parent is -1.
    info: lines_considered, lines_other, leaves_without_line."""
    text = data.decode()
    parent, names, index = [-1], ["root"], {}
    leaf_taxon = [None] * len(leaf_ids)
    considered = other = 0
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for no, line in enumerate(lines, 1):
        if line.endswith("\r"):
            line = line[:-1]
        if line == "" or line.startswith("#"):
            continue
        fields = line.split("\t")
        if len(fields) < 2:
            raise TaxFileError(no, "fewer than two fields")
        genome, lineage = fields[0], fields[1].strip(" ")
        path = [x.strip(" ") for x in lineage.split(";")] if lineage else []
        if any(x == "" for x in path):
            raise TaxFileError(no, "empty name")
        if genome not in leaf_ids:
            other += 1
            continue
        considered += 1
        cur = ()
        for x in path:
            cur = cur + (x,)
            if cur not in index:
                index[cur] = len(parent)
                parent.append(index[cur[:-1]] if len(cur) > 1 else 0)
                names.append(x)
        t = index[cur] if cur else 0
        for l, i in enumerate(leaf_ids):
            if i == genome:
                if leaf_taxon[l] is not None and leaf_taxon[l] != t:
                    raise TaxFileError(no, "two lineages for one genome")
                leaf_taxon[l] = t
    missing = sum(1 for t in leaf_taxon if t is None)
    info = {"lines_considered": considered, "lines_other": other, "leaves_without_line": missing}
    return parent, names, [0 if t is None else t for t in leaf_taxon], info


class Nodes:
    """The node table of a taxonomy over leaves named leaf_ids: table[v] = (parent, depth, first_rank, n_leaves, leaf, name) with
    parent -1 for the root and leaf -1 for a taxon; rank[l], leaf_node[l]."""

    def __init__(self, leaf_ids, taxon_parent, taxon_names, leaf_taxon):
        n_taxa, L = len(taxon_parent), len(leaf_ids)
        assert n_taxa >= 1 and taxon_parent[0] in (-1, NO) and all(0 <= taxon_parent[i] < i for i in range(1, n_taxa))
        assert len(leaf_taxon) == L and all(0 <= t < n_taxa for t in leaf_taxon)
        kids = [[] for _ in range(n_taxa)]
        for i in range(1, n_taxa):
            kids[taxon_parent[i]].append(i)
        genomes = [[] for _ in range(n_taxa)]
        for l, t in enumerate(leaf_taxon):
            genomes[t].append(l)
        alive = [False] * n_taxa                      # a genome anywhere below
        for i in range(n_taxa - 1, -1, -1):
            alive[i] = bool(genomes[i]) or any(alive[c] for c in kids[i])
        self.table, self.rank, self.leaf_node = [], [0] * L, [0] * L
        st = [(0, -1, 0)]
        while st:
            i, p, d = st.pop()
            v = len(self.table)
            self.table.append([p, d, None, 0, -1, taxon_names[i]])
            for l in genomes[i]:
                self.leaf_node[l] = len(self.table)
                self.table.append([v, d + 1, None, 0, l, leaf_ids[l]])
            st += [(c, v, d + 1) for c in reversed(kids[i]) if alive[c]]
        self.par = [r[0] for r in self.table]
        order = [r[4] for r in self.table if r[4] >= 0]          # genomes in node order
        for pos, l in enumerate(order):
            self.rank[l] = pos
        for l in range(L):                                        # every ancestor-or-self of a genome holds its rank
            v = self.leaf_node[l]
            while v >= 0:
                r = self.table[v]
                r[2] = self.rank[l] if r[2] is None else min(r[2], self.rank[l])
                r[3] += 1
                v = self.par[v]
        for r in self.table:                                      # (only a root without genomes is left without a rank)
            if r[2] is None:
                r[2] = 0
        self.table = [tuple(r) for r in self.table]
        self.n = len(self.table)
        self._anc = {}
        self._memo = {}

    def ancestors(self, v):
        """v and everything above it, v first."""
        if v not in self._anc:
            out, t = [], v
            while t >= 0:
                out.append(t)
                t = self.par[t]
            self._anc[v] = out
        return self._anc[v]

    def unit(self, s):
        """(taxon(unit), the set of touched nodes) of the hit set s (leaf indices)."""
        key = frozenset(s)
        if key not in self._memo:
            if not key:
                self._memo[key] = (NO, frozenset())
            else:
                chains = [self.ancestors(self.leaf_node[l]) for l in key]
                touched = frozenset(v for c in chains for v in c)
                common = set(chains[0])
                for c in chains[1:]:
                    common &= set(c)
                # walking up from any genome of the set, the first node all of them share
                taxon = next(v for v in chains[0] if v in common)
                self._memo[key] = (taxon, touched)
        return self._memo[key]

    def counts(self, sets):
        """(last, here, below, any) of the units with hit sets `sets`."""
        last = np.full(len(sets), NO, dtype=np.uint32)
        here, any_ = np.zeros(self.n, dtype=np.uint64), np.zeros(self.n, dtype=np.uint64)
        times = {}
        for u, s in enumerate(sets):
            key = frozenset(s)
            last[u] = self.unit(key)[0]
            times[key] = times.get(key, 0) + 1
        for key, m in times.items():                              # equal sets count alike: once per distinct set, times m
            t, touched = self.unit(key)
            if t != NO:
                here[t] += np.uint64(m)
                any_[np.fromiter(touched, dtype=np.int64)] += np.uint64(m)
        below = here.copy()
        for v in range(self.n - 1, 0, -1):
            below[self.par[v]] += below[v]
        return last, here, below, any_
