"""PFQ_WANT_COVERAGE restated in plain Python ints (include/pfq.h "coverage"): per leaf the units that list it, their matched
k-mers and a HyperLogLog sketch of them, over the oracle's get_kmers / seeded_hash / bf_contains; and the host-side estimator.
Nothing here knows how the library computes any of it."""
import math

from oracle import pfq_oracle as orc

M64 = (1 << 64) - 1
P_MIN, P_MAX, P_DEFAULT = 4, 16, 12


def mix(x):
    """The splitmix64 finaliser."""
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def clz64(w):
    return 64 - w.bit_length()


def slot(u, p):
    """(register index, rho) of the mixed hash u at precision p."""
    j = u >> (64 - p)
    w = (u << p) & M64
    return j, min(clz64(w), 64 - p) + 1


class Sketch:
    def __init__(self, n_leaves, p=P_DEFAULT):
        assert P_MIN <= p <= P_MAX
        self.n_leaves, self.p, self.n_units = n_leaves, p, 0
        self.registers = [[0] * (1 << p) for _ in range(n_leaves)]
        self.units = [0] * n_leaves
        self.matched = [0] * n_leaves

    def add_hash(self, leaf, h, mult=1):
        """One matched k-mer of `leaf` whose seeded hash is h (`mult`: met that many times; the maximum does not care)."""
        j, rho = slot(mix(h), self.p)
        self.matched[leaf] += mult
        if rho > self.registers[leaf][j]:
            self.registers[leaf][j] = rho

    def absorb(self, other):
        assert (self.n_leaves, self.p) == (other.n_leaves, other.p)
        for l in range(self.n_leaves):
            self.registers[l] = [max(a, b) for a, b in zip(self.registers[l], other.registers[l])]
            self.units[l] += other.units[l]
            self.matched[l] += other.matched[l]
        self.n_units += other.n_units

    def distinct(self):
        return [estimate(r, self.p) for r in self.registers]


class TreeSketcher:
    """Sketches units against an oracle tree: `add(row, reads)` is one unit whose row (leaf columns) the query gave and whose
    reads are one read, or the two mates of a fragment; with `mult`, that many equal units."""

    def __init__(self, ot, p=P_DEFAULT, share=None):
        self.ot = ot
        self.rows = [ot.filter_of[v] for v in ot.leaves_dfs()]
        self.sk = Sketch(len(self.rows), p)
        # the oracle's answers per k-mer, kept (`share`: another sketcher of the same tree whose answers are reused)
        self._hash, self._in = (share._hash, share._in) if share is not None else ({}, {})

    def add(self, row, reads, mult=1):
        sk, ot = self.sk, self.ot
        sk.n_units += mult
        for l in row:
            sk.units[l] += mult
            for x in reads:
                for c in orc.get_kmers(x, ot.kmer_size):                     # canonical, duplicates included
                    key = (l, c)
                    if key not in self._in:
                        self._in[key] = orc.bf_contains(ot, self.rows[l], c)
                    if self._in[key]:
                        if c not in self._hash:
                            self._hash[c] = orc.seeded_hash(ot.seed1, c)
                        sk.add_hash(l, self._hash[c], mult)
        return self

    def add_reads(self, rows, reads, mult=None):
        for i, (row, x) in enumerate(zip(rows, reads)):
            self.add(row, [x], 1 if mult is None else int(mult[i]))
        return self

    def add_pairs(self, rows, pairs, mult=None):
        for i, (row, (a, b)) in enumerate(zip(rows, pairs)):
            self.add(row, [a, b], 1 if mult is None else int(mult[i]))
        return self

    def filter_bits(self):
        return [sum(int(w).bit_count() for w in self.ot.bits[r]) for r in self.rows]

    def genome_kmers(self):
        return [genome_kmers(self.ot.nbits, self.ot.num_hashes, b) for b in self.filter_bits()]


def alpha(p):
    m = 1 << p
    return {4: 0.673, 5: 0.697, 6: 0.709}.get(p, 0.7213 / (1.0 + 1.079 / m))


def estimate(reg, p):
    """Classic HyperLogLog without a large-range correction; an all-zero sketch gives 0."""
    m = 1 << p
    assert len(reg) == m
    zeros = sum(1 for r in reg if r == 0)
    if zeros == m:
        return 0.0
    e = alpha(p) * m * m / sum(math.ldexp(1.0, -r) for r in reg)
    return m * math.log(m / zeros) if e <= 2.5 * m and zeros > 0 else e


def genome_kmers(nbits, num_hashes, filter_bits):
    """Swamidass-Baldi: the distinct items behind filter_bits set bits; a full filter is not estimable (0.0)."""
    if filter_bits >= nbits:
        return 0.0
    return -(nbits / num_hashes) * math.log1p(-filter_bits / nbits)
