"""CPU only, the oracle only: why one pass at the lowest threshold answers every threshold of a list (include/pfq.h "threshold
sweep"), why a tree whose parents are not supersets of their children must be refused, tests/sweep_ref.py against brute-force
counts, and what makes the reads of tests/test_gpu_sweep.py a test of every bin.

The rows are the oracle's (oracle_sets), the scores its bf_contains counts (expected_scores), the needs orc.need.  A unit's
row at thr[t] is derived from its row and scores at the base threshold, {l : score(l) >= need(thr[t], n)}, and compared with
the oracle's row at thr[t] for every read and every threshold; no case is left out."""
import numpy as np
import pytest

import sweep_ref
from oracle import pfq_oracle as orc
from test_gpu_best import ProbeContains
from test_gpu_build import SEEDS, _dna, _mutate
from test_gpu_lca import K, W, csr_of, oracle_sets
from test_gpu_parity import oracle_tree
from test_gpu_scores import expected_scores

LIST = (0.3, 0.5, 0.7, 0.9, 1.0)       # the list of the W tests; its lowest value is the base threshold of the one pass
N_NOISY = 600
SMALL_BASES = (0.0, 0.1, 0.3)
SMALL_LIST = (0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0, 1.5)


def noisy_reads(w, n=N_NOISY):
    """Reads of 150 bases cut from W's genomes with 4 + i % 20 substitutions: most pass 0.3 on some genome and few pass 0.7, so
    their tops fill the low bins that W's own reads (one to three substitutions, or foreign) leave empty."""
    rng = np.random.default_rng(4242)
    out = []
    for i in range(n):
        g = w.genomes[int(rng.integers(0, len(w.genomes)))]
        o = int(rng.integers(0, len(g) - 150 + 1))
        r = _mutate(rng, g[o:o + 150], 4 + i % 20)
        out.append(orc.revcomp(r) if i % 2 else r)
    return out


class SweepW:
    """Workload W plus the noisy reads, with the oracle's rows and scores at the base threshold and the reference state over
    LIST, each computed once and left unchanged.  device: W's library tree is built as well."""

    def __init__(self, device=False):
        self.w = W(device=device)
        self.ot, self.gt = self.w.ot, self.w.gt
        self.n_leaves = len(self.w.genomes)
        self.reads = self.w.reads + noisy_reads(self.w)
        self.lengths = [len(r) for r in self.reads]
        self.probe = ProbeContains(self.ot, self.reads)
        self._sets, self._scores, self._ref = {}, {}, {}

    def sets(self, thr):
        if thr not in self._sets:
            n = len(self.w.reads)
            self._sets[thr] = self.w.sets(thr) + oracle_sets(self.ot, self.reads[n:], thr)
        return self._sets[thr]

    def scores(self, thr):
        if thr not in self._scores:
            offs, leaves = csr_of(self.sets(thr))
            self._scores[thr] = expected_scores(self.ot, self.reads, offs, leaves, self.probe)
        return self._scores[thr]

    def rows(self, thr):
        return [sorted(s) for s in self.sets(thr)]

    def ref(self, thresholds=LIST, base=None, mult=None):
        base = thresholds[0] if base is None else base
        key = (tuple(thresholds), base)
        if mult is not None:
            return sweep_ref.sweep(self.rows(base), self.scores(base), self.lengths, K, thresholds, self.n_leaves, mult=mult)
        if key not in self._ref:
            self._ref[key] = sweep_ref.sweep(self.rows(base), self.scores(base), self.lengths, K, thresholds, self.n_leaves)
        return self._ref[key]


@pytest.fixture(scope="module")
def sw():
    return SweepW()


def small_genomes(rng):
    """20 genomes: families of 4 at 1 %, 3 % and 8 % divergence from their base, and 8 unrelated ones."""
    out = []
    for rate in (0.01, 0.03, 0.08):
        base = _dna(rng, 1200)
        out += [_mutate(rng, base, rng.binomial(1200, rate)) for _ in range(4)]
    out += [_dna(rng, 1200) for _ in range(8)]
    return [out[i] for i in rng.permutation(len(out))]


def small_reads(rng, genomes, n=650):
    """Reads of 15 to 160 bases with up to 6 % substitutions, some foreign; then the empty read and reads of k - 1 and k bases."""
    out = []
    for i in range(n):
        length = int(rng.integers(15, 161))
        if i % 9 == 0:
            out.append(_dna(rng, length))
            continue
        g = genomes[int(rng.integers(0, len(genomes)))]
        o = int(rng.integers(0, len(g) - length + 1))
        r = _mutate(rng, g[o:o + length], rng.binomial(length, 0.06 * rng.random()))
        out.append(orc.revcomp(r) if i % 2 else r)
    g = genomes[0]
    return out + [b"", g[5:5 + K - 1], g[40:40 + K], _dna(rng, K)]


def compare_derived(ot, reads, base, thresholds):
    """(cases, mismatches): for every read and every threshold of the list, the row derived from the oracle's row and scores at
    `base` against the oracle's row at that threshold."""
    sets = oracle_sets(ot, reads, base)
    offs, leaves = csr_of(sets)
    scores = expected_scores(ot, reads, offs, leaves, ProbeContains(ot, reads))
    at = [oracle_sets(ot, reads, t) for t in thresholds]
    cases = bad = 0
    for r, s in enumerate(sets):
        row = sorted(s)
        need = sweep_ref.needs(thresholds, len(reads[r]), ot.kmer_size)
        derived = sweep_ref.derived_rows(row, scores[int(offs[r]):int(offs[r + 1])], need)
        for t in range(len(thresholds)):
            cases += 1
            bad += derived[t] != at[t][r]
    return cases, bad


def small_trees():
    rng = np.random.default_rng(2024)
    genomes = small_genomes(rng)
    ids = [f"S{i:03d}" for i in range(len(genomes))]
    balanced = oracle_tree(genomes, K, 30011, 4)[0]
    greedy = orc.build_greedy_tree(genomes, ids, K, 0.001, 1200, *SEEDS)
    return genomes, small_reads(rng, genomes), balanced, greedy


def test_one_pass_at_the_lowest_threshold_answers_every_threshold(sw):
    """The theorem, on W, a balanced and a greedy tree: no mismatch in any case, and more than ten thousand cases on each."""
    cases = bad = 0
    need_of = {n: sweep_ref.needs(LIST, n, K) for n in set(sw.lengths)}
    rows, scores, offs = sw.rows(LIST[0]), sw.scores(LIST[0]), csr_of(sw.sets(LIST[0]))[0]
    at = [sw.sets(t) for t in LIST]
    for r, row in enumerate(rows):
        derived = sweep_ref.derived_rows(row, scores[int(offs[r]):int(offs[r + 1])], need_of[sw.lengths[r]])
        for t in range(len(LIST)):
            cases += 1
            bad += derived[t] != at[t][r]
    print(f"W and the noisy reads: {cases} cases, {bad} mismatches")
    assert cases == len(sw.reads) * len(LIST) >= 10000 and bad == 0
    genomes, reads, balanced, greedy = small_trees()
    assert {len(r) for r in reads} >= {0, K - 1, K}
    for name, ot in (("balanced", balanced), ("greedy", greedy)):
        cases = bad = 0
        for base in SMALL_BASES:
            c, b = compare_derived(ot, reads, base, [t for t in SMALL_LIST if t >= base])
            cases, bad = cases + c, bad + b
        print(f"{name}: {cases} cases, {bad} mismatches")
        assert cases == len(reads) * 21 >= 10000 and bad == 0


def test_a_parent_that_is_no_superset_breaks_it():
    """Every second word of one internal filter cleared: reads pass that node at a low threshold and fail it at a higher one
    although the leaf below still passes, so the derived rows list leaves the oracle does not.  The reason for the refusal."""
    genomes, reads, balanced, _ = small_trees()
    internal = [v for v in range(balanced.n_nodes) if not balanced.is_leaf(v) and v != balanced.root]
    balanced.bits = balanced.bits.copy()
    balanced.bits[balanced.filter_of[internal[0]], ::2] = 0
    cases = bad = 0
    for base in SMALL_BASES:
        c, b = compare_derived(balanced, reads, base, [t for t in SMALL_LIST if t >= base])
        cases, bad = cases + c, bad + b
    print(f"non-superset: {cases} cases, {bad} mismatches")
    assert bad >= 1


def test_sweep_ref_against_counts_per_threshold(sw):
    """sweep_ref on the rows and scores of the base threshold against counts taken from the oracle's rows at every threshold."""
    ref, L = sw.ref(), sw.n_leaves
    assert ref["n_units"] == len(sw.reads) and int(ref["tops"].sum()) == len(sw.reads)
    for t, thr in enumerate(LIST):
        sets = sw.sets(thr)
        units = np.zeros(L, dtype=np.uint64)
        unique = np.zeros(L, dtype=np.uint64)
        for s in sets:
            for l in s:
                units[l] += 1
            if len(s) == 1:
                unique[next(iter(s))] += 1
        assert np.array_equal(ref["leaf_units"][t], units) and np.array_equal(ref["leaf_unique"][t], unique), thr
        assert int(ref["units_hit"][t]) == sum(1 for s in sets if s), thr
        assert int(ref["units_unique"][t]) == sum(1 for s in sets if len(s) == 1), thr
        assert int(ref["entries"][t]) == sum(len(s) for s in sets) and int(ref["genomes_hit"][t]) == int((units > 0).sum()), thr
    half = len(sw.reads) // 2
    offs = csr_of(sw.sets(LIST[0]))[0]
    cut = int(offs[half])
    rows, scores = sw.rows(LIST[0]), sw.scores(LIST[0])
    a = sweep_ref.sweep(rows[:half], scores[:cut], sw.lengths[:half], K, LIST, L)
    b = sweep_ref.sweep(rows[half:], scores[cut:], sw.lengths[half:], K, LIST, L)
    both = sweep_ref.absorb(a, b)
    assert both["n_units"] == ref["n_units"] and all(np.array_equal(both[k], ref[k]) for k in sweep_ref.READ_OUT + ("pass", "uniq", "tops"))


def test_the_reads_reach_every_bin(sw):
    """A condition on the expectation alone: W's own reads leave tops 1 and 2 empty, the noisy reads fill them; every value
    occurs as a top and as a second, the unique reads change from threshold to threshold, and a row is longer than 64 entries."""
    T = len(LIST)
    n_w = len(sw.w.reads)
    ref = sw.ref()
    tops_w = np.bincount(ref["top"][:n_w], minlength=T + 1)
    tops_noisy = np.bincount(ref["top"][n_w:], minlength=T + 1)
    print(f"tops of W {tops_w.tolist()} of the noisy reads {tops_noisy.tolist()} seconds {np.bincount(ref['second'], minlength=T).tolist()}")
    print(f"units_hit {ref['units_hit'].tolist()} units_unique {ref['units_unique'].tolist()} entries {ref['entries'].tolist()}")
    assert (tops_w == 0).any() and set(ref["top"].tolist()) == set(range(T + 1))
    assert set(range(T)) <= set(ref["second"].tolist())
    assert len(set(ref["units_unique"].tolist())) >= 3
    assert max(len(s) for s in sw.sets(LIST[0])) > 64
    assert ref["tops"].tolist() == (tops_w + tops_noisy).tolist()
