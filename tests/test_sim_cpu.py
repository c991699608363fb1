"""CPU only: tests/sim_ref.py itself — the integers on hand-made filters, and what the estimator makes of real k-mer sets put
into the oracle's filters: a filter against itself, strain families against unrelated genomes, the chance overlap of unrelated
genomes, a pair with a known true Jaccard index, and full filters."""
import numpy as np
import pytest

import sim_ref
from oracle import pfq_oracle as orc

K, H, NBITS = 21, 4, 200003
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def dna(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def mutate(rng, g, n_subs):
    b = bytearray(g)
    for p in rng.choice(len(b), size=n_subs, replace=False):
        b[p] = ACGT[(int(np.searchsorted(ACGT, b[p])) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(b)


def strain_families(rng, n_fam, strains, length, rate, singles):
    """As in test_gpu_abund: family f's strains are genomes [f * strains, (f + 1) * strains), then unrelated genomes."""
    out = []
    for _ in range(n_fam):
        base = dna(rng, length)
        out += [mutate(rng, base, rng.binomial(length, rate)) for _ in range(strains)]
    return out + [dna(rng, length) for _ in range(singles)]


def tree_of(genomes):
    return orc.build_balanced_tree(genomes, [f"G{i:03d}" for i in range(len(genomes))], K, NBITS, H, *SEEDS)


def true_jaccard(a, b):
    sa, sb = set(orc.get_kmers(a, K)), set(orc.get_kmers(b, K))
    return len(sa & sb) / len(sa | sb)


def test_integers_on_hand_made_filters():
    # nbits 70: two words, six bits of the second count; the padding above them must not
    a = np.array([[0b1011, 0b100001], [~np.uint64(0), ~np.uint64(0)], [0, 0]], dtype=np.uint64)
    b = np.array([[0b0110, 0b100000 | (1 << 6) | (1 << 63)], [0b1000, 0b1]], dtype=np.uint64)
    s = sim_ref.similarity_rows(a, b, 70, 3)
    assert s["shared_bits"].dtype == np.uint32 and s["shared_bits"].tolist() == [[2, 2], [3, 2], [0, 0]]
    assert s["bits_a"].dtype == np.uint64 and s["bits_a"].tolist() == [5, 70, 0] and s["bits_b"].tolist() == [3, 2]
    # the full row: nothing about it is estimable; the empty row: no k-mers, nothing shared
    assert s["kmers_a"][1] == 0.0 and not s["shared_kmers"][1].any() and not s["jaccard"][1].any()
    assert s["kmers_a"][2] == 0.0 and not s["shared_kmers"][2].any() and not s["jaccard"][2].any()
    assert s["kmers_a"][0] == pytest.approx(-(70 / 3) * np.log1p(-5 / 70), rel=1e-12)
    e = sim_ref.similarity_rows(a[:0], b, 70, 3)
    assert e["shared_bits"].shape == (0, 2) and e["bits_a"].shape == (0,) and e["jaccard"].shape == (0, 2)


def test_a_filter_against_itself():
    rng = np.random.default_rng(41)
    ot = tree_of([dna(rng, 2000) for _ in range(5)])
    s = sim_ref.similarity(ot)
    assert np.array_equal(np.diag(s["shared_bits"]).astype(np.uint64), s["bits_a"]) and np.array_equal(s["bits_a"], s["bits_b"])
    assert (np.diag(s["jaccard"]) == 1.0).all()                              # exactly: (x + x) - x = x in floating point
    assert np.array_equal(np.diag(s["shared_kmers"]), s["kmers_a"])
    assert np.array_equal(s["shared_bits"], s["shared_bits"].T) and np.array_equal(s["jaccard"], s["jaccard"].T)
    # about 1 980 distinct k-mers each
    assert np.allclose(s["kmers_a"], 1980, rtol=0.03)


def test_strain_families_stand_out():
    rng = np.random.default_rng(1217)
    n_fam, strains = 4, 3
    ot = tree_of(strain_families(rng, n_fam, strains, 2000, 0.006, 4))
    j = sim_ref.similarity(ot)["jaccard"]
    fam = [i // strains if i < n_fam * strains else -1 - i for i in range(16)]
    within = [j[a, b] for a in range(16) for b in range(a + 1, 16) if fam[a] == fam[b]]
    across = [j[a, b] for a in range(16) for b in range(a + 1, 16) if fam[a] != fam[b]]
    assert len(within) == n_fam * 3 and len(across) == 120 - len(within)
    assert min(within) > max(across), (min(within), max(across))
    assert min(within) > 0.5 and max(across) < 0.01, (min(within), max(across))


def test_unrelated_genomes_and_a_known_jaccard():
    rng = np.random.default_rng(7)
    x, y, z = dna(rng, 1000), dna(rng, 1000), dna(rng, 1000)
    genomes = [dna(rng, 2000) for _ in range(9)] + [x + y, x + z]
    ot = tree_of(genomes)
    s = sim_ref.similarity(ot)
    j = s["jaccard"]
    # unrelated pairs: the inclusion-exclusion cancels the chance overlap of two filters (about A * B / m bits)
    worst = max(j[a, b] for a in range(9) for b in range(a + 1, 9))
    assert worst < 0.01, worst
    assert (s["shared_bits"][:9, :9][~np.eye(9, dtype=bool)] > 100).all()   # (the bits they share by chance are not few)
    # half the sequence in common: the true value from the k-mer sets themselves
    want = true_jaccard(genomes[9], genomes[10])
    assert 0.3 < want < 0.36, want
    assert abs(j[9, 10] - want) <= 0.02, (j[9, 10], want)
    assert abs(s["shared_kmers"][9, 10] - len(set(orc.get_kmers(x, K)))) <= 0.05 * 980


def test_full_filters_give_zeros():
    nbits = 127
    full = np.array([[~np.uint64(0), ~np.uint64(0)]], dtype=np.uint64)
    half = np.array([[~np.uint64(0), 0]], dtype=np.uint64)
    s = sim_ref.similarity_rows(np.concatenate([full, half]), np.concatenate([full, half]), nbits, 4)
    assert s["bits_a"].tolist() == [127, 64] and s["shared_bits"].tolist() == [[127, 64], [64, 64]]
    assert s["kmers_a"][0] == 0.0 and s["kmers_a"][1] > 0.0
    assert not s["shared_kmers"][0].any() and not s["shared_kmers"][:, 0].any() and not s["jaccard"][0].any() and not s["jaccard"][:, 0].any()
    assert s["jaccard"][1, 1] == 1.0
    # and the line a pair of them gets
    assert sim_ref.tsv_line("a", "b", s, 0, 1, 21) == "a\tb\t127\t64\t64\t0.0\t%.1f\t0.0\t0.000000\t0.000000\t0.000000\t0.000000" % s["kmers_b"][1]
