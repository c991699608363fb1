"""CPU only: tests/deplete_ref.py against an independent brute-force statement of the rule (pfq.h "depletion") — per leaf of the
screen, get_kmers, bf_contains and need(), sharing no code with the oracle's query_batch — on about 40 reads and a screen of 4
leaves: exact screen reads, one substitution (removed at 0.7, kept at 1.0), foreign reads, reads under the screen's k, an empty
read, fragments in both pair modes, two screens in sequence, idempotence."""
import numpy as np
import pytest

import deplete_ref
import prep_ref
from oracle import pfq_oracle as orc

K, H, NBITS, SEEDS = 17, 3, 100003, (0x1111222233334444, 0x9999AAAABBBBCCCC)


def dna(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).astype(np.uint8))


def substitute(read, at):
    return read[:at] + bytes([{65: 67, 67: 71, 71: 84, 84: 65}[read[at]]]) + read[at + 1:]


class Case:
    def __init__(self):
        rng = self.rng = np.random.default_rng(20261020)
        self.genomes = [dna(rng, 1500) for _ in range(4)]
        self.screen = orc.build_balanced_tree(self.genomes, [f"S{i}" for i in range(4)], K, NBITS, H, *SEEDS)
        self.other_genome = dna(rng, 1500)
        self.other = orc.build_balanced_tree([self.other_genome], ["X0"], K, NBITS, H, *SEEDS)
        g = self.genomes
        self.exact = [g[i % 4][50 * i:50 * i + 60] for i in range(10)]
        # a substitution 5 bases from the end of 60 spoils the last 5 of the 44 k-mers: 39 are left, need(0.7, 44) = 31, need(1, 44) = 44
        self.subst = [substitute(g[i % 4][70 * i + 5:70 * i + 65], 55) for i in range(10)]
        self.foreign = [dna(rng, 60) for _ in range(10)]
        self.other_reads = [self.other_genome[40 * i:40 * i + 60] for i in range(4)]
        self.tiny = [g[0][:K - 1], dna(rng, 5), b"A", b""]
        self.reads = self.exact + self.subst + self.foreign + self.other_reads + self.tiny


@pytest.fixture(scope="module")
def case():
    return Case()


def brute_sets(tree, reads, thr):
    """Per read the leaf columns it passes: k-mers counted filter by filter.  The leaves of a balanced tree decide alone: every
    ancestor's filter is the union of its children's, so a read that passes a leaf passes the path to it."""
    leaves = tree.leaves_dfs()
    out = []
    for r in reads:
        kmers = orc.get_kmers(r, tree.kmer_size)
        assert len(kmers) == max(len(r) - tree.kmer_size + 1, 0)
        want = orc.need(thr, len(kmers))
        out.append({c for c, v in enumerate(leaves) if sum(orc.bf_contains(tree, tree.filter_of[v], m) for m in kmers) >= want})
    return out


def brute(tree, reads, thr, paired=False, both=False):
    sets = brute_sets(tree, reads, thr)
    if paired:
        rows = [(sets[i] & sets[i + 1]) if both else (sets[i] | sets[i + 1]) for i in range(0, len(reads), 2)]
    else:
        rows = sets
    return rows, [len(row) > 0 for row in rows]


def test_groups_behave_as_the_rule_says(case):
    assert len(case.reads) == 38 and len(case.screen.leaves_dfs()) == 4
    for thr in (0.7, 1.0):
        got = deplete_ref.deplete(case.reads, case.screen, thr)
        rows, removed = brute(case.screen, case.reads, thr)
        assert got["rows"] == rows and got["removed"] == removed, thr
        n = 0
        assert all(removed[n:n + 10]), "exact screen reads leave at every threshold"
        assert [rows[i] >= {i % 4} for i in range(10)] == [True] * 10
        n += 10
        assert removed[n:n + 10] == [thr < 1.0] * 10, "one substitution: removed at 0.7, kept at 1.0"
        n += 10
        assert not any(removed[n:n + 14]), "foreign reads stay"
        n += 14
        assert all(removed[n:]) and all(row == {0, 1, 2, 3} for row in rows[n:]), "reads under the screen's k pass every leaf"
        stay = [i for i in range(len(case.reads)) if not removed[i]]
        assert got["kept"] == stay and got["survivors"] == [case.reads[i] for i in stay]
        assert got["reason"] == [5 if f else 0 for f in removed]
        assert got["units_removed"] == got["reads_removed"] == sum(removed) and got["n_units"] == 38
        assert got["bases_removed"] == sum(len(case.reads[i]) for i in range(38) if removed[i])
        assert got["n_kept"] == len(stay) and got["bases_kept"] == sum(len(case.reads[i]) for i in stay)
        assert got["leaf_counts"] == [sum(1 for row in rows if c in row) for c in range(4)]
    assert orc.need(0.7, 44) == 31 <= 44 - 5 < orc.need(1.0, 44) == 44                            # why the substituted reads behave so
    assert case.screen.leaf_counts() == [(f"S{i}", 0) for i in range(4)]                          # the reference leaves the oracle's counters alone


@pytest.mark.parametrize("both", [False, True])
def test_fragments(case, both):
    e, f, t = case.exact, case.foreign, case.tiny
    #         both from the screen, one mate, the other mate, none, one mate under k + screen, under k + foreign, both under k, empty + foreign
    frags = [(e[0], e[4]), (e[1], f[0]), (f[1], e[2]), (f[2], f[3]), (t[0], e[3]), (t[1], f[4]), (t[2], t[3]), (t[3], f[5]), (e[0], e[1])]
    reads = [m for p in frags for m in p]
    got = deplete_ref.deplete(reads, case.screen, 1.0, paired=True, both=both)
    rows, removed = brute(case.screen, reads, 1.0, paired=True, both=both)
    assert got["rows"] == rows and got["removed"] == removed
    # either: any mate from the screen or under k; both: the intersection — a mate under k hands the fragment the other mate's set
    assert removed == ([True, True, True, False, True, True, True, True, True] if not both else
                       [True, False, False, False, True, False, True, False, False])
    assert rows[4] >= {3} and (rows[4] == {0, 1, 2, 3}) == (not both)
    assert got["n_units"] == 9 and got["units_removed"] == sum(removed) and got["reads_removed"] == 2 * sum(removed)
    assert got["kept"] == [i for i in range(18) if not removed[i // 2]] and len(got["survivors"]) == got["n_kept"] == 18 - 2 * sum(removed)
    assert [why == 5 for why in got["reason"]] == [removed[i // 2] for i in range(18)]
    assert got["leaf_counts"] == [sum(1 for row in rows if c in row) for c in range(4)]


def test_after_a_prep_the_indices_are_the_blocks(case):
    reads = [case.exact[0], b"ACGT", case.foreign[0], case.exact[1] + b"G" * 12, case.foreign[1], b""]
    prep = prep_ref.prep_block(reads, None, poly_x=10, min_length=K)
    assert prep["kept"] == [0, 2, 3, 4] and prep["begin"][3] == 0 and K <= prep["len"][3] <= 60
    got = deplete_ref.deplete(prep["kept_reads"], case.screen, 1.0, kept=prep["kept"], reason=prep["reason"])
    assert got["kept"] == [2, 4] and got["reason"] == [5, 1, 0, 5, 0, 1] and got["survivors"] == [reads[2], reads[4]]
    assert prep["reason"] == [0, 1, 0, 0, 0, 1]                                                   # the prep's own list is not written to


def test_two_screens_in_sequence_equal_the_union_and_idempotence(case):
    reads, thr = case.reads, 0.7
    a = deplete_ref.deplete(reads, case.screen, thr)
    b = deplete_ref.deplete(a["survivors"], case.other, thr, kept=a["kept"], reason=a["reason"])
    _, in_a = brute(case.screen, reads, thr)
    _, in_b = brute(case.other, reads, thr)
    union = [x or y for x, y in zip(in_a, in_b)]
    assert any(y and not x for x, y in zip(in_a, in_b)), "the second screen removes something the first left"
    assert b["kept"] == [i for i in range(len(reads)) if not union[i]]
    assert b["reason"] == [5 if u else 0 for u in union]
    assert b["n_units"] == a["n_kept"] and b["units_removed"] == sum(union) - sum(in_a)
    # the other order removes the same reads
    b2 = deplete_ref.deplete(reads, case.other, thr)
    a2 = deplete_ref.deplete(b2["survivors"], case.screen, thr, kept=b2["kept"], reason=b2["reason"])
    assert a2["kept"] == b["kept"] and a2["survivors"] == b["survivors"]
    # the same screen again removes nothing
    again = deplete_ref.deplete(a["survivors"], case.screen, thr, kept=a["kept"], reason=a["reason"])
    assert again["units_removed"] == 0 and again["kept"] == a["kept"] and again["reason"] == a["reason"] and again["survivors"] == a["survivors"]
    assert again["leaf_counts"] == [0, 0, 0, 0]
