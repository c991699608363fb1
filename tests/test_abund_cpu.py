"""The abundance surface of the C ABI and of the Python wrapper, without a device: the flag value the header defines is the
one the wrapper passes, the new calls are declared, bound and exported, the wrapper refuses `abundance=True` without the
hits before calling into the library — and the plain-Python restatement of the estimate (tests/abund_ref.py), which the GPU
tests compare the library with, does what include/pfq.h says on logs small enough to work by hand."""
import ctypes as C
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abund_ref  # noqa: E402


def header():
    return open(os.path.join(ROOT, "include", "pfq.h")).read()


def test_abundance_flag_matches_header():
    from phagefilter_amd import _ffi
    flags = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define (PFQ_[A-Z_]+) (\d+|0x[0-9a-f]+)u", header(), re.M)}
    assert flags["PFQ_WANT_ABUNDANCE"] == _ffi.WANT_ABUNDANCE == 64
    bits = [flags[n] for n in ("PFQ_WANT_HITS", "PFQ_WANT_SCORES", "PFQ_PAIRED", "PFQ_PAIR_BOTH", "PFQ_WANT_LCA", "PFQ_LCA_BEST",
                               "PFQ_WANT_ABUNDANCE")]
    assert all(v & (v - 1) == 0 for v in bits) and len(set(bits)) == len(bits)      # distinct single bits
    assert re.search(r"^#define PFQ_ABUND_Q 16\b", header(), re.M) and _ffi.ABUND_Q == abund_ref.Q == 16


def test_abundance_symbols_declared_bound_and_exported():
    import phagefilter_amd
    from phagefilter_amd import _ffi
    L = phagefilter_amd.lib()
    for name in ("pfq_abundance_estimate", "pfq_abundance_reset", "pfq_abundance_absorb"):
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
        assert re.search(rf"^int {name}\(", header(), re.M), name
        assert getattr(L, name).argtypes is not None, name
    # pfq_abundance as the header lays it out
    m = re.search(r"typedef struct pfq_abundance \{(.*?)\} pfq_abundance;", header(), re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)\s*(?:,|$)", re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()))]
    assert names == [f[0] for f in _ffi.Abundance._fields_]
    assert C.sizeof(_ffi.Abundance) == 8 + 2 * C.sizeof(C.c_void_p) + 7 * 8 + 2 * 4
    assert _ffi.Abundance.iterations.offset == C.sizeof(_ffi.Abundance) - 8


def test_abundance_needs_the_hits_before_the_library():
    from phagefilter_amd import BloomTree
    from phagefilter_amd.query import _abundance_flags
    assert _abundance_flags(False, False) == 0 and _abundance_flags(False, True) == 0 and _abundance_flags(True, True) == 64
    with pytest.raises(ValueError):
        _abundance_flags(True, False)
    t = BloomTree(C.c_void_p(), 0)                                  # no device needed: refused before any call
    seq, off = np.zeros(16, dtype=np.uint8), np.zeros(3, dtype=np.uint64)
    with pytest.raises(ValueError):
        t.query_packed(seq, off, 1.0, abundance=True)
    with pytest.raises(ValueError):
        t.query_packed(seq, off, 1.0, want_hits=False, lca="all", abundance=True)
    for call in (t.abundance, t.abundance_reset, t.abundance_absorb):
        assert callable(call)


# ---- the restatement itself

def test_ref_two_leaves_by_hand():
    # 3 units on leaf 0 alone, 1 on leaf 1 alone, 4 on both, in a tree of 3 leaves (so {0, 1} is not "all leaves")
    log = abund_ref.classify([[0]] * 3 + [[1]] + [[0, 1]] * 4, 3)
    assert (log["n_units"], log["n_unique"], log["n_ambiguous"], log["n_entries"], log["unique"]) == (8, 4, 4, 8, [3, 1, 0])
    e1 = abund_ref.estimate(log, max_iters=1, tol=0)
    # uniform start: every shared unit is split in halves
    assert e1["mass"] == [(3 << 16) + 4 * 32768, (1 << 16) + 4 * 32768, 0] and e1["iterations"] == 1 and e1["converged"] == 0
    assert e1["last_delta"] == (5 << 16) - (1 << 16)
    e2 = abund_ref.estimate(log, max_iters=2, tol=0)
    # second iteration: a = (5, 3, 0) units, D = 8 units: shares 5/8 and 3/8 of 2^16, floored
    assert e2["mass"] == [(3 << 16) + 4 * ((5 << 32) // (8 << 16)), (1 << 16) + 4 * ((3 << 32) // (8 << 16)), 0]
    assert e2["mass"] == [(3 << 16) + 4 * 40960, (1 << 16) + 4 * 24576, 0]
    # the fixed point keeps the unique proportions 3 : 1 -> 6 and 2 units, up to the floors
    e = abund_ref.estimate(log, max_iters=500, tol=0)
    assert e["converged"] == 1 and e["last_delta"] == 0 and e["mass"][2] == 0
    assert abs(e["mass"][0] - (6 << 16)) < 64 and abs(e["mass"][1] - (2 << 16)) < 64
    assert 0 <= (8 << 16) - sum(e["mass"]) < 2 * 4                    # the floors lose less than |R| per row and iteration
    # tol: stops at the first iteration whose delta is within it
    et = abund_ref.estimate(log, max_iters=500, tol=65)
    assert et["converged"] == 1 and et["last_delta"] <= 65 and et["iterations"] <= e["iterations"]


def test_ref_class_rules():
    rows = [[], [2], [0, 1, 2, 3], [1, 3], [0, 1, 2], []]
    log = abund_ref.classify(rows, 4)
    assert (log["n_units"], log["n_unhit"], log["n_unique"], log["n_all_leaves"], log["n_ambiguous"], log["n_entries"]) == (6, 2, 1, 1, 2, 5)
    assert log["unique"] == [0, 0, 1, 0] and sum(log["rows"].values()) == 2
    # a tree of one leaf: its only possible non-empty row is unique, never "all leaves"
    one = abund_ref.classify([[0], [0], []], 1)
    assert (one["n_unique"], one["n_all_leaves"], one["n_unhit"], one["unique"]) == (2, 0, 1, [2])
    assert abund_ref.estimate(one, 5, 0)["mass"] == [2 << 16]
    # two leaves: a row of both is "all leaves" and says nothing
    two = abund_ref.classify([[0, 1], [0, 1], [1]], 2)
    assert (two["n_all_leaves"], two["n_ambiguous"], two["n_unique"]) == (2, 0, 1)
    assert abund_ref.estimate(two, 5, 0)["mass"] == [0, 1 << 16]
    # nothing logged: zeros, one iteration
    e = abund_ref.estimate(abund_ref.classify([], 4))
    assert e["mass"] == [0] * 4 and (e["iterations"], e["converged"], e["last_delta"], e["n_units"]) == (1, 1, 0, 0)


def test_ref_zero_denominator_adds_nothing():
    # a row whose leaves all hold no mass contributes nothing (with the uniform start this needs >= 65 536 leaves; here a start)
    log = abund_ref.classify([[0, 1], [2]], 4)
    e = abund_ref.estimate(log, max_iters=1, tol=0, start=[0, 0, 1 << 16, 0])
    assert e["mass"] == [0, 0, 1 << 16, 0]
    # and with the uniform start, once a row's leaves have lost their mass: leaves 0, 1 only share a row with each other
    # -> they keep exactly that row's unit between them and never reach D == 0; a leaf without any row goes to 0 at once
    e = abund_ref.estimate(log, max_iters=3, tol=0)
    assert e["mass"][3] == 0 and e["mass"][0] + e["mass"][1] == 1 << 16


def test_ref_row_order_does_not_matter():
    rnd = random.Random(7)
    rows = [sorted(rnd.sample(range(9), rnd.choice((0, 1, 1, 2, 3, 5, 9)))) for _ in range(400)]
    ref = abund_ref.estimate(abund_ref.classify(rows, 9), 40, 0)
    shuffled = rows[:]
    rnd.shuffle(shuffled)
    assert abund_ref.estimate(abund_ref.classify(shuffled, 9), 40, 0) == ref
    assert abund_ref.estimate(abund_ref.classify(rows[::-1], 9), 40, 0) == ref
    log = abund_ref.classify(rows[:100], 9)                                         # the same rows, logged in two goes
    abund_ref.add(log, rows[100:])
    assert abund_ref.estimate(log, 40, 0) == ref
    assert ref["n_units"] == 400 and ref["n_unhit"] + ref["n_unique"] + ref["n_ambiguous"] + ref["n_all_leaves"] == 400
