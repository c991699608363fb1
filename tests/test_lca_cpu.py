"""The lowest-common-ancestor surface of the C ABI and of the Python wrapper, without a device: the flag values the header
defines are the ones the wrapper passes, the new calls are bound, and the wrapper refuses a bad `lca` argument before
calling into the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "pfq.h")).read()


def test_lca_flags_match_header():
    from phagefilter_amd import _ffi
    flags = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define (PFQ_[A-Z_]+) (\d+|0x[0-9a-f]+)u", header(), re.M)}
    assert flags["PFQ_WANT_LCA"] == _ffi.WANT_LCA == 16 and flags["PFQ_LCA_BEST"] == _ffi.LCA_BEST == 32
    assert flags["PFQ_NO_CLADE"] == _ffi.NO_CLADE == 0xFFFFFFFF
    bits = [flags[n] for n in ("PFQ_WANT_HITS", "PFQ_WANT_SCORES", "PFQ_PAIRED", "PFQ_PAIR_BOTH", "PFQ_WANT_LCA", "PFQ_LCA_BEST")]
    assert all(v & (v - 1) == 0 for v in bits) and len(set(bits)) == len(bits)      # distinct single bits


def test_lca_symbols_declared_bound_and_exported():
    import phagefilter_amd
    from phagefilter_amd import _ffi
    L = phagefilter_amd.lib()
    for name in ("pfq_tree_clades", "pfq_clade_counts", "pfq_last_lca"):
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
        assert re.search(rf"^int {name}\(", header(), re.M), name
        assert getattr(L, name).argtypes is not None, name
    # pfq_clade as the header lays it out: four u32, then the name pointer
    assert [f[0] for f in _ffi.Clade._fields_] == ["parent", "depth", "first_leaf", "n_leaves", "name"]
    assert C.sizeof(_ffi.Clade) == 16 + C.sizeof(C.c_void_p) and _ffi.Clade.name.offset == 16
    m = re.search(r"typedef struct pfq_clade \{(.*?)\} pfq_clade;", header(), re.S)
    assert m and re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)) == \
        ["parent", "depth", "first_leaf", "n_leaves", "name"]


def test_lca_arguments_checked_before_the_library():
    from phagefilter_amd import BloomTree
    from phagefilter_amd.query import _lca_flags
    assert _lca_flags(None, False, False) == 0 and _lca_flags(None, True, True) == 0
    assert _lca_flags("all", False, False) == 16 and _lca_flags("all", True, True) == 16
    assert _lca_flags("best", True, True) == 48
    for hits, scores in ((False, False), (True, False), (False, True)):
        with pytest.raises(ValueError):
            _lca_flags("best", hits, scores)
    for bad in ("", "ALL", "deepest", True, 1):
        with pytest.raises(ValueError):
            _lca_flags(bad, True, True)
    t = BloomTree(C.c_void_p(), 0)                                  # no device needed: refused before any call
    seq, off = np.zeros(16, dtype=np.uint8), np.zeros(3, dtype=np.uint64)
    with pytest.raises(ValueError):
        t.query_packed(seq, off, 1.0, lca="lowest")
    with pytest.raises(ValueError):
        t.query_packed(seq, off, 1.0, lca="best")
    with pytest.raises(ValueError):
        t.query_packed(seq, off, 1.0, want_hits=True, lca="best")
    with pytest.raises(ValueError):
        t.query_device(0, 0, 2, 0, 1.0, lca="best")
    with pytest.raises(ValueError):
        t.query_device(0, 0, 2, 0, 1.0, lca="both")
    with pytest.raises(ValueError):
        t.query_device_hits(0, 0, 2, 0, 1.0, lca="best")
    with pytest.raises(ValueError):
        t.query_device_hits(0, 0, 2, 0, 1.0, want_scores=True, lca="top")
    with pytest.raises(ValueError):
        t.query_pairs([b"ACGT"], [b"ACGT"], 1.0, lca="every")
    for call in (t.clades, t.clade_counts, t.last_lca):
        assert callable(call)
