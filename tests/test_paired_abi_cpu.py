"""The paired-end surface of the C ABI and of the Python wrapper, without a device: the flag values the header defines are the
ones the wrapper passes, and the wrapper refuses bad pairing arguments before calling into the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_flags():
    header = open(os.path.join(ROOT, "include", "pfq.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (PFQ_[A-Z_]+) (\d+)u", header, re.M)}


def test_pair_flags_match_header():
    from phagefilter_amd import _ffi
    flags = header_flags()
    assert flags["PFQ_PAIRED"] == _ffi.PAIRED and flags["PFQ_PAIR_BOTH"] == _ffi.PAIR_BOTH
    assert flags["PFQ_WANT_HITS"] == _ffi.WANT_HITS and flags["PFQ_WANT_SCORES"] == _ffi.WANT_SCORES
    values = [flags[n] for n in ("PFQ_WANT_HITS", "PFQ_WANT_SCORES", "PFQ_PAIRED", "PFQ_PAIR_BOTH")]
    assert all(v & (v - 1) == 0 for v in values) and len(set(values)) == len(values)   # distinct single bits


def test_pair_arguments_checked_before_the_library():
    from phagefilter_amd import BloomTree
    from phagefilter_amd.query import _pair_flags
    assert _pair_flags(False, "either") == 0
    assert _pair_flags(True, "either") == 4 and _pair_flags(True, "both") == 12
    with pytest.raises(ValueError):
        _pair_flags(True, "neither")
    with pytest.raises(ValueError):
        _pair_flags(False, "union")
    t = BloomTree(C.c_void_p(), 0)                                  # no device needed: refused before any call
    with pytest.raises(ValueError):
        t.query_pairs([b"ACGT"], [], 1.0)
    with pytest.raises(ValueError):
        t.query_packed(np.zeros(16, dtype=np.uint8), np.zeros(3, dtype=np.uint64), 1.0, paired=True, pair_mode="all")
