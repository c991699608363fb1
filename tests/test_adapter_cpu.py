"""The adapter rule (pfq.h "adapters") as tests/adapter_ref.py restates it: worked examples, a brute-force cross-check, the defining
property against prep_ref on the cut reads, and the binding's view of the three new entry points."""
import ctypes as C
import os
import re

import numpy as np

import adapter_ref
import prep_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AD = b"AGATCGGAAGAGC"                                                 # 13 bases
NONE = adapter_ref.NO_ADAPTER


def header():
    return open(os.path.join(ROOT, "include", "pfq.h")).read()


def dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n).astype(np.uint8))


def test_match_at_the_first_base():
    assert adapter_ref.find_cut(AD + b"TTTTT", [AD], 5, 0) == (0, 0)
    assert adapter_ref.find_cut(b"", [AD], 5, 0) == (0, NONE)


def test_overlap_of_exactly_min_overlap_at_the_end():
    O = 5
    body = b"CCCCCCCCCCCCCCCCCCCC"                                     # no A or G: nothing in it looks like the adapter's head
    s = body + AD[:O]
    assert adapter_ref.find_cut(s, [AD], O, 0) == (len(s) - O, 0)
    assert adapter_ref.find_cut(body + AD[:O - 1], [AD], O, 0) == (len(body) + O - 1, NONE)      # the overlap at L - O + 1 is O - 1
    assert not adapter_ref.matches(s, len(s) - O + 1, AD, O, 50)


def test_mismatches_at_the_bound_and_one_more():
    ad = b"ACGTACGTACGTACGTACGT"                                       # o = 20, E = 10: two mismatches pass, three do not
    body = b"T" * 12

    def spoiled(k):
        t = bytearray(ad)
        for j in range(k):
            t[3 + 5 * j] = ord("A") if t[3 + 5 * j] != ord("A") else ord("C")
        return bytes(t)
    assert 10 * 20 // 100 == 2
    assert adapter_ref.find_cut(body + spoiled(2), [ad], 5, 10) == (12, 0)
    assert adapter_ref.find_cut(body + spoiled(3), [ad], 20, 10) == (32, NONE)
    assert adapter_ref.find_cut(body + spoiled(3), [ad], 20, 15) == (12, 0)                     # 100 * 3 <= 15 * 20
    # at the read's end the bound follows the overlap: o = 9 at E = 10 allows no mismatch, o = 10 allows one
    assert not adapter_ref.matches(b"G" * 4 + b"ACGTACGTT", 4, ad, 5, 10)
    assert adapter_ref.matches(b"G" * 4 + b"ACGTACGTTC", 4, ad, 5, 10)


def test_n_and_lower_case_inside_the_overlap():
    body = b"CCCCCCCCCC"
    assert adapter_ref.find_cut(body + AD.lower(), [AD], 13, 0) == (10, 0)                      # lower case matches
    with_n = body + AD[:4] + b"N" + AD[5:]
    assert adapter_ref.find_cut(with_n, [AD], 13, 0) == (23, NONE)                               # an N always mismatches
    assert adapter_ref.find_cut(with_n, [AD], 13, 10) == (10, 0)                                 # 100 * 1 <= 10 * 13
    assert adapter_ref.find_cut(body + AD[:4] + b"n" + AD[5:], [AD], 13, 0) == (23, NONE)
    assert adapter_ref.find_cut(body + AD, [AD.lower()], 13, 0) == (10, 0)                       # adapters are stored in upper case


def test_the_lower_index_wins_at_one_position_and_the_smaller_position_wins():
    body = b"CCCCCCCCCC"
    s = body + AD + b"TTTT"
    assert adapter_ref.find_cut(s, [AD[:8], AD], 5, 0) == (10, 0)
    assert adapter_ref.find_cut(s, [AD, AD[:8]], 5, 0) == (10, 0)
    assert adapter_ref.find_cut(s, [b"GGGGGGGG", AD[:8], AD], 5, 0) == (10, 1)
    later, earlier = b"TTTTT", b"CCCCCAGATC"                                                    # adapter 1 matches at 5, adapter 0 only at 23
    assert adapter_ref.find_cut(s, [later, earlier], 5, 0) == (5, 1)
    assert adapter_ref.find_cut(s, [later], 4, 0) == (23, 0)


def brute(s, adapters, O, E):
    best = (len(s), NONE)
    for i in reversed(range(len(adapters))):
        a = adapters[i].upper()
        for p in reversed(range(len(s))):
            o = min(len(a), len(s) - p)
            mm = 0
            for j in range(o):
                c = s[p + j]
                c = c - 32 if 97 <= c <= 122 else c
                mm += 0 if (c in b"ACGT" and c == a[j]) else 1
            if o >= O and 100 * mm <= E * o and (p, i) <= best:
                best = (p, i)
    return best


def test_find_cut_against_brute_force():
    rng = np.random.default_rng(7)
    found = 0
    for _ in range(600):
        O, E = int(rng.integers(1, 9)), int(rng.choice([0, 10, 20, 50]))
        adapters = [dna(rng, int(rng.integers(O, 14))) for _ in range(int(rng.integers(1, 4)))]
        s = bytearray(dna(rng, int(rng.integers(0, 40)), b"ACGTacgtN"))
        if len(s) > 6 and rng.integers(2):
            a = adapters[int(rng.integers(len(adapters)))]
            at = int(rng.integers(0, len(s)))
            s[at:] = (a + dna(rng, 40))[:len(s) - at]
        got = adapter_ref.find_cut(bytes(s), adapters, O, E)
        assert got == brute(bytes(s), adapters, O, E), (bytes(s), adapters, O, E)
        found += got[1] != NONE
    assert 100 < found < 600


def test_the_block_equals_prep_ref_on_the_cut_reads():
    rng = np.random.default_rng(8)
    ad2 = b"CTGTCTCTTATACACATCT"
    reads, quals = [], []
    for i in range(200):
        n = int(rng.integers(0, 60))
        s = dna(rng, n) + ((AD if i % 3 else ad2) + dna(rng, 20))[:int(rng.integers(0, 30))]
        if i % 7 == 0:
            s = s + b"G" * 12
        reads.append(s)
        quals.append(None if i % 11 == 0 else bytes(rng.choice(np.frombuffer(b"#5I", dtype=np.uint8), len(s), p=[.1, .2, .7]).astype(np.uint8)))
    params = dict(trim_quality=20, trim_window=4, poly_x=10, min_length=15, max_n=2, min_complexity=20)
    for paired, set2 in ((False, ()), (True, ()), (True, (ad2,))):
        got = adapter_ref.prep_block(reads, quals, [AD], set2, 5, 10, paired=paired, **params)
        cuts = [adapter_ref.find_cut(s, set2 if paired and i % 2 and set2 else [AD], 5, 10) for i, s in enumerate(reads)]
        assert got["cut"] == [c for c, _ in cuts] and got["which"] == [w for _, w in cuts]
        assert 60 < got["n_found"] < 200 and got["n_found"] == sum(1 for w in got["which"] if w != NONE) == sum(got["found"])
        assert got["bases_cut"] == sum(len(s) - c for s, c in zip(reads, got["cut"]))
        assert bool(sum(got["found"][8:])) == bool(set2)
        want = prep_ref.prep_block([s[:c] for s, c in zip(reads, got["cut"])],
                                   [None if q is None else q[:c] for q, c in zip(quals, got["cut"])], paired=paired, **params)
        for k in ("begin", "len", "reason", "kept", "kept_reads", "n_kept", "bases_kept", "n_reason"):
            assert got[k] == want[k], (paired, k)
        assert got["bases_in"] == sum(map(len, reads)) > want["bases_in"]
        assert got["n_trimmed"] == sum(1 for i in got["kept"] if got["len"][i] < len(reads[i])) > want["n_trimmed"]
        assert all(got["begin"][i] + got["len"][i] <= got["cut"][i] for i in range(len(reads)))


def test_the_binding_declares_the_adapter_calls():
    import phagefilter_amd
    from phagefilter_amd import BloomTree, _ffi
    L = phagefilter_amd.lib()
    for name in ("pfq_tree_set_adapters", "pfq_prep_last_adapters", "pfq_debug_last_adapters"):
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
        assert re.search(rf"^int {name}\(", header(), re.M), name
        assert getattr(L, name).argtypes is not None, name
    assert len(L.pfq_tree_set_adapters.argtypes) == 7
    m = re.search(r"typedef struct pfq_prep_adapters \{(.*?)\} pfq_prep_adapters;", header(), re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)(?:\[[^\]]*\])?\s*(?:,|$)", re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()))]
    assert names == [f[0] for f in _ffi.PrepAdapters._fields_]
    assert re.search(r"#define PFQ_ADAPTER_MAX 8\b", header()) and re.search(r"#define PFQ_ADAPTER_LEN_MAX 64\b", header())
    assert (_ffi.ADAPTER_MAX, _ffi.ADAPTER_LEN_MAX) == (8, 64) == (adapter_ref.ADAPTER_MAX, 64)
    assert C.sizeof(_ffi.PrepAdapters) == 3 * 8 + 16 * 8 + 2 * C.sizeof(C.c_void_p)
    assert (_ffi.PrepAdapters.found.offset, _ffi.PrepAdapters.cut.offset, _ffi.PrepAdapters.which.offset) == (24, 152, 152 + C.sizeof(C.c_void_p))
    for method in ("set_adapters", "last_adapters", "last_adapters_ms"):
        assert callable(getattr(BloomTree, method)), method
    # the existing structs are what they were
    assert C.sizeof(_ffi.PrepParams) == 7 * 4 and len(_ffi.Prep._fields_) == 10
