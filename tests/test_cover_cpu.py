"""The coverage surface without a device: the flag, the struct and the calls as the header, the ctypes mirror and the wrapper
have them; the plain-Python restatement (tests/cover_ref.py) that the GPU tests compare the library with — rho's edge cases,
independence of order and splitting, absorb, the estimator's accuracy; and the option errors of `phage_filter query --coverage`,
which are raised before any device is opened."""
import ctypes as C
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cover_ref  # noqa: E402

CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")
M64 = (1 << 64) - 1


def header():
    return open(os.path.join(ROOT, "include", "pfq.h")).read()


# ---- ABI

def test_coverage_flag_matches_header():
    from phagefilter_amd import _ffi
    flags = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define (PFQ_[A-Z_]+) (\d+|0x[0-9a-f]+)u", header(), re.M)}
    assert flags["PFQ_WANT_COVERAGE"] == _ffi.WANT_COVERAGE == 128
    bits = [flags[n] for n in ("PFQ_WANT_HITS", "PFQ_WANT_SCORES", "PFQ_PAIRED", "PFQ_PAIR_BOTH", "PFQ_WANT_LCA", "PFQ_LCA_BEST",
                               "PFQ_WANT_ABUNDANCE", "PFQ_WANT_COVERAGE")]
    assert all(v & (v - 1) == 0 for v in bits) and len(set(bits)) == len(bits)      # distinct single bits


def test_coverage_symbols_declared_bound_and_exported():
    import phagefilter_amd
    from phagefilter_amd import _ffi
    L = phagefilter_amd.lib()
    for name in ("pfq_coverage_get", "pfq_coverage_reset", "pfq_coverage_absorb"):
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
        assert re.search(rf"^int {name}\(", header(), re.M), name
        assert getattr(L, name).argtypes is not None, name
    m = re.search(r"typedef struct pfq_coverage \{(.*?)\} pfq_coverage;", header(), re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)\s*(?:,|$)", re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()))]
    assert names == [f[0] for f in _ffi.Coverage._fields_]
    # two u64, a u32 padded to 8, six pointers
    assert C.sizeof(_ffi.Coverage) == 3 * 8 + 6 * C.sizeof(C.c_void_p)
    assert _ffi.Coverage.precision.offset == 16 and _ffi.Coverage.registers.offset == 24


def test_coverage_needs_the_hits_before_the_library():
    from phagefilter_amd import BloomTree
    from phagefilter_amd.query import _coverage_flags
    assert _coverage_flags(False, False) == 0 and _coverage_flags(False, True) == 0 and _coverage_flags(True, True) == 128
    with pytest.raises(ValueError):
        _coverage_flags(True, False)
    t = BloomTree(C.c_void_p(), 0)                                  # no device needed: refused before any call
    seq, off = np.zeros(16, dtype=np.uint8), np.zeros(3, dtype=np.uint64)
    with pytest.raises(ValueError):
        t.query_packed(seq, off, 1.0, coverage=True)
    with pytest.raises(ValueError):
        t.query_packed(seq, off, 1.0, want_hits=False, lca="all", coverage=True)
    for call in (t.coverage, t.coverage_reset, t.coverage_absorb):
        assert callable(call)


# ---- the restatement itself

def test_mix_is_the_splitmix64_finaliser():
    # splitmix64's first two outputs from state 0 are the finaliser of the golden-gamma multiples
    g = 0x9E3779B97F4A7C15
    assert cover_ref.mix(g) == 0xE220A8397B1DCDAF and cover_ref.mix((2 * g) & M64) == 0x6E789E6AA1B965F4
    assert cover_ref.mix(0) == 0


@pytest.mark.parametrize("p", [4, 12, 16])
def test_rho_edge_cases(p):
    slot = cover_ref.slot
    assert slot(0, p) == (0, 64 - p + 1)                              # w = 0: the cap, plus one
    assert slot(M64, p) == ((1 << p) - 1, 1)                          # top bit of w set
    assert slot(1 << (63 - p), p) == (0, 1)                           # the first bit below the index
    assert slot(1, p) == (0, 64 - p)                                  # the last bit: 63 - p leading zeros
    assert slot((5 << (64 - p)) | 1, p) == (5 % (1 << p), 64 - p)     # the index bits do not leak into w
    for z in range(64 - p):
        assert slot(1 << (63 - p - z), p)[1] == z + 1
    assert max(slot(u, p)[1] for u in (0, 1, 2, 3)) == 64 - p + 1 <= 61   # a register always fits a byte


def test_sketch_counts_and_keeps_the_maximum():
    sk = cover_ref.Sketch(2, 4)
    hashes = [random.Random(1).getrandbits(64) for _ in range(3)]
    for h in hashes + hashes:                                         # duplicates count in matched, not in the registers
        sk.add_hash(1, h)
    assert sk.matched == [0, 6] and sk.registers[0] == [0] * 16
    want = [0] * 16
    for h in hashes:
        j, rho = cover_ref.slot(cover_ref.mix(h), 4)
        want[j] = max(want[j], rho)
    assert sk.registers[1] == want


def test_sketch_is_independent_of_order_and_splitting():
    rng = random.Random(7)
    items = [(rng.randrange(3), rng.getrandbits(64)) for _ in range(4000)]
    items += items[:500]                                              # duplicates included

    def sketch(seq):
        sk = cover_ref.Sketch(3, 8)
        for l, h in seq:
            sk.add_hash(l, h)
        return sk
    whole = sketch(items)
    rev = sketch(items[::-1])
    shuffled = items[:]
    rng.shuffle(shuffled)
    parts = [sketch(shuffled[:700]), sketch(shuffled[700:701]), sketch(shuffled[701:])]
    merged = cover_ref.Sketch(3, 8)
    for part in parts[::-1]:
        merged.absorb(part)
    for other in (rev, merged):
        assert other.registers == whole.registers and other.matched == whole.matched


def test_absorb_is_the_elementwise_maximum():
    rng = random.Random(11)
    a, b = cover_ref.Sketch(2, 5), cover_ref.Sketch(2, 5)
    for sk, n in ((a, 40), (b, 90)):
        for _ in range(n):
            sk.add_hash(rng.randrange(2), rng.getrandbits(64))
        sk.units = [rng.randrange(100), rng.randrange(100)]
        sk.n_units = sum(sk.units)
    ra, rb = [r[:] for r in a.registers], [r[:] for r in b.registers]
    ua, ma, na = a.units[:], a.matched[:], a.n_units
    a.absorb(b)
    assert a.registers == [[max(x, y) for x, y in zip(r, s)] for r, s in zip(ra, rb)]
    assert a.units == [x + y for x, y in zip(ua, b.units)] and a.matched == [x + y for x, y in zip(ma, b.matched)]
    assert a.n_units == na + b.n_units
    with pytest.raises(AssertionError):
        a.absorb(cover_ref.Sketch(2, 6))


def test_estimator_by_hand():
    assert cover_ref.estimate([0] * 16, 4) == 0.0
    # one register set out of 16: the small-range branch, 16 ln(16 / 15)
    assert cover_ref.estimate([3] + [0] * 15, 4) == pytest.approx(16 * math.log(16 / 15), rel=1e-15)
    # no register empty: the raw estimate alpha m^2 / sum 2^-R
    assert cover_ref.estimate([2] * 16, 4) == pytest.approx(0.673 * 256 / (16 * 0.25), rel=1e-15)
    assert cover_ref.alpha(5) == 0.697 and cover_ref.alpha(6) == 0.709
    assert cover_ref.alpha(12) == pytest.approx(0.7213 / (1 + 1.079 / 4096), rel=1e-15)
    assert cover_ref.genome_kmers(1000, 4, 1000) == 0.0 and cover_ref.genome_kmers(1000, 4, 0) == 0.0
    assert cover_ref.genome_kmers(1000, 4, 330) == pytest.approx(-250 * math.log(0.67), rel=1e-12)


@pytest.mark.parametrize("n", [50, 1980, 10240, 60000])
def test_estimator_accuracy(n):
    """Within 4 standard errors, 4 * 1.04 / sqrt(m) = 6.5 % at p = 12, of the exact cardinality: below, at and above the
    switch between the estimator's two branches (2.5 m = 10 240).  The seed is fixed, so this is deterministic."""
    p = 12
    rng = random.Random(20261017)
    hashes = set()
    while len(hashes) < n:
        hashes.add(rng.getrandbits(64))
    sk = cover_ref.Sketch(1, p)
    for h in hashes:
        sk.add_hash(0, h)
        sk.add_hash(0, h)                                             # seen twice: the estimate is of the distinct ones
    est = sk.distinct()[0]
    bound = 4 * 1.04 / math.sqrt(1 << p)
    print(f"n = {n}: estimate {est:.1f}, relative error {est / n - 1:+.4f}, bound {bound:.4f}")
    assert sk.matched == [2 * n] and abs(est / n - 1) <= bound


# ---- CLI: option errors before any device is opened

def run(tmp_path, *extra):
    out = tmp_path / "out"
    p = subprocess.run([CLI, "query", "-r", FASTQ, "-o", str(out), "-d", str(tmp_path / "no_db"), "--devices", "all", *extra],
                       capture_output=True, text=True, timeout=60)
    assert not out.exists(), extra
    return p


@pytest.mark.parametrize("extra,msg", [
    (["--coverage-precision", "12"], "'--coverage-precision' needs '--coverage'"),
    (["--coverage-precision", "12", "--scores"], "'--coverage-precision' needs '--coverage'"),
    (["--coverage", "--coverage-precision", "3"], "invalid value '3' for '--coverage-precision'"),
    (["--coverage", "--coverage-precision", "17"], "invalid value '17' for '--coverage-precision'"),
    (["--coverage", "--coverage-precision", "x"], "invalid value 'x' for '--coverage-precision'"),
    (["--coverage", "--coverage-precision", "-4"], "invalid value '-4' for '--coverage-precision'"),
])
def test_coverage_option_errors_before_any_device(tmp_path, extra, msg):
    p = run(tmp_path, *extra)
    assert p.returncode == 101 and msg in p.stderr, (extra, p.stderr)
    assert "libpfq" not in p.stderr, p.stderr                       # no library call answered first


def test_coverage_precision_needs_a_value(tmp_path):
    p = run(tmp_path, "--coverage", "--coverage-precision")
    assert p.returncode == 101 and "value is required" in p.stderr, p.stderr


def test_usage_lists_coverage_options():
    p = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert "--coverage:" in p.stderr and "--coverage-precision <P>" in p.stderr and "COVERAGE.tsv" in p.stderr
    assert "distinct_kmers" in p.stderr and "breadth" in p.stderr
