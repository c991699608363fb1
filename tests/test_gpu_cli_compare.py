"""`phage_filter compare`: SIMILARITY.tsv against tests/sim_ref.py over the database the CLI's own `build` makes of the twelve
example genomes, read back through oracle/pfq_format.py.  Names and integer columns are compared exactly; the printed doubles
with the reference's to the digits printed.  --min-containment must write exactly the reference's subset, --against every pair of
two databases, and two databases that cannot be compared are refused with status 101."""
import os
import shutil
import subprocess

import pytest

import sim_ref
from oracle import pfq_format as fmt
from test_gpu_cli_lca import CLI, EX, SEEDS, TIMEOUT

pytestmark = pytest.mark.gpu

GENOMES = os.path.join(EX, "genomes")
DIGITS = (1, 1, 1, 6, 6, 6, 6)                                               # kmers_a, kmers_b, shared_kmers | jaccard, containments, ani


def build(db, genomes, seeds=SEEDS):
    """`build` draws its two hash seeds at random unless --seed1 / --seed2 fix them: that is how two databases get equal seeds."""
    p = subprocess.run([CLI, "build", "--genomes", genomes, "--db-path", db, "--seed1", str(seeds[0]), "--seed2", str(seeds[1])],
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    ot = fmt.read_db(db)
    return ot, [ot.tax_id[v] for v in ot.leaves_dfs()]


def compare(db, out, *args, status=0):
    p = subprocess.run([CLI, "compare", "-d", db, "-o", out, *args], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == status, (p.returncode, p.stderr)
    if status:
        return p.stderr, None
    assert sorted(os.listdir(out)) == ["SIMILARITY.tsv"]
    lines = open(os.path.join(out, "SIMILARITY.tsv"), "rb").read().decode().split("\n")
    assert lines[-1] == "" and lines[0] == sim_ref.HEADER
    return p.stdout, [l.split("\t") for l in lines[1:-1]]


def check_lines(got, ref, names_a, names_b, pairs, k):
    """The lines of SIMILARITY.tsv against the reference's for `pairs`, in order."""
    assert [(g[0], g[1]) for g in got] == [(names_a[i], names_b[j]) for i, j in pairs]
    for g, (i, j) in zip(got, pairs):
        assert len(g) == 12
        ints, floats = sim_ref.pair_values(ref, i, j, k)
        assert tuple(int(x) for x in g[2:5]) == ints, (g, ints)
        for text, w, digits in zip(g[5:], floats, DIGITS):
            # what rounding to the printed digits may do, the doubles' own 1e-9 relative, and 2e-6
            assert len(text.split(".")[1]) == digits and abs(float(text) - w) <= 0.5 * 10 ** -digits + 1e-9 * abs(w) + 2e-6, (g, floats)


@pytest.fixture(scope="module")
def examples(gpu, tmp_path_factory):
    db = str(tmp_path_factory.mktemp("compare_cli") / "db")
    ot, names = build(db, GENOMES)
    assert len(names) == 12
    return db, ot, names, sim_ref.similarity(ot)


def test_all_pairs_of_the_examples(examples, tmp_path):
    db, ot, names, ref = examples
    pairs = [(i, j) for i in range(12) for j in range(i + 1, 12)]
    out = str(tmp_path / "out")
    os.makedirs(os.path.join(out, "stale"))                                  # an existing directory is replaced
    stdout, got = compare(db, out, "--min-containment", "0")
    assert len(got) == 66
    check_lines(got, ref, names, names, pairs, ot.kmer_size)
    assert "66 pairs compared" in stdout and "66 written" in stdout and "12 x 12" in stdout


def test_min_containment_writes_the_reference_subset(examples, tmp_path):
    db, ot, names, ref = examples
    pairs = [(i, j) for i in range(12) for j in range(i + 1, 12)]
    val = {p: sim_ref.max_containment(ref, *p, ot.kmer_size) for p in pairs}
    s = sorted(val.values())
    gap, at = max((s[n + 1] - s[n], n) for n in range(len(s) - 1))
    c = (s[at] + s[at + 1]) / 2                                              # the midpoint of the two most separated adjacent values
    assert gap > 1e-5 and all(abs(v - c) > 1e-6 for v in s) and 0.0 < c < 1.0
    keep = [p for p in pairs if val[p] >= c]
    assert 0 < len(keep) < 66
    stdout, got = compare(db, str(tmp_path / "out"), "--min-containment", repr(c))
    check_lines(got, ref, names, names, keep, ot.kmer_size)
    assert "66 pairs compared" in stdout and f"{len(keep)} written" in stdout
    # the default is 0.1
    _, got = compare(db, str(tmp_path / "out_default"))
    check_lines(got, ref, names, names, [p for p in pairs if val[p] >= 0.1], ot.kmer_size)


def test_against_a_second_database(examples, tmp_path):
    db, ot, names, _ = examples
    files = sorted(os.listdir(GENOMES))
    four = tmp_path / "four"
    four.mkdir()
    for f in (files[7], files[0], files[10], files[3]):
        shutil.copy(os.path.join(GENOMES, f), str(four / f))
    db2 = str(tmp_path / "db2")
    ot2, names2 = build(db2, str(four))                                      # the same -k, -f, -l (the defaults) and the same seeds
    assert len(names2) == 4 and set(names2) <= set(names)
    ref = sim_ref.similarity(ot, ot2)
    pairs = [(i, j) for i in range(12) for j in range(4)]
    stdout, got = compare(db, str(tmp_path / "out"), "--against", db2, "--min-containment", "0")
    assert len(got) == 48 and "48 pairs compared" in stdout and "12 x 4" in stdout
    check_lines(got, ref, names, names2, pairs, ot.kmer_size)
    twins = [g for g in got if g[0] == g[1]]
    assert len(twins) == 4 and all(g[8:11] == ["1.000000"] * 3 and g[2] == g[3] == g[4] for g in twins)
    # the other way round, thresholded: the four identical pairs are among the lines
    _, back = compare(db2, str(tmp_path / "back"), "--against", db, "--min-containment", "0.999")
    assert [(g[0], g[1]) for g in back if g[0] == g[1]] == [(n, n) for n in names2]


def test_mismatched_databases_are_refused(examples, tmp_path):
    db, _, _, _ = examples
    one = tmp_path / "one"
    one.mkdir()
    f = sorted(os.listdir(GENOMES))[0]
    shutil.copy(os.path.join(GENOMES, f), str(one / f))
    db2 = str(tmp_path / "db2")
    build(db2, str(one), seeds=(SEEDS[0], SEEDS[1] + 1))
    out = str(tmp_path / "out")
    err, _ = compare(db, out, "--against", db2, status=101)
    assert "seed2" in err and not os.path.exists(out), err
