"""`phage_filter recluster` and `build --cluster` on the example genomes: a query gives the same answers on the old and the new
database, MERGES.tsv equals the text tests/cluster_ref.py makes of the old database read back, and `build --cluster` writes what
`build` followed by `recluster` writes, byte for byte."""
import collections
import os
import subprocess

import pytest

import cluster_ref as cr
from oracle import pfq_format as fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "examples")
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(EX, "reads", "sim_reads_c10000_n5_e0.01.fq")
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
TIMEOUT = 300
BUILD = ["build", "--genomes", os.path.join(EX, "genomes"), "--seed1", str(SEEDS[0]), "--seed2", str(SEEDS[1])]


def run(args, cwd):
    p = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=TIMEOUT, cwd=str(cwd))
    assert p.returncode == 0, (args, p.stderr)
    return p.stdout


def files_of(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def dbs(gpu, tmp_path_factory):
    """two/db0 by `build`, two/db by `recluster` of it (with --merges), one/db by `build --cluster`: both db are named alike
    relative to the directory the command runs in, because a .bf file records the path it was saved under."""
    base = tmp_path_factory.mktemp("recluster_cli")
    one, two = base / "one", base / "two"
    one.mkdir()
    two.mkdir()
    run(BUILD + ["--db-path", "db0"], two)
    out = run(["recluster", "-d", "db0", "-o", "db", "--merges", "MERGES.tsv"], two)
    run(BUILD + ["--db-path", "db", "--cluster"], one)
    return one, two, out


def test_merges_tsv_and_the_new_database(dbs):
    _, two, out = dbs
    ot = fmt.read_db(str(two / "db0"))
    nt, log, rounds, names = cr.recluster(ot)
    assert open(two / "MERGES.tsv").read() == cr.merges_tsv(log, names)
    n = len(ot.leaves_dfs())
    assert f"Reclustered {n} genomes in {rounds} rounds" in out
    new = fmt.read_db(str(two / "db"))
    assert cr.clade_table(new) == cr.clade_table(nt) and new.n_nodes == 2 * n - 1
    old_files, new_files = files_of(two / "db0"), files_of(two / "db")
    for v in ot.leaves_dfs():                                                 # the leaves' filter words: byte-identical
        a, b = old_files[ot.bf_path[v]], new_files[ot.bf_path[v]]
        words = 8 * ot.n_words
        head = a.index(b"bitvec::order::Lsb0") + len(b"bitvec::order::Lsb0") + 2 + 16
        assert a[:head + words] == b[:head + words]


def test_build_cluster_equals_build_then_recluster(dbs):
    one, two, _ = dbs
    a, b = files_of(one / "db"), files_of(two / "db")
    assert sorted(a) == sorted(b) and "tree.bin" in a and len(a) == 2 * 12
    for f in a:
        assert a[f] == b[f], f


def normal(data):
    """POS / NEG records as a multiset of lines, the genome list behind " |" sorted (its order is unspecified)."""
    lines = []
    for ln in data.decode().splitlines():
        if " |" in ln:
            head, _, gs = ln.rpartition(" |")
            ln = head + " |" + ",".join(sorted(gs.split(",")))
        lines.append(ln)
    return collections.Counter(lines)


@pytest.mark.parametrize("thr", ["1.0", "0.3"])
def test_query_gives_the_same_answers(dbs, tmp_path, thr):
    _, two, _ = dbs
    got = {}
    for name in ("db0", "db"):
        out = str(tmp_path / name)
        run(["query", "--out", out, "--db-path", str(two / name), "--reads", FASTQ, "--filter-threshold", thr, "--pos-filter", "--neg-filter"], tmp_path)
        got[name] = files_of(out)
    old, new = got["db0"], got["db"]
    assert sorted(old) == sorted(new) and len(old) == 3
    assert sorted(old["CLASSIFICATION.csv"].splitlines()) == sorted(new["CLASSIFICATION.csv"].splitlines()) and old["CLASSIFICATION.csv"]
    for f in old:
        if f != "CLASSIFICATION.csv":
            assert normal(old[f]) == normal(new[f]), f
