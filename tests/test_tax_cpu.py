"""The taxonomy file, the node table and the argument checks of `phage_filter taxonomy` / `query --taxonomy`, all without a
device: only tree.bin and the file are read.  The expected tables come from tests/tax_ref.py, the model in plain Python; the
database is written with the oracle's greedy build and oracle/pfq_format."""
import os
import subprocess

import pytest

import tax_ref
from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import PfqError, read_taxonomy
from phagefilter_amd.query import db_leaf_ids, taxonomy_nodes
from test_shard_count_cpu import greedy_genomes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
EX = os.path.join(ROOT, "tests", "golden", "examples")
PFQ_ERR_ARG, PFQ_ERR_IO, PFQ_ERR_FORMAT = -1, -2, -3


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    d = tmp_path_factory.mktemp("taxdb") / "db"
    genomes, ids = greedy_genomes()
    t = orc.build_greedy_tree(genomes, ids, 15, 0.01, 2000, 5, 10)
    fmt.write_db(t, str(d))
    leaf_ids = [t.tax_id[v] for v in t.leaves_dfs()]
    assert sorted(leaf_ids) == sorted(ids) and leaf_ids != ids         # the leaf order is the tree's, not the input's
    return str(d), leaf_ids


# file -> what it exercises.  The database's genomes are g0 .. g10.
FILES = {
    "nested": b"g0\tA;B;C\ng1\tA;B;C\ng2\tA;B\ng3\tA;D\ng4\tA\ng5\tE;F\ng6\tE;F\ng7\tE\ng8\tA;B;C\ng9\tG\ng10\tA;D\n",
    "missing_genomes": b"g3\tA;B\ng7\tA\n",
    "extra_genomes": b"x1\tZ;Y\ng0\tA\nx2\tA;Q\ng1\tA;B\nx3\t\n" + b"".join(b"g%d\tA;B\n" % i for i in range(2, 11)),
    # Z;Y and A;Q are named by absent genomes only: no such taxon exists; W holds genomes only through W;V
    "absent_taxon": b"x1\tZ;Y\ng0\tW;V\nx2\tW;U\ng1\tW;V\n",
    "same_name_two_parents": b"g0\tA;X\ng1\tB;X\ng2\tA;X\ng3\tB;X\ng4\tX\ng5\tX;X\n",
    "one_child_chains": b"".join(b"g%d\tR1;R2;R3;%s\n" % (i, b"P;Q;S" if i % 2 else b"T") for i in range(11)),
    "empty_lineage": b"g0\t\ng1\t  \ng2\tA\ng3\t\tignored\n",
    "crlf_comments_columns": b"# a comment\r\n\r\ng0\tA; B ;C\tNC_1\t3\r\n#g1\tZ\r\ng1\tA;B\r\n\ng2\t A\r\ng3\tA;B;C",
    "same_lineage_twice": b"g0\tA;B\ng0\tA; B\ng1\tA\n",
}


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)


def read_tsv(path):
    rows = [line.split("\t") for line in open(path).read().splitlines()]
    assert rows[0] == ["#node", "parent", "depth", "kind", "genomes", "name"]
    return rows[1:]


@pytest.mark.parametrize("name", sorted(FILES))
def test_taxonomy_command_and_read_taxonomy_equal_the_reference(db, tmp_path, name):
    d, leaf_ids = db
    assert db_leaf_ids(d) == leaf_ids
    f = tmp_path / "tax.tsv"
    f.write_bytes(FILES[name])
    parent, names, leaf_taxon, info = tax_ref.parse(FILES[name], leaf_ids)
    ref = tax_ref.Nodes(leaf_ids, parent, names, leaf_taxon)
    # the Python reader and the node table it leads to
    assert read_taxonomy(str(f), leaf_ids) == (parent, names, leaf_taxon)
    assert taxonomy_nodes(leaf_ids, parent, names, leaf_taxon) == ref.table
    # the command
    out = tmp_path / "out"
    p = run(["taxonomy", "-d", d, "--taxonomy", str(f), "-o", str(out)])
    assert p.returncode == 0, p.stderr
    want = [[str(v), "-" if r[0] < 0 else str(r[0]), str(r[1]), "genome" if r[4] >= 0 else "taxon", str(r[3]), r[5]] for v, r in enumerate(ref.table)]
    assert read_tsv(out / "TAXA.tsv") == want
    assert f"{info['lines_other']} lines for genomes that are not in the database" in p.stderr
    assert f"{info['leaves_without_line']} of {len(leaf_ids)} genomes without a line" in p.stderr


def test_what_the_files_exercise(db):
    """Asserted on the reference alone: the files do contain the shapes their names promise."""
    _, leaf_ids = db

    def nodes(name):
        parent, names, leaf_taxon, info = tax_ref.parse(FILES[name], leaf_ids)
        return tax_ref.Nodes(leaf_ids, parent, names, leaf_taxon), names, info
    n, names, info = nodes("nested")
    assert max(r[1] for r in n.table) == 4 and info["leaves_without_line"] == 0
    assert [n.rank[l] for l in range(len(leaf_ids))] != list(range(len(leaf_ids)))
    n, names, info = nodes("missing_genomes")
    assert info["leaves_without_line"] == 9 and sum(1 for r in n.table if r[0] == 0 and r[4] >= 0) == 9
    n, names, info = nodes("extra_genomes")
    assert info["lines_other"] == 3 and "Z" not in names and "Q" not in names
    n, names, info = nodes("absent_taxon")
    assert names == ["root", "W", "V"] and info["lines_other"] == 2
    n, names, info = nodes("same_name_two_parents")
    assert names.count("X") == 4 and len({v for v, r in enumerate(n.table) if r[5] == "X"}) == 4
    n, names, info = nodes("one_child_chains")
    assert [r[3] for r in n.table[:4]] == [11, 11, 11, 11] and n.table[4][3] < 11         # root - R1 - R2 - R3, then the split
    n, names, info = nodes("empty_lineage")
    assert [n.table[n.leaf_node[leaf_ids.index(g)]][0] for g in ("g0", "g1", "g3")] == [0, 0, 0]
    n, names, info = nodes("crlf_comments_columns")
    assert names == ["root", "A", "B", "C"] and info["lines_considered"] == 4


def test_a_taxon_without_genomes_is_dropped_and_argument_errors(db):
    _, leaf_ids = db
    parent, names = [-1, 0, 0, 2, 1], ["root", "empty", "full", "empty_below_full", "empty_too"]
    leaf_taxon = [2] * len(leaf_ids)
    ref = tax_ref.Nodes(leaf_ids, parent, names, leaf_taxon)
    got = taxonomy_nodes(leaf_ids, parent, names, leaf_taxon)
    assert got == ref.table and [r[5] for r in got if r[4] < 0] == ["root", "full"]
    for bad_parent, bad_leaf in (([-1, 1, 0, 2, 1], leaf_taxon), ([-1, 0, 0, 3, 1], leaf_taxon), ([0, 0, 0, 2, 1], leaf_taxon),
                                 (parent, [5] + leaf_taxon[1:]), ([], [])):
        with pytest.raises(PfqError) as e:
            taxonomy_nodes(leaf_ids if bad_leaf else [], bad_parent, names[:len(bad_parent)], bad_leaf)
        assert e.value.code == PFQ_ERR_ARG, (bad_parent, bad_leaf)


ERRORS = {
    "one_field": (b"g0\tA\n# fine\n\ng1\n", 4),
    "one_field_absent_genome": (b"g0\tA\nnot_in_db\n", 2),
    "empty_name_inside": (b"g0\tA;;B\n", 1),
    "empty_name_at_the_end": (b"g0\tA\r\ng1\tA;B;\r\n", 2),
    "empty_name_spaces": (b"g0\tA\ng1\tA\ng2\tA; ;B\n", 3),
    "two_lineages": (b"g0\tA;B\ng1\tA\ng0\tA\n", 3),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_file_errors_give_status_101_and_name_the_line(db, tmp_path, name):
    d, leaf_ids = db
    data, line = ERRORS[name]
    with pytest.raises(tax_ref.TaxFileError) as r:
        tax_ref.parse(data, leaf_ids)
    assert r.value.line == line
    f = tmp_path / "tax.tsv"
    f.write_bytes(data)
    with pytest.raises(PfqError) as e:
        read_taxonomy(str(f), leaf_ids)
    assert e.value.code == PFQ_ERR_FORMAT and f"line {line}:" in str(e.value)
    p = run(["taxonomy", "-d", d, "--taxonomy", str(f), "-o", str(tmp_path / "out")])
    assert p.returncode == 101 and f"line {line}:" in p.stderr, p.stderr
    assert not (tmp_path / "out").exists()
    # query checks the file before any device is used
    p = run(["query", "--reads", os.path.join(EX, "reads"), "--out", str(tmp_path / "q"), "--db-path", d, "--taxonomy", str(f)])
    assert p.returncode == 101 and f"line {line}:" in p.stderr and p.stdout == "", (p.stdout, p.stderr)
    assert not (tmp_path / "q").exists()


def test_missing_files(db, tmp_path):
    d, leaf_ids = db
    with pytest.raises(PfqError) as e:
        read_taxonomy(str(tmp_path / "nope.tsv"), leaf_ids)
    assert e.value.code == PFQ_ERR_IO
    p = run(["taxonomy", "-d", d, "--taxonomy", str(tmp_path / "nope.tsv"), "-o", str(tmp_path / "out")])
    assert p.returncode == 101 and "nope.tsv" in p.stderr
    f = tmp_path / "tax.tsv"
    f.write_bytes(FILES["nested"])
    p = run(["taxonomy", "-d", str(tmp_path / "nodb"), "--taxonomy", str(f), "-o", str(tmp_path / "out")])
    assert p.returncode == 101 and "tree.bin" in p.stderr
    with pytest.raises(PfqError) as e:
        db_leaf_ids(str(tmp_path / "nodb"))
    assert e.value.code == PFQ_ERR_IO


def test_query_refusals_without_a_device(db, tmp_path):
    d, _ = db
    f = tmp_path / "tax.tsv"
    f.write_bytes(FILES["nested"])
    q = ["query", "--reads", os.path.join(EX, "reads"), "--out", str(tmp_path / "q"), "--db-path", d]
    for extra, words in ((["--taxon-reads"], ["--taxon-reads", "needs", "--taxonomy"]),
                         (["--taxonomy", str(f), "--shard-depth", "1"], ["--taxonomy", "--shard-depth"]),
                         (["--taxonomy", str(f), "--frame", "100"], ["--taxonomy", "--frame"]),
                         (["--taxonomy", str(f), "--device-parse"], ["--taxonomy", "--device-parse"]),
                         (["--taxonomy", str(tmp_path / "nope.tsv")], ["nope.tsv"])):
        p = run(q + extra)
        assert p.returncode == 101 and all(w in p.stderr for w in words) and p.stdout == "", (extra, p.stdout, p.stderr)
        assert not (tmp_path / "q").exists()
