"""`phage_filter query --coverage`: COVERAGE.tsv against tests/cover_ref.py over the oracle's hit rows, on the database the
CLI's own `build` makes of the example genomes.  The integer columns are compared exactly, `units` also with
CLASSIFICATION.csv; the derived columns with the reference's doubles to the digits printed.  Every other output must be
byte-identical to the run without --coverage; --reads2 sketches fragments; two replicas on one device, merged before
writing, and the subtree shards of depth 2 must give the file the whole tree on one replica gives."""
import os
import subprocess

import pytest

import cover_ref
from oracle import pfq_format as fmt
from test_gpu_cli_lca import CLI, EX, FASTQ, SEEDS, TIMEOUT, fastq_records, query, write_fasta
from test_gpu_lca import oracle_sets
from test_gpu_paired import combine, mate_sets

pytestmark = pytest.mark.gpu

HEADER = "#genome\tunits\tmatched_kmers\tdistinct_kmers\tgenome_kmers\tbreadth\tduplication"


@pytest.fixture(scope="module")
def examples(gpu, tmp_path_factory):
    db = str(tmp_path_factory.mktemp("cover_cli") / "db")
    p = subprocess.run([CLI, "build", "--genomes", os.path.join(EX, "genomes"), "--db-path", db, "--seed1", str(SEEDS[0]),
                        "--seed2", str(SEEDS[1])], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    ot = fmt.read_db(db)
    cache = cover_ref.TreeSketcher(ot)                                       # (the oracle's answers, shared by the cases)
    return db, ot, [ot.tax_id[v] for v in ot.leaves_dfs()], fastq_records(FASTQ), cache


def check_tsv(data, ref, names, classification=None):
    """COVERAGE.tsv against the reference sketcher `ref`: one line per leaf in leaf order."""
    sk = ref.sk
    lines = data.decode().split("\n")
    assert lines[-1] == "" and lines[0] == HEADER
    got = [l.split("\t") for l in lines[1:-1]]
    assert [g[0] for g in got] == names and all(len(g) == 7 for g in got)
    assert [int(g[1]) for g in got] == sk.units and [int(g[2]) for g in got] == sk.matched
    for g, d, n, m in zip(got, sk.distinct(), ref.genome_kmers(), sk.matched):
        want = (d, n, d / n if n > 0 else 0.0, m / d if d > 0 else 0.0)
        for text, w, digits in zip(g[3:], want, (1, 1, 4, 2)):
            assert len(text.split(".")[1]) == digits and abs(float(text) - w) <= 0.5 * 10 ** -digits + 1e-9 * abs(w), (g, want)
    if classification is not None:                                           # "<tax_id>,<count>" for count > 0
        counts = dict(l.split(",") for l in classification.decode().split("\n") if l)
        assert {g[0]: g[1] for g in got if g[1] != "0"} == counts
    return sk


def test_examples_database(examples, tmp_path):
    db, ot, names, recs, cache = examples
    thr = "0.7"
    reads = [s for _, s in recs]
    rows = [sorted(s) for s in oracle_sets(ot, reads, float(thr))]
    ref = cover_ref.TreeSketcher(ot, share=cache).add_reads(rows, reads)
    assert sum(1 for u in ref.sk.units if u) >= 2 and any(0 < m < (100 - ot.kmer_size + 1) * u for m, u in zip(ref.sk.matched, ref.sk.units))
    r = ["--reads", FASTQ]
    # alone (what would be the counts-only mode) and with every other per-read output
    out0, plain = query(db, str(tmp_path / "p0"), *r, thr=thr)
    out1, got = query(db, str(tmp_path / "c0"), *r, "--coverage", thr=thr)
    check_tsv(got.pop("COVERAGE.tsv"), ref, names, got["CLASSIFICATION.csv"])
    assert got == plain and out1 == out0
    extra = ["--pos-filter", "--neg-filter", "--scores", "--lca", "all", "--abundance"]
    out0, plain = query(db, str(tmp_path / "p1"), *r, *extra, thr=thr)
    out1, got = query(db, str(tmp_path / "c1"), *r, *extra, "--coverage", thr=thr)
    whole = got.pop("COVERAGE.tsv")
    check_tsv(whole, ref, names, got["CLASSIFICATION.csv"])
    assert got == plain and out1 == out0 and len(plain) == 6
    # two replicas on one device, merged before writing
    _, two = query(db, str(tmp_path / "d2"), *r, "--coverage", "--pos-filter", "--devices", "0,0", thr=thr, threads="3", block="17")
    assert two["COVERAGE.tsv"] == whole and two["CLASSIFICATION.csv"] == plain["CLASSIFICATION.csv"]
    # subtree shards: the shards' lines one after the other
    _, sh = query(db, str(tmp_path / "s2"), *r, "--coverage", "--shard-depth", "2", thr=thr)
    assert sh["COVERAGE.tsv"] == whole and sh["CLASSIFICATION.csv"] == plain["CLASSIFICATION.csv"]


def test_threshold_one_and_precision(examples, tmp_path):
    db, ot, names, recs, cache = examples
    reads = [s for _, s in recs]
    rows = [sorted(s) for s in oracle_sets(ot, reads, 1.0)]
    _, plain = query(db, str(tmp_path / "p"), "--reads", FASTQ)
    for p in (12, 6):
        ref = cover_ref.TreeSketcher(ot, p, share=cache).add_reads(rows, reads)
        extra = [] if p == 12 else ["--coverage-precision", str(p)]
        _, got = query(db, str(tmp_path / f"c{p}"), "--reads", FASTQ, "--coverage", *extra)
        check_tsv(got.pop("COVERAGE.tsv"), ref, names, got["CLASSIFICATION.csv"])
        assert got == plain


@pytest.mark.parametrize("pair_mode", ["either", "both"])
def test_reads2_sketches_fragments(examples, tmp_path, pair_mode):
    db, ot, names, recs, cache = examples
    recs = recs[:600]
    pairs = [(recs[2 * i][1], recs[2 * i + 1][1]) for i in range(len(recs) // 2)]
    r1 = write_fasta(tmp_path / "r1.fa", [(f"f{i}/1", p[0]) for i, p in enumerate(pairs)])
    r2 = write_fasta(tmp_path / "r2.fa", [(f"f{i}/2", p[1]) for i, p in enumerate(pairs)])
    thr = "0.5"
    frag = [sorted(s) for s in combine(mate_sets(ot, [m for p in pairs for m in p], float(thr)), pair_mode)]
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    ref = cover_ref.TreeSketcher(ot, share=cache).add_pairs(frag, pairs)
    assert ref.sk.n_units == len(pairs) and sum(ref.sk.units) > 0
    src = ["--reads", r1, "--reads2", r2, "--pair-mode", pair_mode]
    _, plain = query(db, str(tmp_path / "p"), *src, "--pos-filter", "--neg-filter", thr=thr)
    _, got = query(db, str(tmp_path / "c"), *src, "--pos-filter", "--neg-filter", "--coverage", thr=thr)
    whole = got.pop("COVERAGE.tsv")
    check_tsv(whole, ref, names, got["CLASSIFICATION.csv"])
    assert got == plain
    _, two = query(db, str(tmp_path / "d"), *src, "--coverage", "--devices", "0,0", thr=thr, block="16")
    assert sorted(two) == ["CLASSIFICATION.csv", "COVERAGE.tsv"] and two["COVERAGE.tsv"] == whole
    assert two["CLASSIFICATION.csv"] == plain["CLASSIFICATION.csv"]
