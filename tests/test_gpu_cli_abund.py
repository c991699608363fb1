"""`phage_filter query --abundance`: ABUNDANCE.tsv must equal the text built here from the oracle's hit rows (orc.query_batch)
and the plain-Python estimate of tests/abund_ref.py, on the database the CLI's own `build` makes of the example genomes;
CLASSIFICATION.csv and the POS / NEG files must be byte-identical to the run without --abundance; --reads2 logs fragments;
two replicas on one device, merged before the estimate, must give the file one replica gives."""
import os
import subprocess

import pytest

import abund_ref
from oracle import pfq_format as fmt
from test_gpu_cli_lca import CLI, EX, FASTQ, SEEDS, TIMEOUT, fastq_records, query, write_fasta
from test_gpu_lca import oracle_sets
from test_gpu_paired import combine, mate_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def examples(gpu, tmp_path_factory):
    db = str(tmp_path_factory.mktemp("abund_cli") / "db")
    p = subprocess.run([CLI, "build", "--genomes", os.path.join(EX, "genomes"), "--db-path", db, "--seed1", str(SEEDS[0]),
                        "--seed2", str(SEEDS[1])], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    ot = fmt.read_db(db)
    return db, ot, [ot.tax_id[v] for v in ot.leaves_dfs()], fastq_records(FASTQ)


def check_tsv(data, sets, names, iters=200):
    """ABUNDANCE.tsv against the estimate over `sets`: header and totals exactly, unique and estimated as strings, fraction
    to 1e-6."""
    est = abund_ref.estimate(abund_ref.classify([sorted(s) for s in sets], len(names)), iters, 65)
    lines = data.decode().split("\n")
    assert lines[-1] == "" and lines[0] == "#genome\tunique\testimated\tfraction"
    assert lines[1] == (f"#units={est['n_units']} unhit={est['n_unhit']} unique={est['n_unique']} ambiguous={est['n_ambiguous']} "
                        f"all_leaves={est['n_all_leaves']} iterations={est['iterations']} converged={est['converged']}")
    want = abund_ref.tsv_lines(est, names)
    got = [l.split("\t") for l in lines[2:-1]]
    assert len(want) >= 2 and [g[:3] for g in got] == [list(w[:3]) for w in want]
    for g, w in zip(got, want):
        assert len(g) == 4 and len(g[3].split(".")[1]) == 6 and abs(float(g[3]) - w[3]) <= 1e-6, (g, w)
    return est


@pytest.mark.parametrize("thr", ["1.0", "0.3"])
def test_examples_database(examples, tmp_path, thr):
    db, ot, names, recs = examples
    sets = oracle_sets(ot, [s for _, s in recs], float(thr))
    r = ["--reads", FASTQ]
    # alone (what would be the counts-only mode) and with every other per-read output
    out0, plain = query(db, str(tmp_path / "p0"), *r, thr=thr)
    out1, got = query(db, str(tmp_path / "a0"), *r, "--abundance", thr=thr)
    est = check_tsv(got.pop("ABUNDANCE.tsv"), sets, names)
    assert est["n_ambiguous"] + est["n_unique"] > 0
    assert got == plain and out1 == out0
    extra = ["--pos-filter", "--neg-filter", "--scores", "--lca", "all"]
    out0, plain = query(db, str(tmp_path / "p1"), *r, *extra, thr=thr)
    out1, got = query(db, str(tmp_path / "a1"), *r, *extra, "--abundance", thr=thr)
    check_tsv(got.pop("ABUNDANCE.tsv"), sets, names)
    assert got == plain and out1 == out0 and len(plain) == 5
    # --abundance-iters
    _, got = query(db, str(tmp_path / "a2"), *r, "--abundance", "--abundance-iters", "2", thr=thr)
    check_tsv(got["ABUNDANCE.tsv"], sets, names, iters=2)
    # two replicas on one device
    _, one = query(db, str(tmp_path / "d1"), *r, "--abundance", "--pos-filter", thr=thr)
    _, two = query(db, str(tmp_path / "d2"), *r, "--abundance", "--pos-filter", "--devices", "0,0", thr=thr, threads="3", block="17")
    check_tsv(two["ABUNDANCE.tsv"], sets, names)
    assert two["ABUNDANCE.tsv"] == one["ABUNDANCE.tsv"] and two["CLASSIFICATION.csv"] == one["CLASSIFICATION.csv"]


@pytest.mark.parametrize("pair_mode", ["either", "both"])
def test_reads2_logs_fragments(examples, tmp_path, pair_mode):
    db, ot, names, recs = examples
    recs = recs[:2 * (min(len(recs), 3000) // 2)]
    pairs = [(recs[2 * i][1], recs[2 * i + 1][1]) for i in range(len(recs) // 2)]
    r1 = write_fasta(tmp_path / "r1.fa", [(f"f{i}/1", p[0]) for i, p in enumerate(pairs)])
    r2 = write_fasta(tmp_path / "r2.fa", [(f"f{i}/2", p[1]) for i, p in enumerate(pairs)])
    thr = "0.5"
    frag = combine(mate_sets(ot, [m for p in pairs for m in p], float(thr)), pair_mode)
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    src = ["--reads", r1, "--reads2", r2, "--pair-mode", pair_mode]
    _, plain = query(db, str(tmp_path / "p"), *src, "--pos-filter", "--neg-filter", thr=thr)
    _, got = query(db, str(tmp_path / "a"), *src, "--pos-filter", "--neg-filter", "--abundance", thr=thr)
    est = check_tsv(got.pop("ABUNDANCE.tsv"), frag, names)
    assert est["n_units"] == len(pairs) and got == plain
    _, alone = query(db, str(tmp_path / "c"), *src, "--abundance", thr=thr)                       # no other per-read output
    assert sorted(alone) == ["ABUNDANCE.tsv", "CLASSIFICATION.csv"] and alone["CLASSIFICATION.csv"] == plain["CLASSIFICATION.csv"]
    check_tsv(alone["ABUNDANCE.tsv"], frag, names)
    _, two = query(db, str(tmp_path / "d"), *src, "--abundance", "--devices", "0,0", thr=thr, block="16")
    assert two["ABUNDANCE.tsv"] == alone["ABUNDANCE.tsv"]
