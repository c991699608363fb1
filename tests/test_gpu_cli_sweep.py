"""`phage_filter query --sweep` on the example database: per threshold of the list, THRESHOLD_GENOMES.tsv and THRESHOLDS.tsv must
say what a run of its own at that threshold writes — the `genome,reads` pairs of CLASSIFICATION.csv byte for byte and the number
of records POS filtering keeps — and every other output of the sweep run must be the run's without the option.  Replicas, the
block size and the thread count change nothing."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "examples")
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(EX, "reads", "sim_reads_c10000_n5_e0.01.fq")
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
TIMEOUT = 300
LIST = ("0.3", "0.5", "0.7", "1.0")
OURS = ("THRESHOLDS.tsv", "THRESHOLD_GENOMES.tsv")


def run(args, env=None):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=TIMEOUT, env=env)


def query(db, out, thr, *args, env=None):
    p = run(["query", "-r", FASTQ, "-o", out, "-d", db, "-f", thr, "--pos-filter", *args], env=env)
    assert p.returncode == 0, (args, p.stderr)
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """The example database by `build`; the sweep run at -f 0.3; one plain run per threshold of the list."""
    base = tmp_path_factory.mktemp("sweep_cli")
    db = str(base / "db")
    p = run(["build", "--genomes", os.path.join(EX, "genomes"), "--db-path", db, "--seed1", str(SEEDS[0]), "--seed2", str(SEEDS[1])])
    assert p.returncode == 0, p.stderr
    swept = query(db, str(base / "swept"), LIST[0], "--sweep", ",".join(LIST))
    own = {t: query(db, str(base / f"own_{t}"), t) for t in LIST}
    return base, db, swept, own


def records(fastq):
    lines = fastq.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return (len(lines) - 1) // 4


def test_every_threshold_equals_a_run_of_its_own(runs):
    _, _, swept, own = runs
    assert set(OURS) <= set(swept)
    genomes = swept["THRESHOLD_GENOMES.tsv"].decode().splitlines()
    assert genomes[0] == "#genome\tthreshold\treads\tunique_reads"
    rows = [l.split("\t") for l in genomes[1:]]
    assert all(len(r) == 4 for r in rows)
    totals = swept["THRESHOLDS.tsv"].decode().splitlines()
    assert totals[0] == "#threshold\treads\treads_hit\treads_unique\tassignments\tgenomes_hit"
    totals = [l.split("\t") for l in totals[1:]]
    assert [r[0] for r in totals] == list(LIST)                       # as typed, ascending
    n_reads = records(open(FASTQ, "rb").read())
    hit = []
    for t, line in zip(LIST, totals):
        mine = [r for r in rows if r[1] == t]
        csv = "".join(f"{r[0]},{r[2]}\n" for r in mine).encode()
        assert csv == own[t]["CLASSIFICATION.csv"] and csv, t
        pos = records(own[t]["POS_FILTERING.fq"])
        assert [int(x) for x in line[1:]] == [n_reads, pos, sum(int(r[3]) for r in mine), sum(int(r[2]) for r in mine), len(mine)], t
        assert all(int(r[3]) <= int(r[2]) for r in mine)
        hit.append(pos)
    assert hit == sorted(hit, reverse=True) and hit[0] > hit[-1] > 0   # the list makes a difference on these reads
    order = [r[0] for r in rows if r[1] == LIST[0]]                   # genomes in CLASSIFICATION.csv's order, thresholds ascending within
    assert [(r[0], r[1]) for r in rows] == [(g, t) for g in order for t in LIST if any(x[0] == g and x[1] == t for x in rows)]


def test_the_other_outputs_are_those_of_the_run_without_the_option(runs):
    _, _, swept, own = runs
    plain = own[LIST[0]]
    assert sorted(set(swept) - set(OURS)) == sorted(plain)
    for f in plain:
        assert swept[f] == plain[f], f


@pytest.mark.parametrize("how", ["devices", "batch", "threads"])
def test_replicas_block_size_and_threads_change_nothing(runs, how):
    base, db, swept, _ = runs
    args, env = ["--sweep", ",".join(LIST)], None
    if how == "devices":
        args += ["--devices", "0,0"]
        env = dict(os.environ, PFQ_CLI_BATCH_READS="777")             # (several batches, so that both replicas count)
    elif how == "batch":
        env = dict(os.environ, PFQ_CLI_BATCH_READS="777")
    else:
        args += ["-t", "1"]
    got = query(db, str(base / how), LIST[0], *args, env=env)
    for f in OURS + ("CLASSIFICATION.csv",):
        assert got[f] == swept[f], (how, f)
    assert records(got["POS_FILTERING.fq"]) == records(swept["POS_FILTERING.fq"])


def test_a_value_below_the_filter_threshold_is_refused(runs):
    base, db, _, _ = runs
    out = str(base / "refused")
    p = run(["query", "-r", FASTQ, "-o", out, "-d", db, "-f", "0.3", "--sweep", "0.2,0.5,0.7"])
    assert p.returncode == 101 and "'--sweep 0.2'" in p.stderr and "'--filter-threshold 0.3'" in p.stderr, p.stderr
    assert not os.path.exists(out)
