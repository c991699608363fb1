"""`phage_filter query --deplete`: every output file the run without the option writes, the exit status and stderr must be those of
that run on the file the references write — tests/prep_ref.py's kept, trimmed records of which tests/deplete_ref.py (the CPU
oracle on the screen's database) removes the ones that hit — whatever -b, -t and --devices; DEPLETION*.csv must hold the oracle's
counts (one screen: also the existing CLI's CLASSIFICATION.csv of the kept file against the screen) and PREPROCESS.tsv the old and
the new lines."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import deplete_ref
import prep_ref
import test_ingest as ing
from oracle import pfq_format as fmt
from test_gpu_cli_prep import CLI, EX, K, OPTIONS, PARAM_ROWS, PARAMS, SEEDS, TIMEOUT, fastq, kept_records, spoil

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(EX, "reads", "sim_reads_c10000_n5_e0.01.fq")
THR = "0.7"
# the golden reads come genome by genome: records 100 .. 499 are of ViralProj219118 (100), ViralProj215674 (200) and ViralProj219114 (100)
FIRST, COUNT = 100, 400
SCREEN_A = ["GCF_000912575.1_ViralProj215674_genomic.fna", "GCF_900149655.1_LeviOr01_genomic.fna"]
SCREEN_B = ["GCF_000912695.1_ViralProj219114_genomic.fna", "GCF_927798495.1_Voltaire_bis_genomic.fna"]


def build(db, genomes, *args):
    p = subprocess.run([CLI, "build", "--genomes", str(genomes), "--db-path", str(db), "--seed1", str(SEEDS[0]), "--seed2", str(SEEDS[1]), *args],
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr


def csv_of(tree, counts):
    """CLASSIFICATION.csv's lines for per-column counts of a tree."""
    return "".join(f"{tree.tax_id[v]},{c}\n" for v, c in zip(tree.leaves_dfs(), counts) if c > 0).encode()


def rows_of(tree, reads, thr, paired=False):
    sets = deplete_ref.leaf_sets(tree, reads, thr)
    return [sets[i] | sets[i + 1] for i in range(0, len(sets), 2)] if paired else sets


@pytest.fixture(scope="module")
def env(gpu, tmp_path_factory):
    base = tmp_path_factory.mktemp("deplete_cli")
    db = str(base / "db")
    build(db, os.path.join(EX, "genomes"))
    screens = []
    for tag, names in (("a", SCREEN_A), ("b", SCREEN_B)):
        src = base / ("genomes_" + tag)
        src.mkdir()
        for n in names:
            shutil.copy(os.path.join(EX, "genomes", n), src / n)
        build(base / ("screen_" + tag), src, "-k", "17")
        screens.append(str(base / ("screen_" + tag)))
    rng = np.random.default_rng(21)
    golden = ing.parse_fastq(open(GOLDEN, "rb").read())
    r1 = spoil(rng, golden[FIRST:FIRST + COUNT])
    r2 = spoil(rng, golden[FIRST:FIRST + COUNT][::-1])
    r2 = [(a[0], b[1], b[2]) for a, b in zip(r1, r2[3:] + r2[:3])]    # mates carry one id; their kinds differ
    e = {"db": db, "base": base, "screens": screens, "r1": r1, "r2": r2, "main_o": fmt.read_db(db), "screen_o": [fmt.read_db(s) for s in screens]}
    assert e["screen_o"][0].kmer_size == 17 and e["main_o"].kmer_size == K
    # the reference alone, before the option is tried
    prep = prep_ref.prep_block([r[1] for r in r1], [r[2] for r in r1], **PARAMS)
    dep = deplete_ref.deplete(prep["kept_reads"], e["screen_o"][0], float(THR), kept=prep["kept"], reason=prep["reason"])
    assert dep["units_removed"] >= 100 and dep["n_kept"] >= 100, (dep["units_removed"], dep["n_kept"])
    assert sum(map(bool, rows_of(e["main_o"], dep["survivors"], 1.0))) >= 50
    e.update(prep=prep, dep=dep)
    (base / "raw.fq").write_bytes(fastq(r1))
    (base / "kept.fq").write_bytes(fastq(kept_records(r1, prep)))
    (base / "left.fq").write_bytes(fastq(kept_records(r1, dict(prep, kept=dep["kept"]))))
    return e


def query(env, out, reads, *args, db=None, threads="4"):
    p = subprocess.run([CLI, "query", "--reads", str(reads), "--out", str(out), "--db-path", db or env["db"], "--threads", threads, *args],
                       capture_output=True, text=True, timeout=TIMEOUT)
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))} if os.path.isdir(out) else None
    return p.returncode, files, p.stderr


def stderr_lines(text):
    return [line for line in text.splitlines() if not line.startswith("preprocessing:")]


def check_preprocess(files, prep, deps, screens):
    lines = [line.split("\t") for line in files["PREPROCESS.tsv"].decode().splitlines()]
    r = prep["n_reason"]
    old = {"reads": prep["n_reads"], "reads_kept": prep["n_kept"], "reads_trimmed": prep["n_trimmed"], "dropped_short": r["short"], "dropped_n": r["n"],
           "dropped_complexity": r["complexity"], "dropped_mate": r["mate"], "bases": prep["bases_in"], "bases_kept": prep["bases_kept"]}
    want = [[k, str(v)] for k, v in old.items()] + [[k, PARAM_ROWS[k]] for k in ("trim_quality", "trim_window", "trim_poly_x", "min_length", "max_n", "min_complexity")]
    for dep, screen in zip(deps, screens):
        want += [["deplete_db", screen], ["deplete_threshold", THR], ["depleted_units", str(dep["units_removed"])],
                 ["depleted_reads", str(dep["reads_removed"])], ["depleted_bases", str(dep["bases_removed"])]]
    assert lines == want


def same(env, tmp_path, tag, *args, threads="4"):
    """The raw file with the trim options and one screen against the references' remaining records without either."""
    base = env["base"]
    got = query(env, tmp_path / (tag + "_deplete"), base / "raw.fq", *args, *OPTIONS, "--deplete", env["screens"][0], "--deplete-threshold", THR, threads=threads)
    ref = query(env, tmp_path / (tag + "_ref"), base / "left.fq", *args, threads=threads)
    assert got[0] == ref[0] == 0, (got[2], ref[2])
    assert sorted(got[1]) == sorted([*ref[1], "PREPROCESS.tsv", "DEPLETION.csv"]), tag
    for name, data in ref[1].items():
        assert got[1][name] == data, (tag, name)
    assert stderr_lines(got[2]) == stderr_lines(ref[2]), tag
    assert b"," in got[1]["CLASSIFICATION.csv"]
    assert got[1]["DEPLETION.csv"] == csv_of(env["screen_o"][0], env["dep"]["leaf_counts"]), tag
    check_preprocess(got[1], env["prep"], [env["dep"]], env["screens"][:1])
    assert "screen %s took %d reads" % (env["screens"][0], env["dep"]["reads_removed"]) in got[2]
    return got[1]


def test_counts_only_and_the_two_run_pipeline(env, tmp_path):
    files = same(env, tmp_path, "a")
    # the existing CLI, asked what the screen sees: the kept, trimmed reads against the screen's database at T
    two_run = query(env, tmp_path / "screen_run", env["base"] / "kept.fq", "-f", THR, "--neg-filter", db=env["screens"][0])
    assert two_run[0] == 0 and files["DEPLETION.csv"] == two_run[1]["CLASSIFICATION.csv"] and b"," in files["DEPLETION.csv"]
    left = [(rid, s.upper(), q) for _, rid, s, q in ing.parse_fastq((env["base"] / "left.fq").read_bytes())]   # (the writers print upper case)
    assert [r[1:] for r in ing.parse_fastq(two_run[1]["NEG_FILTERING.fq"])] == left and len(left) == env["dep"]["n_kept"]   # it leaves what the references leave


def test_filtering_and_scores(env, tmp_path):
    files = same(env, tmp_path, "a", "--pos-filter", "--neg-filter")
    assert len(files["POS_FILTERING.fq"]) > 1000
    files = same(env, tmp_path, "b", "--scores", "--pos-filter")
    assert len(files["READ_SCORES.tsv"]) > 1000


def test_replicas_blocks_and_threads(env, tmp_path):
    same(env, tmp_path, "a", "--devices", "0,0")
    same(env, tmp_path, "b", "--devices", "0,0", "--pos-filter", "--scores")
    same(env, tmp_path, "c", "-b", "100")
    same(env, tmp_path, "d", "-b", "100", "--neg-filter")
    same(env, tmp_path, "e", "--neg-filter", threads="1")


def test_pairs(env, tmp_path):
    r1, r2, screen = env["r1"], env["r2"], env["screen_o"][0]
    mates = [m for pair in zip(r1, r2) for m in pair]
    prep = prep_ref.prep_block([m[1] for m in mates], [m[2] for m in mates], paired=True, **PARAMS)
    dep = deplete_ref.deplete(prep["kept_reads"], screen, float(THR), paired=True, kept=prep["kept"], reason=prep["reason"])
    assert dep["units_removed"] >= 20 and dep["n_kept"] >= 40 and prep["n_reason"]["mate"] >= 20
    left = kept_records(mates, dict(prep, kept=dep["kept"]))
    for name, recs in (("r1.fq", r1), ("r2.fq", r2), ("l1.fq", left[0::2]), ("l2.fq", left[1::2])):
        (tmp_path / name).write_bytes(fastq(recs))
    args = ("--pos-filter", "--neg-filter", "--scores")
    got = query(env, tmp_path / "deplete", tmp_path / "r1.fq", "--reads2", str(tmp_path / "r2.fq"), *args, *OPTIONS, "--deplete", env["screens"][0],
                "--deplete-threshold", THR)
    ref = query(env, tmp_path / "ref", tmp_path / "l1.fq", "--reads2", str(tmp_path / "l2.fq"), *args)
    assert got[0] == ref[0] == 0, (got[2], ref[2])
    assert sorted(got[1]) == sorted([*ref[1], "PREPROCESS.tsv", "DEPLETION.csv"])
    for name, data in ref[1].items():
        assert got[1][name] == data, name
    assert stderr_lines(got[2]) == stderr_lines(ref[2])
    assert got[1]["DEPLETION.csv"] == csv_of(screen, dep["leaf_counts"])              # a fragment counts once per genome either mate hits
    check_preprocess(got[1], prep, [dep], env["screens"][:1])
    assert len(got[1]["POS_FILTERING_2.fq"]) > 1000


def test_two_screens(env, tmp_path):
    base, prep, a = env["base"], env["prep"], env["dep"]
    b = deplete_ref.deplete(a["survivors"], env["screen_o"][1], float(THR), kept=a["kept"], reason=a["reason"])
    assert b["units_removed"] >= 20 and b["n_kept"] >= 20
    (tmp_path / "left2.fq").write_bytes(fastq(kept_records(env["r1"], dict(prep, kept=b["kept"]))))
    for tag, args in (("a", ("--pos-filter", "--neg-filter")), ("b", ("--devices", "0,0", "-b", "100"))):
        got = query(env, tmp_path / (tag + "_deplete"), base / "raw.fq", *args, *OPTIONS, "--deplete", env["screens"][0], "--deplete", env["screens"][1],
                    "--deplete-threshold", THR)
        ref = query(env, tmp_path / (tag + "_ref"), tmp_path / "left2.fq", *args)
        assert got[0] == ref[0] == 0, (got[2], ref[2])
        assert sorted(got[1]) == sorted([*ref[1], "PREPROCESS.tsv", "DEPLETION_1.csv", "DEPLETION_2.csv"])
        for name, data in ref[1].items():
            assert got[1][name] == data, (tag, name)
        assert stderr_lines(got[2]) == stderr_lines(ref[2])
        assert got[1]["DEPLETION_1.csv"] == csv_of(env["screen_o"][0], a["leaf_counts"])
        assert got[1]["DEPLETION_2.csv"] == csv_of(env["screen_o"][1], b["leaf_counts"]) and b"," in got[1]["DEPLETION_2.csv"]   # screen 2 sees what screen 1 left
        check_preprocess(got[1], prep, [a, b], env["screens"])


def test_the_threshold_defaults_to_the_runs(env, tmp_path):
    base, prep = env["base"], env["prep"]
    dep = deplete_ref.deplete(prep["kept_reads"], env["screen_o"][0], 0.5, kept=prep["kept"], reason=prep["reason"])
    (tmp_path / "left.fq").write_bytes(fastq(kept_records(env["r1"], dict(prep, kept=dep["kept"]))))
    got = query(env, tmp_path / "deplete", base / "raw.fq", "-f", "0.5", *OPTIONS, "--deplete", env["screens"][0])
    ref = query(env, tmp_path / "ref", tmp_path / "left.fq", "-f", "0.5")
    assert got[0] == ref[0] == 0, (got[2], ref[2])
    assert got[1]["CLASSIFICATION.csv"] == ref[1]["CLASSIFICATION.csv"] and got[1]["DEPLETION.csv"] == csv_of(env["screen_o"][0], dep["leaf_counts"])
    assert "deplete_threshold\t0.5\n" in got[1]["PREPROCESS.tsv"].decode()
