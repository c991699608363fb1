"""`phage_filter query --mate-overlap .. --mate-correct`: every output file except PREPROCESS.tsv and INSERT_SIZES.tsv, and the exit
status, must be those of the same command without --mate-overlap, --mate-correct and --adapter on files that hold the corrected
mates of tests/correct_ref.py — bases and qualities, cut at min(adapter cut, ocut) of the original mates, ids unchanged.  The new
lines of PREPROCESS.tsv and the clause on stderr hold the reference's values; a run with --mate-overlap alone has neither."""
import os
import shutil
import subprocess

import pytest

import correct_ref
import test_ingest as ing
from test_gpu_cli_overlap import E, ILLUMINA, O, OVERLAP, OWN, PLAIN, SHARED, make_mates, rows_of, run
from test_gpu_cli_prep import CLI, EX, GOLDEN, K, SEEDS, TIMEOUT, fastq

pytestmark = pytest.mark.gpu

CORRECT = [*OVERLAP, "--mate-correct"]
OTHER = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}


def spoil_overlaps(mates, inserts):
    """A substitution in the overlap of every third fragment with read-through: in mate 2 with quality '#' where mate 1's is 'I' (to
    be corrected), every other one of them also one in mate 1 against a good base of mate 2, and every fourth one with both
    qualities low (unresolvable)."""
    out = [list(m) for m in mates]
    planted = 0
    for f, n in enumerate(inserts):
        if n is None or f % 3:
            continue
        a, q1, b, q2 = (bytearray(out[2 * f + m][x]) for m in (0, 1) for x in (1, 2))
        spots = [(5, "b")] + ([(min(n, 70) - 2, "a")] if f % 2 == 0 else []) + ([(20, "both")] if f % 4 == 0 else [])
        for i, kind in spots:
            j = n - 1 - i
            if kind == "a":
                a[i], q1[i], q2[j] = OTHER[a[i]], ord("#"), ord("I")
            else:
                b[j], q2[j], q1[i] = OTHER[b[j]], ord("#"), ord("#" if kind == "both" else "I")
            planted += 1
        out[2 * f][1:], out[2 * f + 1][1:] = [bytes(a), bytes(q1)], [bytes(b), bytes(q2)]
    return [tuple(m) for m in out], planted


@pytest.fixture(scope="module")
def env(gpu, tmp_path_factory):
    base = tmp_path_factory.mktemp("correct_cli")
    db, screen, few = str(base / "db"), str(base / "screen"), base / "few"
    few.mkdir()
    for name in sorted(os.listdir(os.path.join(EX, "genomes")))[:3]:
        shutil.copy(os.path.join(EX, "genomes", name), few / name)
    for path, genomes in ((db, os.path.join(EX, "genomes")), (screen, str(few))):
        p = subprocess.run([CLI, "build", "--genomes", genomes, "--db-path", path, "--seed1", str(SEEDS[0]), "--seed2", str(SEEDS[1])],
                           capture_output=True, text=True, timeout=TIMEOUT)
        assert p.returncode == 0, p.stderr
    mates, inserts = make_mates(ing.parse_fastq(open(GOLDEN, "rb").read()))
    mates, planted = spoil_overlaps(mates, inserts)
    assert planted > 80
    for name, recs in (("r1.fq", mates[0::2]), ("r2.fq", mates[1::2]), ("ri.fq", mates)):
        (base / name).write_bytes(fastq(recs))
    return {"db": db, "screen": screen, "base": base, "mates": mates, "inserts": inserts}


def reference(env, base, tag, set1=(), **params):
    """correct_ref's results and the files of the corrected, cut mates: t1 / t2 and interleaved."""
    mates = env["mates"]
    want = correct_ref.prep_block([m[1] for m in mates], [m[2] for m in mates], O, E, set1=set1, min_length=K, **params)
    cor = want["corrections"]
    assert min(want["cut"]) >= O and cor["n_fragments_corrected"] > 40 and min(cor["n_bases"]) > 20 and cor["n_unresolved"] > 8
    cut = [(m[0], s[:c], q[:c]) for m, s, q, c in zip(mates, cor["reads"], cor["quals"], want["cut"])]
    for name, recs in ((tag + "1.fq", cut[0::2]), (tag + "2.fq", cut[1::2]), (tag + "i.fq", cut)):
        (base / name).write_bytes(fastq(recs))
    return want


def same(env, tmp_path, tag, raw, cut, want, options, cut_options, *args, high=30, low=14, **kw):
    """The raw mates with the options against the corrected, cut mates without them."""
    got = run(env, tmp_path / (tag + "_correct"), raw[0], *raw[1:], *args, *options, **kw)
    ref = run(env, tmp_path / (tag + "_ref"), cut[0], *cut[1:], *args, *cut_options, **kw)
    assert got[0] == ref[0] == 0, (got[2], ref[2])
    assert sorted(got[1]) == sorted({*ref[1], *OWN})
    for name, data in ref[1].items():
        if name not in OWN:
            assert got[1][name] == data, (tag, name)
    got_rows, ref_rows = rows_of(got[1]), rows_of(ref[1])
    assert {k: got_rows[k] for k in SHARED} == {k: ref_rows[k] for k in SHARED}
    assert got_rows["reads_kept"] == str(want["n_kept"]) and b"," in got[1]["CLASSIFICATION.csv"]
    cor = want["corrections"]
    rows = [("corrected_fragments", cor["n_fragments_corrected"]), ("corrected_bases", sum(cor["n_bases"])), ("correct_unresolved", cor["n_unresolved"]),
            ("correct_no_quality", cor["n_no_quality"]), ("mate_correct_quality", high), ("mate_correct_low", low)]
    lines = [line.split("\t") for line in got[1]["PREPROCESS.tsv"].decode().splitlines()]
    at = lines.index(["mate_overlap_errors", str(E)])                # directly behind the overlap rows, before any deplete rows
    assert lines[at + 1:at + 1 + len(rows)] == [[k, str(v)] for k, v in rows]
    assert all(line[0].startswith("deplet") for line in lines[at + 1 + len(rows):])
    assert "; %d bases corrected in %d fragments (%d mismatches unresolved, %d fragments without qualities)" % (
        sum(cor["n_bases"]), cor["n_fragments_corrected"], cor["n_unresolved"], cor["n_no_quality"]) in got[2]
    return got[1]


def test_two_files_and_interleaved(env, tmp_path):
    base = env["base"]
    want = reference(env, tmp_path, "t")
    two = same(env, tmp_path, "a", (base / "r1.fq", "--reads2", str(base / "r2.fq")), (tmp_path / "t1.fq", "--reads2", str(tmp_path / "t2.fq")), want,
               CORRECT, PLAIN, "--pos-filter", "--neg-filter", "--scores")
    assert len(two["POS_FILTERING_1.fq"]) > 1000 and len(two["POS_FILTERING_2.fq"]) > 1000
    inter = same(env, tmp_path, "b", (base / "ri.fq", "--interleaved"), (tmp_path / "ti.fq", "--interleaved"), want,
                 [*CORRECT, "--mate-correct-quality", "30,14"], PLAIN, "--pos-filter")
    assert inter["CLASSIFICATION.csv"] == two["CLASSIFICATION.csv"] and all(inter[name] == two[name] for name in OWN)
    # --mate-overlap alone: no new row, no clause, and other results (the errors stay in the reads)
    alone = run(env, tmp_path / "alone", base / "ri.fq", "--interleaved", *OVERLAP, "--pos-filter")
    assert alone[0] == 0 and "correct" not in alone[1]["PREPROCESS.tsv"].decode() and "corrected" not in alone[2]
    assert alone[1]["PREPROCESS.tsv"].decode().splitlines()[-1] == "mate_overlap_errors\t%d" % E
    assert alone[1]["INSERT_SIZES.tsv"] == two["INSERT_SIZES.tsv"] and [v for k, v in sorted(alone[1].items()) if k.startswith("POS_")] != [v for k, v in sorted(inter.items()) if k.startswith("POS_")]


def test_other_bounds(env, tmp_path):
    base = env["base"]
    mates = env["mates"]
    want = correct_ref.prep_block([m[1] for m in mates], [m[2] for m in mates], O, E, 41, 1, min_length=K)      # nothing qualifies
    assert want["corrections"]["patches"] == [] and want["corrections"]["n_unresolved"] > 80
    cut = [(m[0], m[1][:c], m[2][:c]) for m, c in zip(mates, want["cut"])]
    (tmp_path / "ti.fq").write_bytes(fastq(cut))
    same(env, tmp_path, "a", (base / "ri.fq", "--interleaved"), (tmp_path / "ti.fq", "--interleaved"), want, [*CORRECT, "--mate-correct-quality", "41,1"], PLAIN,
         "--pos-filter", high=41, low=1)


def test_with_an_adapter_and_quality_trimming_on_top(env, tmp_path):
    base = env["base"]
    want = reference(env, tmp_path, "t", [ILLUMINA], trim_quality=20, trim_window=4)
    options = [*CORRECT, "--adapter", "illumina", "--trim-quality", "20"]
    same(env, tmp_path, "a", (base / "r1.fq", "--reads2", str(base / "r2.fq")), (tmp_path / "t1.fq", "--reads2", str(tmp_path / "t2.fq")), want,
         options, ["--trim-quality", "20"], "--pos-filter", "--neg-filter")
    same(env, tmp_path, "b", (base / "ri.fq", "--interleaved"), (tmp_path / "ti.fq", "--interleaved"), want, options, ["--trim-quality", "20"], "--scores")


def test_with_a_screen(env, tmp_path):
    base = env["base"]
    want = reference(env, tmp_path, "t")
    raw, cut = (base / "ri.fq", "--interleaved"), (tmp_path / "ti.fq", "--interleaved")
    got = same(env, tmp_path, "a", raw, cut, want, CORRECT, PLAIN, "--deplete", env["screen"], "--pos-filter", "--neg-filter")
    rows = rows_of(got)
    assert int(rows["depleted_reads"]) > 20 and "DEPLETION.csv" in got


def test_threads_small_batches_and_two_replicas(env, tmp_path):
    base = env["base"]
    want = reference(env, tmp_path, "t")
    raw, cut = (base / "ri.fq", "--interleaved"), (tmp_path / "ti.fq", "--interleaved")
    runs = [same(env, tmp_path, "a", raw, cut, want, CORRECT, PLAIN, "--pos-filter", "--scores", threads=1),
            same(env, tmp_path, "b", raw, cut, want, CORRECT, PLAIN, "--pos-filter", "--scores", "--devices", "0,0", threads=4),
            same(env, tmp_path, "c", raw, cut, want, CORRECT, PLAIN, "--pos-filter", "--scores", "-b", "20", batch=60),
            same(env, tmp_path, "d", raw, cut, want, CORRECT, PLAIN, "--devices", "0,0", "-b", "20", batch=60)]
    assert all(r[name] == runs[0][name] for r in runs[:2] for name in runs[0])
    assert all(r[name] == runs[0][name] for r in runs for name in (*OWN, "CLASSIFICATION.csv"))
