"""`phage_filter query --mate-overlap ..`: every output file except PREPROCESS.tsv and INSERT_SIZES.tsv, and the exit status, must
be those of the same command without the two options on files that hold the cut mates — every read of the input, cut at
min(adapter cut, ocut) of tests/overlap_ref.py, ids unchanged.  Both steps look at the original reads, so a command that also has
--adapter is compared with one that has neither on those files; the lines of PREPROCESS.tsv that do not depend on the original
lengths must agree between the two, the others, the overlap lines and INSERT_SIZES.tsv hold the reference's values."""
import os
import subprocess

import numpy as np
import pytest

import overlap_ref
import test_ingest as ing
from test_gpu_cli_prep import CLI, EX, GOLDEN, K, SEEDS, TIMEOUT, dna, fastq
from test_overlap_cpu import revcomp

pytestmark = pytest.mark.gpu

AD33 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
ILLUMINA = b"AGATCGGAAGAGC"
O, E = 30, 10
SHARED = ("reads", "reads_kept", "dropped_short", "dropped_n", "dropped_complexity", "dropped_mate", "bases_kept", "trim_quality", "trim_window",
          "trim_poly_x", "min_length", "max_n", "min_complexity")
OWN = ("PREPROCESS.tsv", "INSERT_SIZES.tsv")


def run(env, out, reads, *args, threads=4, batch=None):
    e = dict(os.environ)
    if batch is not None:
        e["PFQ_CLI_BATCH_READS"] = str(batch)
    p = subprocess.run([CLI, "query", "--reads", str(reads), "--out", str(out), "--db-path", env["db"], "--threads", str(threads), *args],
                       capture_output=True, text=True, env=e, timeout=TIMEOUT)
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))} if os.path.isdir(out) else None
    return p.returncode, files, p.stderr


def make_mates(golden):
    """Fragments of 100-base mates: inserts of 30 .. 99 bases of a golden read with an adapter and a random tail behind them in
    either mate (every other first mate: the Illumina adapter), and whole golden reads whose mates do not overlap (unless the
    simulator drew them from one place)."""
    rng = np.random.default_rng(36)
    assert len(golden) == 1000 and all(len(r[2]) == 100 for r in golden)
    mates, inserts = [], []
    for i in range(300):
        rid, seq = golden[i][1], golden[i][2]
        n = int(rng.integers(30, 150))
        q1, q2 = (b"I" * 75 + bytes(rng.choice(np.frombuffer(b"!#+5", dtype=np.uint8), 25).astype(np.uint8)) if (i + j) % 3 == 0 else b"I" * 100 for j in (0, 1))
        if n < 100:
            a = (seq[:n] + (AD33 if i % 2 else dna(rng, 33)) + dna(rng, 100))[:100]
            b = (revcomp(seq[:n]) + dna(rng, 100))[:100]
        else:
            a, b = seq, revcomp(golden[500 + i][2])
            if i % 5 == 0:
                a = a[:80] + AD33[:20]                                # an adapter the overlap knows nothing of
        mates += [(rid, a, q1), (rid, b, q2)]
        inserts.append(n if n < 100 else None)
    return mates, inserts


@pytest.fixture(scope="module")
def env(gpu, tmp_path_factory):
    base = tmp_path_factory.mktemp("overlap_cli")
    db = str(base / "db")
    p = subprocess.run([CLI, "build", "--genomes", os.path.join(EX, "genomes"), "--db-path", db, "--seed1", str(SEEDS[0]),
                        "--seed2", str(SEEDS[1])], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    mates, inserts = make_mates(ing.parse_fastq(open(GOLDEN, "rb").read()))
    for name, recs in (("r1.fq", mates[0::2]), ("r2.fq", mates[1::2]), ("ri.fq", mates)):
        (base / name).write_bytes(fastq(recs))
    return {"db": db, "base": base, "mates": mates, "inserts": inserts}


def reference(env, base, tag, set1=(), **params):
    """overlap_ref's results and the files of the cut mates: t1 / t2 and interleaved."""
    mates = env["mates"]
    want = overlap_ref.prep_block([m[1] for m in mates], [m[2] for m in mates], O, E, set1, (), 5, 10, min_length=K, **params)
    assert min(want["cut"]) >= O                                      # (no record of the cut files is empty)
    cut = [(rid, s[:c], q[:c]) for (rid, s, q), c in zip(mates, want["cut"])]
    for name, recs in ((tag + "1.fq", cut[0::2]), (tag + "2.fq", cut[1::2]), (tag + "i.fq", cut)):
        (base / name).write_bytes(fastq(recs))
    return want


def rows_of(files):
    return dict(line.split("\t") for line in files["PREPROCESS.tsv"].decode().splitlines())


def check_own(files, want, set1=()):
    """The lines and the file that only the run with the options has, against the reference."""
    lines = [line.split("\t") for line in files["PREPROCESS.tsv"].decode().splitlines()]
    rows = dict(lines)
    assert rows["bases"] == str(want["bases_in"]) and rows["reads_trimmed"] == str(want["n_trimmed"])
    tail = [("overlap_fragments", want["n_analysed"]), ("overlap_skipped", want["n_skipped"]), ("overlap_found", want["n_overlapped"]),
            ("overlap_readthrough", want["n_readthrough"]), ("overlap_reads", want["reads_cut"]), ("overlap_bases", want["bases_cut"]),
            ("mate_overlap", O), ("mate_overlap_errors", E)]
    assert lines[-len(tail):] == [[k, str(v)] for k, v in tail]
    if len(set1):
        ad = want["adapters"]
        assert lines[15:-len(tail)] == [["adapter_reads", str(ad["n_found"])], ["adapter_bases", str(ad["bases_cut"])], ["adapter_overlap", "5"],
                                        ["adapter_errors", "10"], *([f"adapter1.{a.decode()}", str(ad["found"][i])] for i, a in enumerate(set1))]
    else:
        assert len(lines) == 15 + len(tail)
    hist = [(i, n) for i, n in enumerate(want["hist"]) if n]
    assert files["INSERT_SIZES.tsv"] == b"insert\tfragments\n" + b"".join(b"%d\t%d\n" % row for row in hist)


def same(env, tmp_path, tag, raw, cut, want, options, cut_options, *args, set1=(), **kw):
    """The raw mates with the options against the cut mates without them."""
    got = run(env, tmp_path / (tag + "_overlap"), raw[0], *raw[1:], *args, *options, **kw)
    ref = run(env, tmp_path / (tag + "_ref"), cut[0], *cut[1:], *args, *cut_options, **kw)
    assert got[0] == ref[0] == 0, (got[2], ref[2])
    assert sorted(got[1]) == sorted({*ref[1], *OWN})
    for name, data in ref[1].items():
        if name not in OWN:
            assert got[1][name] == data, (tag, name)
    got_rows, ref_rows = rows_of(got[1]), rows_of(ref[1])
    assert {k: got_rows[k] for k in SHARED} == {k: ref_rows[k] for k in SHARED}
    assert got_rows["reads_kept"] == str(want["n_kept"]) and b"," in got[1]["CLASSIFICATION.csv"]
    check_own(got[1], want, set1)
    assert "; mates overlap in %d of %d fragments, %d with read-through: %d reads cut (%d bases)\n" % (
        want["n_overlapped"], want["n_analysed"], want["n_readthrough"], want["reads_cut"], want["bases_cut"]) in got[2]
    return got[1]


OVERLAP = ["--mate-overlap", str(O)]
PLAIN = ["--min-length", str(K)]                                      # (what the options default to: the cut files' run has PREPROCESS.tsv too)


def test_two_files_and_interleaved(env, tmp_path):
    base = env["base"]
    want = reference(env, tmp_path, "t")
    assert all(got == n for got, n in zip(want["insert"], env["inserts"]) if n is not None)       # the planted inserts are all found
    assert 100 < want["n_readthrough"] <= want["n_overlapped"] < 250 and want["reads_cut"] == 2 * want["n_readthrough"]
    two = same(env, tmp_path, "a", (base / "r1.fq", "--reads2", str(base / "r2.fq")), (tmp_path / "t1.fq", "--reads2", str(tmp_path / "t2.fq")), want,
               OVERLAP, PLAIN, "--pos-filter", "--neg-filter", "--scores")
    assert len(two["POS_FILTERING_1.fq"]) > 1000 and len(two["POS_FILTERING_2.fq"]) > 1000
    inter = same(env, tmp_path, "b", (base / "ri.fq", "--interleaved"), (tmp_path / "ti.fq", "--interleaved"), want,
                 [*OVERLAP, "--mate-overlap-errors", str(E)], PLAIN, "--pos-filter")
    assert inter["CLASSIFICATION.csv"] == two["CLASSIFICATION.csv"] and all(inter[name] == two[name] for name in OWN)
    plain = run(env, tmp_path / "plain", base / "ri.fq", "--interleaved")
    assert plain[0] == 0 and not {*OWN} & {*plain[1]} and "preprocessing" not in plain[2]    # without the options nothing changes
    assert plain[1]["CLASSIFICATION.csv"] != two["CLASSIFICATION.csv"]


def test_with_an_adapter_and_quality_trimming_on_top(env, tmp_path):
    base = env["base"]
    want = reference(env, tmp_path, "t", [ILLUMINA], trim_quality=20, trim_window=4)
    ad = want["adapters"]["cut"]
    assert sum(1 for c, o in zip(ad, want["ocut"]) if c < o) > 20 and sum(1 for c, o in zip(ad, want["ocut"]) if c > o) > 100
    only_overlap = overlap_ref.prep_block([m[1] for m in env["mates"]], [m[2] for m in env["mates"]], O, E, min_length=K)
    assert want["bases_kept"] < only_overlap["bases_kept"]
    options = [*OVERLAP, "--adapter", "illumina", "--trim-quality", "20"]
    same(env, tmp_path, "a", (base / "r1.fq", "--reads2", str(base / "r2.fq")), (tmp_path / "t1.fq", "--reads2", str(tmp_path / "t2.fq")), want,
         options, ["--trim-quality", "20"], "--pos-filter", "--neg-filter", set1=[ILLUMINA])
    same(env, tmp_path, "b", (base / "ri.fq", "--interleaved"), (tmp_path / "ti.fq", "--interleaved"), want, options, ["--trim-quality", "20"], set1=[ILLUMINA])


def test_threads_small_batches_and_two_replicas(env, tmp_path):
    base = env["base"]
    want = reference(env, tmp_path, "t")
    raw, cut = (base / "ri.fq", "--interleaved"), (tmp_path / "ti.fq", "--interleaved")
    runs = [same(env, tmp_path, "a", raw, cut, want, OVERLAP, PLAIN, "--pos-filter", "--scores", threads=1),
            same(env, tmp_path, "b", raw, cut, want, OVERLAP, PLAIN, "--pos-filter", "--scores", threads=4),
            same(env, tmp_path, "c", raw, cut, want, OVERLAP, PLAIN, "--pos-filter", "--scores", "--devices", "0,0"),
            same(env, tmp_path, "d", raw, cut, want, OVERLAP, PLAIN, "--pos-filter", "--scores", "-b", "20", batch=60),
            same(env, tmp_path, "e", raw, cut, want, OVERLAP, PLAIN, "--devices", "0,0", "-b", "20", batch=60)]
    assert all(r[name] == runs[0][name] for r in runs[:3] for name in runs[0])
    assert all(r[name] == runs[0][name] for r in runs for name in (*OWN, "CLASSIFICATION.csv"))
