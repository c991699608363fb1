"""`phage_filter query --adapter ..`: every output file except PREPROCESS.tsv, and the exit status, must be those of the same command
without the adapter options on the file tests/adapter_ref.py writes — only the kept reads, each cut to what was kept, ids unchanged;
PREPROCESS.tsv must hold the reference's totals, the parameters in force and the adapter rows."""
import os
import subprocess

import numpy as np
import pytest

import adapter_ref
import test_ingest as ing
from test_gpu_cli_prep import CLI, EX, GOLDEN, K, SEEDS, TIMEOUT, dna, fasta, fastq, kept_records, query

pytestmark = pytest.mark.gpu

AD33 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
ILLUMINA, NEXTERA = b"AGATCGGAAGAGC", b"CTGTCTCTTATACACATCT"
O, E = 5, 10
OFF_ROWS = {"trim_quality": "0", "trim_window": "4", "trim_poly_x": "0", "min_length": str(K), "max_n": "off", "min_complexity": "0"}


def read_through(rng, records, adapter):
    """Read i as a library with short inserts gives it: its first n bases, the adapter, a random tail — cut to the read's length."""
    out, inserts = [], []
    for _, rid, seq, qual in records:
        n = int(rng.integers(0, len(seq) + 1))
        out.append((rid, (seq[:n] + adapter + dna(rng, len(seq)))[:len(seq)], qual))
        inserts.append(n)
    return out, inserts


@pytest.fixture(scope="module")
def env(gpu, tmp_path_factory):
    base = tmp_path_factory.mktemp("adapter_cli")
    db = str(base / "db")
    p = subprocess.run([CLI, "build", "--genomes", os.path.join(EX, "genomes"), "--db-path", db, "--seed1", str(SEEDS[0]),
                        "--seed2", str(SEEDS[1])], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    rng = np.random.default_rng(33)
    golden = ing.parse_fastq(open(GOLDEN, "rb").read())
    assert len(golden) == 1000 and all(len(r[2]) == 100 for r in golden)
    # the untouched reads: few false cuts
    false_cuts = sum(1 for r in golden if adapter_ref.find_cut(r[2], [AD33], O, E)[0] < len(r[2]))
    assert false_cuts < 10
    r1, inserts = read_through(rng, golden, AD33)
    single = adapter_ref.prep_block([r[1] for r in r1], [r[2] for r in r1], [AD33], (), O, E, min_length=K)
    findable = [i for i, n in enumerate(inserts) if n <= 100 - O]
    assert sum(1 for i in findable if single["cut"][i] == inserts[i]) >= 0.95 * len(findable) and len(findable) > 900
    assert single["n_reason"]["short"] > 100 and single["n_kept"] > 700 and single["n_trimmed"] > 650
    (base / "raw.fq").write_bytes(fastq(r1))
    (base / "cut.fq").write_bytes(fastq(kept_records(r1, single)))
    return {"db": db, "base": base, "golden": golden, "r1": r1, "single": single, "raw": base / "raw.fq", "cut": base / "cut.fq"}


def check_rows(files, want, params, set1, set2=(), overlap=O, errors=E):
    lines = [line.split("\t") for line in files["PREPROCESS.tsv"].decode().splitlines()]
    r = want["n_reason"]
    exp = [("reads", want["n_reads"]), ("reads_kept", want["n_kept"]), ("reads_trimmed", want["n_trimmed"]), ("dropped_short", r["short"]),
           ("dropped_n", r["n"]), ("dropped_complexity", r["complexity"]), ("dropped_mate", r["mate"]), ("bases", want["bases_in"]),
           ("bases_kept", want["bases_kept"]), *params.items(),
           ("adapter_reads", want["n_found"]), ("adapter_bases", want["bases_cut"]), ("adapter_overlap", overlap), ("adapter_errors", errors),
           *((f"adapter1.{a.decode()}", want["found"][i]) for i, a in enumerate(set1)),
           *((f"adapter2.{a.decode()}", want["found"][8 + i]) for i, a in enumerate(set2))]
    assert lines == [[k, str(v)] for k, v in exp]


def same(env, tmp_path, tag, raw, cut, want, options, *args, batch=None, raw_args=(), cut_args=(), cut_options=()):
    """The raw input with the adapter options against the reference's kept, cut input without them."""
    got = query(env, tmp_path / (tag + "_adapter"), raw, *raw_args, *args, *options, batch=batch)
    ref = query(env, tmp_path / (tag + "_ref"), cut, *cut_args, *args, *cut_options, batch=batch)
    assert got[0] == ref[0] == 0, (got[2], ref[2])
    assert sorted(got[1]) == sorted({*ref[1], "PREPROCESS.tsv"})
    for name, data in ref[1].items():
        if name != "PREPROCESS.tsv":
            assert got[1][name] == data, (tag, name)
    assert b"," in got[1]["CLASSIFICATION.csv"]
    assert "preprocessing: %d reads, %d kept" % (want["n_reads"], want["n_kept"]) in got[2]
    assert "bases kept; adapters cut from %d reads (%d bases)\n" % (want["n_found"], want["bases_cut"]) in got[2]
    return got[1]


ADAPTER = ["--adapter", AD33.decode()]


def test_counts_filtering_and_scores(env, tmp_path):
    files = same(env, tmp_path, "a", env["raw"], env["cut"], env["single"], ADAPTER)                  # counts only
    check_rows(files, env["single"], OFF_ROWS, [AD33])
    files = same(env, tmp_path, "b", env["raw"], env["cut"], env["single"], ADAPTER, "--pos-filter", "--neg-filter", "--scores")
    assert len(files["POS_FILTERING.fq"]) > 1000 and len(files["READ_SCORES.tsv"]) > 1000
    check_rows(files, env["single"], OFF_ROWS, [AD33])
    plain = query(env, tmp_path / "plain", env["raw"])
    assert plain[0] == 0 and "PREPROCESS.tsv" not in plain[1] and "preprocessing" not in plain[2]   # without the options nothing changes
    assert plain[1]["CLASSIFICATION.csv"] != files["CLASSIFICATION.csv"]


def test_small_batches_and_two_replicas(env, tmp_path):
    files = same(env, tmp_path, "a", env["raw"], env["cut"], env["single"], ADAPTER, "--pos-filter", "--scores", "-b", "50", batch=50)
    check_rows(files, env["single"], OFF_ROWS, [AD33])
    files = same(env, tmp_path, "b", env["raw"], env["cut"], env["single"], ADAPTER, "--devices", "0,0", "--pos-filter", "--scores")
    check_rows(files, env["single"], OFF_ROWS, [AD33])
    same(env, tmp_path, "c", env["raw"], env["cut"], env["single"], ADAPTER, "--devices", "0,0", "-b", "50", batch=50)


def test_pairs_with_a_second_set(env, tmp_path):
    rng = np.random.default_rng(34)
    golden = env["golden"]
    r1 = env["r1"][:500]
    r2, _ = read_through(rng, golden[500:], NEXTERA)
    r2 = [(a[0], b[1], b[2]) for a, b in zip(r1, r2)]                 # mates carry one id
    mates = [m for pair in zip(r1, r2) for m in pair]
    want = adapter_ref.prep_block([m[1] for m in mates], [m[2] for m in mates], [AD33], [NEXTERA], 8, E, paired=True, min_length=K)
    assert want["n_reason"]["mate"] >= 20 and want["n_kept"] >= 300 and want["found"][0] > 300 and want["found"][8] > 300
    kept = kept_records(mates, want)
    for name, recs in (("r1.fq", r1), ("r2.fq", r2), ("t1.fq", kept[0::2]), ("t2.fq", kept[1::2]), ("ri.fq", mates), ("ti.fq", kept)):
        (tmp_path / name).write_bytes(fastq(recs))
    options = [*ADAPTER, "--adapter2", "nextera", "--adapter-overlap", "8"]
    files = same(env, tmp_path, "a", tmp_path / "r1.fq", tmp_path / "t1.fq", want, options, "--pos-filter", "--neg-filter", "--scores",
                 raw_args=("--reads2", str(tmp_path / "r2.fq")), cut_args=("--reads2", str(tmp_path / "t2.fq")))
    assert len(files["POS_FILTERING_2.fq"]) > 1000
    check_rows(files, want, OFF_ROWS, [AD33], [NEXTERA], overlap=8)
    files = same(env, tmp_path, "b", tmp_path / "ri.fq", tmp_path / "ti.fq", want, options, "--interleaved", "--devices", "0,0", "-b", "20", batch=60)
    check_rows(files, want, OFF_ROWS, [AD33], [NEXTERA], overlap=8)


def test_a_preset_together_with_quality_trimming(env, tmp_path):
    r1 = env["r1"]
    rng = np.random.default_rng(35)
    # (the golden reads' qualities are all '#': good ones here, and every third read with a tail of bad ones)
    spoiled = [(rid, s, b"I" * 70 + bytes(rng.choice(np.frombuffer(b"!#+5", dtype=np.uint8), len(s) - 70).astype(np.uint8)) if i % 3 == 0 else b"I" * len(s))
               for i, (rid, s, _) in enumerate(r1)]
    params = dict(trim_quality=20, trim_window=4, min_length=K)
    want = adapter_ref.prep_block([r[1] for r in spoiled], [r[2] for r in spoiled], [ILLUMINA, NEXTERA], (), O, E, **params)
    only_quality = adapter_ref.prep_block([r[1] for r in spoiled], [r[2] for r in spoiled], [b"C" * 64], (), 64, 0, **params)
    assert want["bases_kept"] < only_quality["bases_kept"] < want["bases_in"] and only_quality["n_found"] == 0
    (tmp_path / "raw.fq").write_bytes(fastq(spoiled))
    (tmp_path / "cut.fq").write_bytes(fastq(kept_records(spoiled, want)))
    files = same(env, tmp_path, "a", tmp_path / "raw.fq", tmp_path / "cut.fq", want, ["--adapter", "illumina", "--adapter", "nextera", "--trim-quality", "20"],
                 "--pos-filter", "--neg-filter")
    check_rows(files, want, {**OFF_ROWS, "trim_quality": "20"}, [ILLUMINA, NEXTERA])


def test_fasta_input(env, tmp_path):
    r1, single = env["r1"], env["single"]
    want = adapter_ref.prep_block([r[1] for r in r1], None, [AD33], (), O, E, min_length=K)
    assert want["cut"] == single["cut"] and want["kept"] == single["kept"]
    (tmp_path / "raw.fa").write_bytes(fasta(r1))
    (tmp_path / "cut.fa").write_bytes(fasta(kept_records(r1, want)))
    files = same(env, tmp_path, "a", tmp_path / "raw.fa", tmp_path / "cut.fa", want, ["--adapter=" + AD33.decode().lower()], "--pos-filter", "--neg-filter")
    check_rows(files, want, OFF_ROWS, [AD33])
