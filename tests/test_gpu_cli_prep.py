"""`phage_filter query` with the preprocessing options: every output file except PREPROCESS.tsv, and the exit status, must be
those of the same command without the options on the file tests/prep_ref.py writes — only the kept reads, each cut to what was
kept, ids unchanged; PREPROCESS.tsv must hold the reference's totals and the parameters in force."""
import os
import subprocess

import numpy as np
import pytest

import prep_ref
import test_ingest as ing
from oracle import pfq_format as fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "examples")
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
GOLDEN = os.path.join(EX, "reads", "sim_reads_c10000_n5_e0.01.fq")
TIMEOUT = 300
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
K = 20                                                                # `build`'s default k-mer size
OPTIONS = ["--trim-quality", "20", "--trim-poly-x", "10", "--max-n", "3", "--min-complexity", "30"]
PARAMS = dict(trim_quality=20, trim_window=4, poly_x=10, min_length=K, max_n=3, min_complexity=30)    # --min-length defaults to k
PARAM_ROWS = {"trim_quality": "20", "trim_window": "4", "trim_poly_x": "10", "min_length": str(K), "max_n": "3", "min_complexity": "30"}


def dna(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).astype(np.uint8))


def spoil(rng, records):
    """The golden reads as a sequencer might have left them: random low-quality tails, varied qualities, some poly-G tails, some
    reads under k, some N-rich and some homopolymer reads."""
    out = []
    for i, (_, rid, seq, _) in enumerate(records):
        kind = i % 10
        if kind == 0:                                                 # a poly-G tail under good qualities
            s, q = seq[:70] + b"G" * 14, b"I" * 84
        elif kind == 1:                                               # under k
            s, q = seq[:int(rng.integers(1, K))], b"I" * 100
            q = q[:len(s)]
        elif kind == 2:                                               # N-rich
            s = bytearray(seq)
            for j in rng.integers(0, len(s), 8).tolist():
                s[j] = ord("N")
            s, q = bytes(s), b"I" * len(seq)
        elif kind == 3:                                               # low complexity
            s, q = b"A" * 60 + seq[:3], b"I" * 63
        elif kind == 4:                                               # a few bad leading bases, lower case
            s, q = seq.lower(), b"#" * 3 + b"5" * (len(seq) - 3)
        else:                                                         # a random tail whose qualities decay
            t = int(rng.integers(5, 40))
            s = seq + dna(rng, t)
            q = bytes(rng.choice(np.frombuffer(b"5?IJ", dtype=np.uint8), len(seq)).astype(np.uint8)) + \
                bytes(rng.choice(np.frombuffer(b"!#+5", dtype=np.uint8), t, p=[.3, .4, .2, .1]).astype(np.uint8))
        out.append((rid, s, q))
    return out


def fastq(records):
    return b"".join(b"@" + rid + b"\n" + s + b"\n+\n" + q + b"\n" for rid, s, q in records)


def fasta(records):
    return b"".join(b">" + rid + b"\n" + s + b"\n" for rid, s, _ in records)


def kept_records(records, res):
    return [(records[i][0], records[i][1][res["begin"][i]:res["begin"][i] + res["len"][i]],
             records[i][2][res["begin"][i]:res["begin"][i] + res["len"][i]]) for i in res["kept"]]


@pytest.fixture(scope="module")
def env(gpu, tmp_path_factory):
    base = tmp_path_factory.mktemp("prep_cli")
    db = str(base / "db")
    p = subprocess.run([CLI, "build", "--genomes", os.path.join(EX, "genomes"), "--db-path", db, "--seed1", str(SEEDS[0]),
                        "--seed2", str(SEEDS[1])], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    rng = np.random.default_rng(20)
    golden = ing.parse_fastq(open(GOLDEN, "rb").read())
    r1, r2 = spoil(rng, golden[:400]), spoil(rng, golden[400:800][::-1])
    r2 = [(a[0], b[1], b[2]) for a, b in zip(r1, r2[3:] + r2[:3])]    # mates carry one id; their kinds differ
    single = prep_ref.prep_block([r[1] for r in r1], [r[2] for r in r1], **PARAMS)
    assert all(single["n_reason"][k] >= 20 for k in ("kept", "short", "n", "complexity")) and single["n_trimmed"] >= 150
    ot = fmt.read_db(db)
    names = sorted(ot.tax_id[v] for v in ot.leaves_dfs())
    return {"db": db, "base": base, "r1": r1, "r2": r2, "single": single, "names": names}


def query(env, out, reads, *args, batch=None):
    e = dict(os.environ)
    if batch is not None:
        e["PFQ_CLI_BATCH_READS"] = str(batch)
    p = subprocess.run([CLI, "query", "--reads", str(reads), "--out", str(out), "--db-path", env["db"], "--threads", "4", *args],
                       capture_output=True, text=True, env=e, timeout=TIMEOUT)
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))} if os.path.isdir(out) else None
    return p.returncode, files, p.stderr


def check_totals(files, want):
    rows = dict(line.split("\t") for line in files["PREPROCESS.tsv"].decode().splitlines())
    r = want["n_reason"]
    exp = {"reads": want["n_reads"], "reads_kept": want["n_kept"], "reads_trimmed": want["n_trimmed"], "dropped_short": r["short"],
           "dropped_n": r["n"], "dropped_complexity": r["complexity"], "dropped_mate": r["mate"], "bases": want["bases_in"],
           "bases_kept": want["bases_kept"]}
    assert rows == {**{k: str(v) for k, v in exp.items()}, **PARAM_ROWS}
    assert list(rows)[:9] == list(exp)


def same(env, tmp_path, tag, raw, trimmed, want, *args, batch=None, options=OPTIONS, raw_args=(), trimmed_args=()):
    """The original input with the options against the reference's kept, trimmed input without them."""
    got = query(env, tmp_path / (tag + "_prep"), raw, *raw_args, *args, *options, batch=batch)
    ref = query(env, tmp_path / (tag + "_ref"), trimmed, *trimmed_args, *args, batch=batch)
    assert got[0] == ref[0] == 0, (got[2], ref[2])
    assert sorted(got[1]) == sorted([*ref[1], "PREPROCESS.tsv"])
    for name, data in ref[1].items():
        assert got[1][name] == data, (tag, name)
    assert b"," in got[1]["CLASSIFICATION.csv"]
    check_totals(got[1], want)
    assert "preprocessing: %d reads, %d kept" % (want["n_reads"], want["n_kept"]) in got[2]
    return got[1]


@pytest.fixture(scope="module")
def inputs(env):
    base, r1, single = env["base"], env["r1"], env["single"]
    (base / "raw.fq").write_bytes(fastq(r1))
    (base / "trimmed.fq").write_bytes(fastq(kept_records(r1, single)))
    return base / "raw.fq", base / "trimmed.fq"


def test_filtering_and_scores(env, inputs, tmp_path):
    files = same(env, tmp_path, "a", *inputs, env["single"], "--pos-filter", "--neg-filter", "--scores")
    assert len(files["POS_FILTERING.fq"]) > 1000 and len(files["READ_SCORES.tsv"]) > 1000
    same(env, tmp_path, "b", *inputs, env["single"])                  # counts only: nothing is mapped back


def test_lca_and_several_batches(env, inputs, tmp_path):
    files = same(env, tmp_path, "a", *inputs, env["single"], "-f", "0.7", "--lca", "all", "--lca-reads")
    assert len(files["READ_LCA.tsv"]) > 1000 and "CLADE_COUNTS.tsv" in files
    same(env, tmp_path, "b", *inputs, env["single"], "--pos-filter", "--scores", "-b", "50", batch=50)
    same(env, tmp_path, "c", *inputs, env["single"], "-b", "50", batch=50)


def test_taxonomy_abundance_coverage_best_hits(env, inputs, tmp_path):
    lineages = ["Caudoviricetes;Autographiviridae", "Caudoviricetes;Straboviridae", "Microviridae", ""]
    tax = tmp_path / "taxonomy.tsv"
    tax.write_text("".join(f"{g}\t{lineages[i % 4]}\n" for i, g in enumerate(env["names"])))
    files = same(env, tmp_path, "a", *inputs, env["single"], "-f", "0.7", "--taxonomy", str(tax), "--taxon-reads", "--abundance", "--coverage",
                 "--best-hits")
    assert {"TAXON_COUNTS.tsv", "READ_TAXA.tsv", "ABUNDANCE.tsv", "COVERAGE.tsv"} <= set(files)


def test_two_replicas(env, inputs, tmp_path):
    same(env, tmp_path, "a", *inputs, env["single"], "--devices", "0,0", "--pos-filter", "--scores")
    same(env, tmp_path, "b", *inputs, env["single"], "--devices", "0,0")


def test_pairs(env, tmp_path):
    r1, r2 = env["r1"], env["r2"]
    mates = [m for pair in zip(r1, r2) for m in pair]
    want = prep_ref.prep_block([m[1] for m in mates], [m[2] for m in mates], paired=True, **PARAMS)
    assert want["n_reason"]["mate"] >= 20 and want["n_kept"] >= 100
    kept = kept_records(mates, want)
    for name, recs in (("r1.fq", r1), ("r2.fq", r2), ("t1.fq", kept[0::2]), ("t2.fq", kept[1::2]), ("ri.fq", mates), ("ti.fq", kept)):
        (tmp_path / name).write_bytes(fastq(recs))
    args = ("--pos-filter", "--neg-filter", "--scores")
    files = same(env, tmp_path, "a", tmp_path / "r1.fq", tmp_path / "t1.fq", want, *args, raw_args=("--reads2", str(tmp_path / "r2.fq")),
                 trimmed_args=("--reads2", str(tmp_path / "t2.fq")))
    assert len(files["POS_FILTERING_2.fq"]) > 1000
    same(env, tmp_path, "b", tmp_path / "ri.fq", tmp_path / "ti.fq", want, "--interleaved", *args, "--devices", "0,0", "-b", "20", batch=60)
    same(env, tmp_path, "c", tmp_path / "ri.fq", tmp_path / "ti.fq", want, "--interleaved")


def test_fasta_input_skips_the_quality_steps(env, tmp_path):
    r1 = env["r1"]
    want = prep_ref.prep_block([r[1] for r in r1], None, **PARAMS)
    assert 35 <= want["n_trimmed"] <= 45                              # only the poly-G tails are cut
    assert want["begin"] == [0] * len(r1)
    (tmp_path / "raw.fa").write_bytes(fasta(r1))
    (tmp_path / "trimmed.fa").write_bytes(fasta(kept_records(r1, want)))
    same(env, tmp_path, "a", tmp_path / "raw.fa", tmp_path / "trimmed.fa", want, "--pos-filter", "--neg-filter")


def test_default_min_length_keeps_short_reads_from_every_genome(env, inputs, tmp_path):
    """A read shorter than k has no k-mer and counts at every genome; with any preprocessing option on, --min-length defaults to k
    and those reads are dropped."""
    raw = inputs[0]
    want = prep_ref.prep_block([r[1] for r in env["r1"]], [r[2] for r in env["r1"]], trim_window=4, min_length=K)
    assert want["n_reason"]["short"] >= 20 and want["n_trimmed"] == 0
    (tmp_path / "long.fq").write_bytes(fastq(kept_records(env["r1"], want)))
    plain = query(env, tmp_path / "plain", raw)
    got = query(env, tmp_path / "prep", raw, "--trim-window", "4")
    ref = query(env, tmp_path / "ref", tmp_path / "long.fq")
    assert plain[0] == got[0] == ref[0] == 0
    assert got[1]["CLASSIFICATION.csv"] == ref[1]["CLASSIFICATION.csv"] != plain[1]["CLASSIFICATION.csv"]
