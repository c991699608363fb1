"""`phage_filter query --scores`: READ_SCORES.tsv — per read record and genome it hits, how many of the read's k-mers the
genome's filter contains.  The file must equal one built here from the oracle's hits and k-mer counts on the examples
database; every other output (and stdout) must equal the run without --scores byte for byte; replicas, shards, thread and
block counts must not change the file."""
import gzip
import os
import subprocess

import pytest

from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from test_gpu_scores import Contains

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "examples")
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
TIMEOUT = 300
ENV = dict(os.environ, PFQ_CLI_BATCH_READS="128", PFQ_INGEST_CHUNK_BYTES="20000")
FASTQ = os.path.join(EX, "reads", "sim_reads_c10000_n5_e0.01.fq")


def query(db, reads, out, *extra, threads="4", block="64"):
    p = subprocess.run([CLI, "query", "--reads", reads, "--out", out, "--db-path", db, "--block-size-reads", block,
                        "--threads", threads, *extra], capture_output=True, text=True, env=ENV, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    return p.stdout, files


def fastq_records(path):
    lines = open(path, "rb").read().decode().splitlines()
    return [(lines[i][1:].split(" ")[0], lines[i + 1].encode()) for i in range(0, len(lines) - 3, 4)]


def expected_tsv(ot, records, thr):
    """READ_SCORES.tsv from the oracle: records in input order, genomes by matched k-mers descending, ties in leaf order."""
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    hits, _, _ = orc.query_batch(ot, [s for _, s in records], thr)
    leaves = ot.leaves_dfs()
    col = {v: i for i, v in enumerate(leaves)}
    per_read = {}
    for r, v in hits:
        per_read.setdefault(r, []).append(col[v])
    cont = Contains(ot)
    lines = ["#read_id\tkmers\tgenome\tmatched_kmers\n"]
    for r, (rid, s) in enumerate(records):
        if r not in per_read:
            continue
        kmers = orc.get_kmers(s, ot.kmer_size)
        scored = [(-cont.count(ot.filter_of[leaves[c]], kmers), c) for c in sorted(per_read[r])]
        for neg, c in sorted(scored):
            lines.append(f"{rid}\t{len(kmers)}\t{ot.tax_id[leaves[c]]}\t{-neg}\n")
    return "".join(lines).encode()


@pytest.fixture(scope="module")
def db(gpu, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("scores_cli") / "db")
    p = subprocess.run([CLI, "build-balanced", "--genomes", os.path.join(EX, "genomes"), "--db-path", d],
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    return d


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """FASTQ as shipped; FASTA (gzipped) of 600 of its records plus a duplicate id, a lowercase and an IUPAC record."""
    base = tmp_path_factory.mktemp("scores_in")
    recs = fastq_records(FASTQ)[:600]
    recs += [(recs[3][0], recs[10][1]), ("low", recs[5][1].lower()), ("iupac", recs[7][1][:40] + b"NNRYK" + recs[7][1][45:]),
             ("short", b"ACGT"), ("empty_ish", b"N")]
    fa = str(base / "reads.fa.gz")
    with gzip.open(fa, "wb") as f:
        f.write(b"".join(b">" + rid.encode() + b" some description\n" + s + b"\n" for rid, s in recs))
    return {"fq": (FASTQ, fastq_records(FASTQ)), "fa": (fa, recs)}


@pytest.mark.parametrize("kind", ["fq", "fa"])
@pytest.mark.parametrize("thr", ["1.0", "0.3"])
def test_read_scores_equal_oracle_and_leave_other_outputs_alone(db, inputs, tmp_path, kind, thr):
    reads, records = inputs[kind]
    ot = fmt.read_db(db)
    want = expected_tsv(ot, records, float(thr))
    for extra in ([], ["--pos-filter", "--neg-filter"]):
        out0, files0 = query(db, reads, str(tmp_path / "plain"), "--filter-threshold", thr, *extra)
        out1, files1 = query(db, reads, str(tmp_path / "scores"), "--filter-threshold", thr, "--scores", *extra)
        assert out1 == out0
        assert files1.pop("READ_SCORES.tsv") == want, (kind, thr, extra)
        assert files1 == files0


@pytest.mark.parametrize("thr", ["1.0", "0.3"])
def test_read_scores_do_not_depend_on_devices_shards_threads_blocks(db, inputs, tmp_path, thr):
    reads, _ = inputs["fq"]
    base_out, base = query(db, reads, str(tmp_path / "base"), "--filter-threshold", thr, "--scores", "--pos-filter")
    for i, (extra, threads, block) in enumerate([(["--devices", "0,0"], "4", "64"), (["--devices", "0,0", "--shard-depth", "1"], "4", "64"),
                                                 (["--shard-depth", "2"], "4", "64"), ([], "1", "7"), ([], "16", "1000"),
                                                 (["--search-depth", "3"], "4", "64")]):
        out, files = query(db, reads, str(tmp_path / f"v{i}"), "--filter-threshold", thr, "--scores", "--pos-filter", *extra,
                           threads=threads, block=block)
        if "--search-depth" in extra:
            ot = fmt.read_db(db)
            ot.prune(3)
            assert files["READ_SCORES.tsv"] == expected_tsv(ot, inputs["fq"][1], float(thr))
            continue
        assert files == base, (extra, threads, block)


def test_usage_lists_scores():
    p = subprocess.run([CLI], capture_output=True, text=True, timeout=TIMEOUT)
    assert "--scores" in p.stderr
