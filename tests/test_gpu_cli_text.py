"""`phage_filter query --device-parse`: the output directory, the exit status and the error message must be those of the same
command without the option, byte for byte — on ordinary files (every record parsed on the device), on files the device hands
back to the host reader half-way (multi-line records, boundary guesses that are wrong, malformed tails), on gzip files."""
import gzip
import os
import re
import subprocess

import pytest

import test_ingest as ing
from test_text_cpu import ADVERSARIAL, MALFORMED_TAILS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "examples")
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
READS = os.path.join(EX, "reads")
TIMEOUT = 300
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)


@pytest.fixture(scope="module")
def db(gpu, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("text_cli") / "db")
    p = subprocess.run([CLI, "build", "--genomes", os.path.join(EX, "genomes"), "--db-path", path, "--seed1", str(SEEDS[0]),
                        "--seed2", str(SEEDS[1])], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    return path


def run(db, reads, out, *args, chunk=None, threads="4"):
    env = dict(os.environ, PFQ_INGEST_TIMING="1")
    if chunk is not None:
        env["PFQ_INGEST_CHUNK_BYTES"] = str(chunk)
    p = subprocess.run([CLI, "query", "--reads", str(reads), "--out", str(out), "--db-path", db, "--threads", threads, *args],
                       capture_output=True, text=True, env=env, timeout=TIMEOUT)
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))} if os.path.isdir(out) else None
    errors = [l for l in p.stderr.splitlines() if l.startswith("phage_filter:")]
    m = re.search(r"device parse: (\d+) records parsed on the device, (\d+) by the host reader", p.stderr)
    return p.returncode, files, errors, (int(m.group(1)), int(m.group(2))) if m else None


def same(db, reads, tmp_path, *args, chunk=None, threads="4", rc=0):
    """Both runs; returns (device records, host records) of the one with the option."""
    want = run(db, reads, tmp_path / "plain", *args, chunk=chunk, threads=threads)
    got = run(db, reads, tmp_path / "device", *args, "--device-parse", chunk=chunk, threads=threads)
    assert want[0] == rc and want[3] is None
    assert got[:3] == want[:3]
    if rc == 0:
        assert b"," in got[1]["CLASSIFICATION.csv"]                  # (something was classified)
    return got[3]


def n_fastq(path):
    return sum(len(ing.parse_fastq(open(os.path.join(path, f), "rb").read())) for f in os.listdir(path)) if os.path.isdir(path) \
        else len(ing.parse_fastq(open(path, "rb").read()))


@pytest.mark.parametrize("threads", ["1", "4"])
@pytest.mark.parametrize("chunk", [113, 5000, None])
def test_golden_reads(db, tmp_path, chunk, threads):
    assert same(db, READS, tmp_path, chunk=chunk, threads=threads) == (n_fastq(READS), 0)   # every record parsed on the device


def test_two_replicas_and_lca(db, tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    assert same(db, READS, tmp_path / "a", "--devices", "0,0", chunk=5000) == (n_fastq(READS), 0)
    assert same(db, READS, tmp_path / "b", "--lca", "all", "--filter-threshold", "0.5", chunk=5000) == (n_fastq(READS), 0)
    assert os.path.exists(tmp_path / "b" / "device" / "CLADE_COUNTS.tsv")


def as_fasta(fastq_path):
    recs = ing.parse_fastq(open(fastq_path, "rb").read())
    return b"".join(b">" + rid + b" x\n" + b"\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + b"\n" for _, rid, seq, _ in recs)


def test_fasta_under_a_fastq_name(db, tmp_path):
    p = tmp_path / "reads.fq"
    p.write_bytes(as_fasta(os.path.join(READS, "sim_reads_c10000_n5_e0.0.fq")))
    n = len(ing.parse_fasta(p.read_bytes()))
    for chunk in (700, None):
        (tmp_path / str(chunk)).mkdir()
        assert same(db, p, tmp_path / str(chunk), chunk=chunk) == (n, 0)


def test_directory_of_plain_and_gzip_files(db, tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    a = open(os.path.join(READS, "sim_reads_c10000_n5_e0.0.fq"), "rb").read()
    b = open(os.path.join(READS, "sim_reads_c10000_n5_e0.01.fq"), "rb").read()
    (d / "a.fq").write_bytes(a)
    (d / "b.fastq.gz").write_bytes(gzip.compress(b))
    (d / "c.fa").write_bytes(as_fasta(os.path.join(READS, "sim_reads_c10000_n5_e0.0.fq")))
    (d / "d.fq").write_bytes(b"")
    n_dev, n_host = same(db, d, tmp_path, chunk=20000)
    assert n_dev == 2 * len(ing.parse_fastq(a)) and n_host == len(ing.parse_fastq(b))      # gzip streams keep the host reader


def multiline(records):
    return b"".join(b"@" + rid + b"\n" + seq[:len(seq) // 2] + b"\n" + seq[len(seq) // 2:] + b"\n+\n" + q[:3] + b"\n" + q[3:] + b"\n"
                    for _, rid, seq, q in records)


def test_file_that_turns_multi_line(db, tmp_path):
    data = open(os.path.join(READS, "sim_reads_c10000_n5_e0.0.fq"), "rb").read()
    recs = ing.parse_fastq(data)
    half = len(recs) // 2
    head = data[:sum(len(l) + 1 for l in data.split(b"\n")[:4 * half])]
    p = tmp_path / "turns.fq"
    p.write_bytes(head + multiline(recs[half:]))
    assert len(ing.parse_fastq(p.read_bytes())) == len(recs)
    for chunk in (3000, None):
        (tmp_path / str(chunk)).mkdir()
        n_dev, n_host = same(db, p, tmp_path / str(chunk), chunk=chunk)
        assert n_dev > 0 and n_host > 0 and n_dev + n_host == len(recs)
        if chunk is None:
            assert (n_dev, n_host) == (half, len(recs) - half)


def test_adversarial_file(db, tmp_path):
    p = tmp_path / "adversarial.fq"
    p.write_bytes(ADVERSARIAL)
    for chunk in (113, 4096):
        (tmp_path / str(chunk)).mkdir()
        n_dev, n_host = same(db, p, tmp_path / str(chunk), "--filter-threshold", "0.0", chunk=chunk)
        assert n_dev + n_host == 300


@pytest.mark.parametrize("tail", [MALFORMED_TAILS[1], MALFORMED_TAILS[3], MALFORMED_TAILS[5]], ids=["no_quality", "no_header", "two_sequence_lines"])
def test_malformed_tail(db, tmp_path, tail):
    good = open(os.path.join(READS, "sim_reads_c10000_n5_e0.0.fq"), "rb").read()
    p = tmp_path / "bad.fq"
    p.write_bytes(good + tail)
    for chunk in (5000, None):
        (tmp_path / str(chunk)).mkdir()
        same(db, p, tmp_path / str(chunk), chunk=chunk, rc=101)


def test_wrong_guess_is_parsed_again_on_the_device(db, tmp_path):
    """Ordinary four-line records whose quality lines begin with '@': near the end of the file such a line followed by one last
    record passes the worker's trial parse (a three-line record, then the end), so the chunk's guessed start is wrong.  The proof
    fails, the device parses the chunk again from the proven position, and every record is still parsed on the device."""
    recs = ing.parse_fastq(open(os.path.join(READS, "sim_reads_c10000_n5_e0.0.fq"), "rb").read())[:60]
    data = b"".join(b"@" + rid + b"\n" + seq + b"\n+\n@" + q[1:] + b"\n" for _, rid, seq, q in recs)
    assert len(ing.parse_fastq(data)) == 60
    p = tmp_path / "at_qualities.fq"
    p.write_bytes(data)
    for chunk in (50, 113, 1000):
        (tmp_path / str(chunk)).mkdir()
        assert same(db, p, tmp_path / str(chunk), chunk=chunk) == (60, 0)
