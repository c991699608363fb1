"""`phage_filter query --pos-filter --neg-filter --device-output`: the output directory, the exit status and the error message
must be those of the same command without `--device-output`, byte for byte — with every record formatted on the device where the
blocks are whole and their ids differ, through the carry where chunks cut blocks, through the host formatter where an id repeats,
where the host reader takes over and for gzip files.  X and Y are the `device output:` line's records formatted on the device and
by the host formatter."""
import gzip
import os
import re
import subprocess

import pytest

import test_ingest as ing
from test_gpu_cli_text import CLI, READS, TIMEOUT, as_fasta, db, multiline, n_fastq  # noqa: F401  (db: the module's fixture)
from test_text_cpu import MALFORMED_TAILS

pytestmark = pytest.mark.gpu

SMALL = os.path.join(READS, "sim_reads_c10000_n5_e0.0.fq")
BOTH = ("--pos-filter", "--neg-filter")


def run(db, reads, out, *args, chunk=None, threads="4"):
    env = dict(os.environ, PFQ_INGEST_TIMING="1")
    if chunk is not None:
        env["PFQ_INGEST_CHUNK_BYTES"] = str(chunk)
    p = subprocess.run([CLI, "query", "--reads", str(reads), "--out", str(out), "--db-path", db, "--threads", threads, *args],
                       capture_output=True, text=True, env=env, timeout=TIMEOUT)
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))} if os.path.isdir(out) else None
    errors = [l for l in p.stderr.splitlines() if l.startswith("phage_filter:")]
    m = re.search(r"device output: (\d+) records formatted on the device, (\d+) by the host formatter; pfq_text_format", p.stderr)
    return p.returncode, files, errors, (int(m.group(1)), int(m.group(2))) if m else None


def same(db, reads, tmp_path, *args, chunk=None, threads="4", rc=0, filters=BOTH):
    """Both runs; returns (X, Y) of the one with the option."""
    tmp_path.mkdir(exist_ok=True)
    want = run(db, reads, tmp_path / "plain", *filters, *args, chunk=chunk, threads=threads)
    got = run(db, reads, tmp_path / "device", *filters, *args, "--device-output", chunk=chunk, threads=threads)
    assert want[0] == rc and want[3] is None
    assert got[0] == want[0] and got[2] == want[2]
    assert sorted(got[1]) == sorted(want[1])
    for name in want[1]:
        assert got[1][name] == want[1][name], name
    if rc == 0:
        assert sum(len(want[1][n]) for n in want[1] if n.startswith(("POS", "NEG"))) > 0
    return got[3]


def test_golden_reads_are_formatted_on_the_device(db, tmp_path):
    n = n_fastq(READS)
    assert n == 1500 and n_fastq(SMALL) == 500
    assert same(db, READS, tmp_path / "a", "-b", "100") == (1500, 0)               # one chunk per file, whole blocks, ids unique
    assert same(db, SMALL, tmp_path / "b", "-b", "7") == (500 - 500 % 7, 500 % 7)  # the last block is a partial one
    same(db, READS, tmp_path / "c", "-b", "1000")                                  # the reference harness's value


@pytest.mark.parametrize("threads", ["1", "4"])
@pytest.mark.parametrize("chunk", [113, 5000])
def test_blocks_of_one_record_never_reach_the_host(db, tmp_path, chunk, threads):
    assert same(db, READS, tmp_path, "-b", "1", "--devices", "0,0", chunk=chunk, threads=threads) == (1500, 0)


def test_edge_blocks_go_through_the_carry(db, tmp_path):
    x, y = same(db, READS, tmp_path / "b100", "-b", "100", chunk=5000)             # (a chunk holds about 15 records: no whole block in any)
    assert x + y == 1500 and y > 0
    x, y = same(db, READS, tmp_path / "b10", "-b", "10", chunk=20000)              # whole blocks inside the chunks, cut ones at their edges
    assert x + y == 1500 and y > 0 and x > 0


def test_one_filter_and_threshold_zero(db, tmp_path):
    same(db, READS, tmp_path / "pos", "-b", "100", filters=("--pos-filter",))
    same(db, READS, tmp_path / "neg", "-b", "100", chunk=5000, filters=("--neg-filter",))
    same(db, SMALL, tmp_path / "zero", "-b", "100", "--filter-threshold", "0.0")   # every record mapped to every genome
    same(db, SMALL, tmp_path / "lca", "-b", "64", "--lca", "all", "--filter-threshold", "0.5", chunk=5000)


def test_a_repeated_id_sends_its_block_to_the_host(db, tmp_path):
    lines = open(SMALL, "rb").read().split(b"\n")
    lines[4 * 5] = lines[4 * 3]                                       # record 3's header on record 5
    p = tmp_path / "repeated.fq"
    p.write_bytes(b"\n".join(lines))
    x, y = same(db, p, tmp_path / "a", "-b", "100")
    assert y >= 100 and x + y == 500
    same(db, p, tmp_path / "b", "-b", "10", chunk=5000)


def test_fasta_under_a_fastq_name(db, tmp_path):
    p = tmp_path / "reads.fq"
    p.write_bytes(as_fasta(SMALL))
    for chunk in (700, None):
        x, y = same(db, p, tmp_path / str(chunk), "-b", "100", chunk=chunk)
        assert x + y == 500


def test_directory_of_plain_gzip_and_empty_files(db, tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    a = open(SMALL, "rb").read()
    b = open(os.path.join(READS, "sim_reads_c10000_n5_e0.01.fq"), "rb").read()
    (d / "a.fq").write_bytes(a)
    (d / "b.fastq.gz").write_bytes(gzip.compress(b))
    (d / "d.fq").write_bytes(b"")
    x, y = same(db, d, tmp_path / "run", "-b", "100", chunk=20000)
    assert x + y == 1500 and y >= len(ing.parse_fastq(b))             # gzip streams keep the host reader and the host formatter


def test_file_that_turns_multi_line(db, tmp_path):
    data = open(SMALL, "rb").read()
    recs = ing.parse_fastq(data)
    half = len(recs) // 2
    head = data[:sum(len(l) + 1 for l in data.split(b"\n")[:4 * half])]
    p = tmp_path / "turns.fq"
    p.write_bytes(head + multiline(recs[half:]))
    for chunk in (3000, None):
        x, y = same(db, p, tmp_path / str(chunk), "-b", "50", chunk=chunk)
        assert y > 0 and x + y == len(recs)
        if chunk is None:
            assert (x, y) == (half, len(recs) - half)                 # five whole blocks on the device, the multi-line half on the host


@pytest.mark.parametrize("tail", [MALFORMED_TAILS[1], MALFORMED_TAILS[5]], ids=["no_quality", "two_sequence_lines"])
def test_malformed_tail(db, tmp_path, tail):
    p = tmp_path / "bad.fq"
    p.write_bytes(open(SMALL, "rb").read() + tail)
    for chunk in (5000, None):
        same(db, p, tmp_path / str(chunk), "-b", "100", chunk=chunk, rc=101)   # the outputs of the records before the error too
