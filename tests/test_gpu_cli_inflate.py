"""`phage_filter query --device-parse --device-inflate`: the output directory, the exit status and the error message must be those
of the same command without the two options, byte for byte — on blocked gzip (BGZF) files whose members the device inflates, on
files the device hands to the streaming host reader (foreign bytes, plain gzip members, corrupt and truncated members, records
that are not ordinary) and on gzip files that are not BGZF at all."""
import gzip
import os
import re
import subprocess

import pytest

import bgzf_ref as B
import test_ingest as ing
from test_gpu_cli_text import CLI, READS, SEEDS, TIMEOUT, EX, as_fasta, multiline, n_fastq

pytestmark = pytest.mark.gpu

FQ = os.path.join(READS, "sim_reads_c10000_n5_e0.0.fq")


@pytest.fixture(scope="module")
def db(gpu, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("inflate_cli") / "db")
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
    m = re.search(r"device inflate: (\d+) members inflated on the device, (\d+) handed to the host reader", p.stderr)
    r = re.search(r"device parse: (\d+) records parsed on the device, (\d+) by the host reader", p.stderr)
    return p.returncode, files, errors, (int(m.group(1)), int(m.group(2))) if m else None, (int(r.group(1)), int(r.group(2))) if r else None


def same(db, reads, tmp_path, *args, chunk=None, threads="4", rc=0):
    """Both runs; returns ((members on the device, members handed over), (device records, host records)) of the one with the options."""
    want = run(db, reads, tmp_path / "plain", *args, chunk=chunk, threads=threads)
    got = run(db, reads, tmp_path / "device", *args, "--device-parse", "--device-inflate", chunk=chunk, threads=threads)
    assert want[0] == rc and want[3] is None
    assert got[:3] == want[:3]
    if rc == 0:
        assert b"," in got[1]["CLASSIFICATION.csv"]                  # (something was classified)
    return got[3], got[4]


def golden_bgzf(d, block):
    """The golden reads, file by file, as BGZF; returns the members of all files (end markers included)."""
    d.mkdir()
    n = 0
    for f in sorted(os.listdir(READS)):
        gz = B.write(open(os.path.join(READS, f), "rb").read(), block)
        (d / (f + ".gz")).write_bytes(gz)
        n += len(B.scan(gz)[0]) - 1
    return n


@pytest.mark.parametrize("threads", ["1", "4"])
@pytest.mark.parametrize("chunk", [5000, None])
@pytest.mark.parametrize("block", [B.BLOCK, 997])
def test_golden_reads_as_bgzf(db, tmp_path, block, chunk, threads):
    n = golden_bgzf(tmp_path / "in", block)                            # (members of 997 bytes: records span members and chunks)
    assert same(db, tmp_path / "in", tmp_path, chunk=chunk, threads=threads) == ((n, 0), (n_fastq(READS), 0))


def test_two_replicas_and_lca(db, tmp_path):
    n = golden_bgzf(tmp_path / "in", 997)
    for name, args in (("a", ("--devices", "0,0")), ("b", ("--lca", "all", "--filter-threshold", "0.5"))):
        (tmp_path / name).mkdir()
        assert same(db, tmp_path / "in", tmp_path / name, *args, chunk=5000) == ((n, 0), (n_fastq(READS), 0))
    assert os.path.exists(tmp_path / "b" / "device" / "CLADE_COUNTS.tsv")


def test_fasta_as_bgzf(db, tmp_path):
    data = as_fasta(FQ)
    p = tmp_path / "reads.fa.gz"
    gz = B.write(data, 997)
    p.write_bytes(gz)
    for chunk in (3000, None):
        (tmp_path / str(chunk)).mkdir()
        assert same(db, p, tmp_path / str(chunk), chunk=chunk) == ((len(B.scan(gz)[0]) - 1, 0), (len(ing.parse_fasta(data)), 0))


def test_plain_gzip_keeps_the_host_reader(db, tmp_path):
    data = open(FQ, "rb").read()
    p = tmp_path / "reads.fq.gz"
    p.write_bytes(gzip.compress(data))
    assert same(db, p, tmp_path) == ((0, 0), (0, len(ing.parse_fastq(data))))


def two_halves():
    data = open(FQ, "rb").read()
    recs = ing.parse_fastq(data)
    cut = len(data) // 2 + 17                                          # (inside a record)
    return data, recs, cut


@pytest.mark.parametrize("what", ["gzip_member_behind", "junk_behind", "junk_between"])
def test_foreign_bytes(db, tmp_path, what):
    data, recs, cut = two_halves()
    head = B.write(data[:cut], 997, marker=False)
    n_head = len(B.scan(head)[0]) - 1
    junk = b"this is not gzip, and it is long enough to be looked at as a header\n" * 3
    if what == "gzip_member_behind":                                   # zlib reads on through the plain member: every record
        gz = head + gzip.compress(data[cut:])
    elif what == "junk_behind":                                        # zlib ignores what follows the last member: the file ends inside a record
        gz = head + junk
    else:                                                              # ... and everything behind the junk
        gz = head + junk + B.write(data[cut:], 997)
    p = tmp_path / "reads.fq.gz"
    p.write_bytes(gz)
    rc = 0 if what == "gzip_member_behind" else None
    for chunk in (5000, None):
        (tmp_path / str(chunk)).mkdir()
        want = run(db, p, tmp_path / str(chunk) / "plain", chunk=chunk)
        got = run(db, p, tmp_path / str(chunk) / "device", "--device-parse", "--device-inflate", chunk=chunk)
        assert got[:3] == want[:3] and (rc is None or want[0] == rc)
        if want[0] == 0:                                               # (a run that fails prints no report)
            members, records = got[3], got[4]
            assert members[0] > 0 and members[0] + members[1] == n_head    # the members in front were inflated on the device
            assert records[0] > 0
        if rc == 0:
            assert got[4][1] > 0 and sum(got[4]) == len(recs)


@pytest.mark.parametrize("what", ["corrupt_member", "truncated"])
def test_broken_files_fail_alike(db, tmp_path, what):
    data = open(FQ, "rb").read()
    gz = B.write(data, 997)
    begin = B.scan(gz)[0]
    mid = len(begin) // 2
    if what == "corrupt_member":
        h, _ = B.payload_of(gz[begin[mid]:begin[mid + 1]])
        at = begin[mid] + h + 20
        gz = gz[:at] + bytes([gz[at] ^ 0x55]) + gz[at + 1:]
    else:
        gz = gz[:begin[mid] + 100]
    p = tmp_path / "reads.fq.gz"
    p.write_bytes(gz)
    for chunk in (5000, None):
        (tmp_path / str(chunk)).mkdir()
        want = run(db, p, tmp_path / str(chunk) / "plain", chunk=chunk)
        got = run(db, p, tmp_path / str(chunk) / "device", "--device-parse", "--device-inflate", chunk=chunk)
        assert want[0] != 0 and want[2]
        assert got[:3] == want[:3]


def test_file_that_turns_multi_line(db, tmp_path):
    data = open(FQ, "rb").read()
    recs = ing.parse_fastq(data)
    half = len(recs) // 2
    head = data[:sum(len(l) + 1 for l in data.split(b"\n")[:4 * half])]
    text = head + multiline(recs[half:])
    p = tmp_path / "turns.fq.gz"
    gz = B.write(text, 997)
    p.write_bytes(gz)
    n = len(B.scan(gz)[0]) - 1
    for chunk in (3000, None):
        (tmp_path / str(chunk)).mkdir()
        members, records = same(db, p, tmp_path / str(chunk), chunk=chunk)
        assert sum(records) == len(recs) and records[1] >= len(recs) - half and sum(members) == n and members[1] > 0
        if chunk == 3000:
            assert records[0] > 0 and members[0] > 0


def test_directory_of_plain_gzip_and_bgzf_files(db, tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    a = open(FQ, "rb").read()
    b = open(os.path.join(READS, "sim_reads_c10000_n5_e0.01.fq"), "rb").read()
    gz = B.write(b, 997)
    (d / "a.fq").write_bytes(a)
    (d / "b.fastq.gz").write_bytes(gzip.compress(b))
    (d / "c.fq.gz").write_bytes(gz)
    fa = B.write(as_fasta(FQ))
    (d / "d.fa.gz").write_bytes(fa)
    (d / "e.fq.gz").write_bytes(B.EOF_MARKER)
    (d / "f.fq").write_bytes(b"")
    members, records = same(db, d, tmp_path, chunk=20000)
    assert members == (len(B.scan(gz)[0]) - 1 + len(B.scan(fa)[0]) - 1 + 1, 0)
    assert records == (2 * len(ing.parse_fastq(a)) + len(ing.parse_fastq(b)), len(ing.parse_fastq(b)))


def test_needs_device_parse(db, tmp_path):
    got = run(db, FQ, tmp_path / "out", "--device-inflate")
    assert got[0] != 0 and got[2] and "--device-parse" in got[2][0] and got[1] is None
