"""`phage_filter query --gzip-output`: every run is held against the same command without the option.  The POS / NEG files are
then `.gz` files of blocked gzip that end with the end marker and that pfq_gz_scan takes whole; inflated they are, byte for byte,
the plain run's files; CLASSIFICATION.csv, the exit status and stderr (but for the timing lines) are the plain run's."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from phagefilter_amd import gz_scan
from test_gpu_cli_text import CLI, READS, TIMEOUT, db  # noqa: F401  (db: the module's fixture)

pytestmark = pytest.mark.gpu

SMALL = os.path.join(READS, "sim_reads_c10000_n5_e0.0.fq")
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """About 300 reads of the examples (left runs and whole blocks both occur with -b 7 and -b 1000), the same with a repeated
    id, gzipped, as mates, and reads that hit nothing."""
    d = tmp_path_factory.mktemp("gzip_reads")
    lines = open(SMALL, "rb").read().split(b"\n")[:4 * 300]
    rng = np.random.default_rng(31)
    out = {"plain": d / "reads.fq", "repeated": d / "repeated.fq", "gz": d / "reads.fastq.gz", "none": d / "none.fq", "r1": d / "r1.fq", "r2": d / "r2.fq",
           "interleaved": d / "interleaved.fq"}
    out["plain"].write_bytes(b"\n".join(lines) + b"\n")
    rep = list(lines)
    rep[4 * 5] = rep[4 * 3]                                           # record 3's header on record 5
    out["repeated"].write_bytes(b"\n".join(rep) + b"\n")
    out["gz"].write_bytes(gzip.compress(b"\n".join(lines) + b"\n"))
    out["none"].write_bytes(b"".join(b"@n%d\n%s\n+\n%s\n" % (i, bytes(rng.choice(list(b"ACGT"), 150).tolist()), b"I" * 150) for i in range(300)))
    recs = [lines[4 * i:4 * i + 4] for i in range(300)]
    mates = [([b"@f%d/1" % i] + a[1:], [b"@f%d/2" % i] + b[1:]) for i, (a, b) in enumerate(zip(recs[0::2], recs[1::2]))]
    out["r1"].write_bytes(b"".join(b"\n".join(a) + b"\n" for a, _ in mates))
    out["r2"].write_bytes(b"".join(b"\n".join(b) + b"\n" for _, b in mates))
    out["interleaved"].write_bytes(b"".join(b"\n".join(a + b) + b"\n" for a, b in mates))
    return {k: str(v) for k, v in out.items()}


def run(db, reads, out, *args):
    p = subprocess.run([CLI, "query", "--reads", reads, "--out", str(out), "--db-path", db, "--threads", "4", "--pos-filter", "--neg-filter", *args],
                       capture_output=True, text=True, timeout=TIMEOUT)   # (no PFQ_INGEST_TIMING: stderr has no timing line)
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    return p.returncode, files, p.stderr, p.stdout


def same(db, reads, tmp_path, *args, gzip_args=("--gzip-output",)):
    """Both runs; returns the plain run's files and the other's."""
    tmp_path.mkdir(exist_ok=True)
    want = run(db, reads, tmp_path / "plain", *args)
    got = run(db, reads, tmp_path / "gz", *args, *gzip_args)
    assert want[0] == 0 and got[0] == 0 and got[2] == want[2] and got[3] == want[3]
    assert sorted(got[1]) == sorted(n + ".gz" if n.startswith(("POS", "NEG")) else n for n in want[1])
    for name, data in want[1].items():
        if not name.startswith(("POS", "NEG")):
            assert got[1][name] == data, name
            continue
        gz = got[1][name + ".gz"]
        assert gz.endswith(EOF_MARKER), name
        scan = gz_scan(gz)
        assert scan["stop"] == "end" and scan["consumed"] == len(gz) and scan["text_bytes"] == len(data), name
        assert gzip.decompress(gz) == data, name
    assert any(data for name, data in want[1].items() if name.startswith(("POS", "NEG")))
    return want[1], got[1]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device_output"])
@pytest.mark.parametrize("block", ["7", "1000"])
def test_plain_reads(db, reads, tmp_path, block, device):
    plain, gz = same(db, reads["plain"], tmp_path, "-b", block, *(["--device-output"] if device else []))
    assert plain["POS_FILTERING.fq"] and plain["NEG_FILTERING.fq"] is not None


@pytest.mark.parametrize("device", [False, True], ids=["host", "device_output"])
def test_repeated_id_gzip_input_and_replicas(db, reads, tmp_path, device):
    extra = ["--device-output"] if device else []
    same(db, reads["repeated"], tmp_path / "repeated", "-b", "7", *extra)
    same(db, reads["gz"], tmp_path / "gz_input", "-b", "7", *extra)     # the host reader's path
    same(db, reads["plain"], tmp_path / "replicas", "-b", "7", "--devices", "0,0", *extra)
    same(db, reads["plain"], tmp_path / "level", "-b", "7", *extra, gzip_args=("--gzip-output", "--gzip-level", "1"))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device_output"])
def test_nothing_hits(db, reads, tmp_path, device):
    plain, gz = same(db, reads["none"], tmp_path, "-b", "100", *(["--device-output"] if device else []))
    assert plain["POS_FILTERING.fq"] == b"" and gz["POS_FILTERING.fq.gz"] == EOF_MARKER   # the bare end marker
    assert plain["NEG_FILTERING.fq"] == open(reads["none"], "rb").read()


def test_the_device_deflates_what_it_formats(db, reads, tmp_path):
    """Under --device-output the timing line says how many compressed bytes the device made: most of both files with -b 7."""
    out = tmp_path / "out"
    p = subprocess.run([CLI, "query", "--reads", reads["plain"], "--out", str(out), "--db-path", db, "--threads", "4", "--pos-filter", "--neg-filter", "-b", "7",
                        "--device-output", "--gzip-output"], capture_output=True, text=True, env=dict(os.environ, PFQ_INGEST_TIMING="1"), timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    m = re.search(r"device output: (\d+) records formatted on the device, (\d+) by the host formatter; .* deflated on the device to (\d+) bytes", p.stderr)
    assert m, p.stderr
    on_device, on_host, gz_bytes = (int(x) for x in m.groups())
    written = sum(os.path.getsize(out / f) for f in ("POS_FILTERING.fq.gz", "NEG_FILTERING.fq.gz"))
    assert on_device == 300 - 300 % 7 and on_host == 300 % 7 and 0 < gz_bytes < written and gz_bytes > written // 2


def test_mates(db, reads, tmp_path):
    plain, gz = same(db, reads["r1"], tmp_path / "reads2", "-b", "16", "--reads2", reads["r2"])
    assert {"POS_FILTERING_1.fq.gz", "POS_FILTERING_2.fq.gz", "NEG_FILTERING_1.fq.gz", "NEG_FILTERING_2.fq.gz"} <= set(gz)
    same(db, reads["interleaved"], tmp_path / "interleaved", "-b", "16", "--interleaved")


def test_the_filtered_file_feeds_the_next_run(db, reads, tmp_path):
    """NEG_FILTERING.fq.gz as -r with --device-parse --device-inflate gives what the plain NEG_FILTERING.fq gives."""
    plain, gz = same(db, reads["plain"], tmp_path / "first", "-b", "100", "--device-output")
    inputs = {"plain": tmp_path / "neg.fq", "gz": tmp_path / "neg.fq.gz"}
    inputs["plain"].write_bytes(plain["NEG_FILTERING.fq"])
    inputs["gz"].write_bytes(gz["NEG_FILTERING.fq.gz"])
    results = {}
    for kind, path in inputs.items():
        out = tmp_path / ("second_" + kind)
        p = subprocess.run([CLI, "query", "--reads", str(path), "--out", str(out), "--db-path", db, "--threads", "4", "--device-parse", "--device-inflate",
                            "--filter-threshold", "0.5"], capture_output=True, text=True, env=dict(os.environ, PFQ_INGEST_TIMING="1"), timeout=TIMEOUT)
        assert p.returncode == 0, p.stderr
        results[kind] = (open(out / "CLASSIFICATION.csv", "rb").read(), p.stderr)
    assert results["gz"][0] == results["plain"][0]
    assert "device inflate:" in results["gz"][1]


def test_refused_without_a_filter(db, reads, tmp_path):
    for args, needs in ((["--gzip-output"], "'--gzip-output' needs '--pos-filter' or '--neg-filter'"), (["--pos-filter", "--gzip-level", "3"], "'--gzip-level' needs '--gzip-output'"),
                        (["--pos-filter", "--gzip-output", "--gzip-level", "10"], "invalid value '10' for '--gzip-level'")):
        p = subprocess.run([CLI, "query", "--reads", reads["plain"], "--out", str(tmp_path / "out"), "--db-path", db, *args], capture_output=True, text=True, timeout=TIMEOUT)
        assert p.returncode == 101 and needs in p.stderr and not (tmp_path / "out").exists(), args
