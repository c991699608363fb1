"""CPU only: `phage_filter query` with the adapter options refuses the modes it does not serve and values it cannot take before any
device or output directory is touched (status 101, a message that names the options), and the usage text lists the options."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")
# (no device may be touched: one that is asked for does not exist)
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")

AD = ["--adapter", "AGATCGGAAGAGC"]
OPTIONS = [AD, ["--adapter=illumina,nextera"], [*AD, "--adapter-overlap", "6"], [*AD, "--adapter-errors", "20"]]
REFUSED = [["--device-parse"], ["--device-output", "--pos-filter"], ["--frame", "500"], ["--shard-depth", "1"]]


def refused(tmp_path, *args):
    out = str(tmp_path / "out")
    p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), *args],
                       capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101, (args, p.returncode, p.stderr)
    assert not os.path.exists(out), "refused before the output directory is touched"
    return p.stderr


@pytest.mark.parametrize("other", REFUSED, ids=[o[0] for o in REFUSED])
@pytest.mark.parametrize("option", OPTIONS, ids=["adapter", "presets", "overlap", "errors"])
def test_refused_combinations(tmp_path, option, other):
    for args in ([*other, *option], [*option, *other]):
        err = refused(tmp_path, *args)
        assert "'--adapter" in err and f"'{other[0]}'" in err and "cannot be used with" in err, err


@pytest.mark.parametrize("args,named", [
    (["--adapter", "AGATCGGAAGAGX"], "AGATCGGAAGAGX"),                 # another letter
    (["--adapter", "AGATCGGAAGAGC,ACGN"], "ACGN"),
    (["--adapter", "ACGT"], "ACGT"),                                  # shorter than the default overlap
    (["--adapter", "ACGTACGT", "--adapter-overlap", "9"], "ACGTACGT"),
    (["--adapter", "A" * 65], "A" * 65),                              # longer than 64
    (["--adapter", "AGATCGGAAGAGC,,ACGTACGT"], "''"),                  # an empty entry
    (["--adapter", "truseq"], "truseq"),                              # no such preset
    (["--adapter", ",".join(["ACGTACGTA"] * 9)], "at most 8"),
    (["--adapter", "ACGTACGTA,ACGTACGTC,ACGTACGTG,ACGTACGTT,ACGTACCTA", "--adapter", "CCGTACGTA,CCGTACGTC,CCGTACGTG,CCGTACGTT"], "at most 8"),
    (["--adapter", "illumina", "--adapter-overlap", "0"], "'0'"),
    (["--adapter", "illumina", "--adapter-overlap", "65"], "'65'"),
    (["--adapter", "illumina", "--adapter-overlap", "x"], "'x'"),
    (["--adapter", "illumina", "--adapter-errors", "51"], "'51'"),
    (["--adapter", "illumina", "--adapter-errors", "-1"], "'-1'"),
    (["--adapter", "illumina", "--trim-quality", "94"], "'94'"),
], ids=lambda a: " ".join(a)[:60] if isinstance(a, list) else None)
def test_values_that_cannot_be_taken(tmp_path, args, named):
    err = refused(tmp_path, *args)
    assert named in err and args[-2] in err and "invalid value" in err, err


def test_options_that_need_another(tmp_path):
    err = refused(tmp_path, "--adapter2", "illumina", "--interleaved")
    assert "'--adapter2'" in err and "'--adapter <SEQ>'" in err
    err = refused(tmp_path, "--adapter-overlap", "7")
    assert "'--adapter-overlap'" in err and "'--adapter <SEQ>'" in err
    err = refused(tmp_path, "--adapter-errors", "7")
    assert "'--adapter-errors'" in err and "'--adapter <SEQ>'" in err
    err = refused(tmp_path, "--adapter", "illumina", "--adapter2", "nextera")
    assert "'--adapter2'" in err and "--reads2" in err and "--interleaved" in err
    err = refused(tmp_path, "--adapter")
    assert "a value is required" in err and "--adapter" in err


def test_valid_options_reach_the_database(tmp_path):
    """Accepted: presets, lower case, repeated options, the bounds of O and E — the run then goes on to open the database and fails
    there, at the device that is hidden or the directory that is missing (still no output directory)."""
    for args in (["--adapter", "illumina,nextera", "--adapter", "smallrna"], ["--adapter", "agatcggaagagc", "--adapter-overlap", "13"],
                 ["--adapter", "A" * 64, "--adapter-overlap", "64", "--adapter-errors", "50"],
                 ["--adapter=ACGTA", "--adapter-overlap", "1", "--adapter-errors", "0"],
                 ["--adapter", "illumina", "--adapter2", "nextera,ACGTACGT", "--adapter2", "smallrna", "--reads2", FASTQ]):
        out = str(tmp_path / "out")
        p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), *args],
                           capture_output=True, text=True, env=ENV, timeout=60)
        assert p.returncode != 0 and not os.path.exists(out), args
        assert not any(w in p.stderr for w in ("invalid value", "cannot be used", "needs '", "unexpected argument", "a value is required")), (args, p.stderr)
        assert "no HIP device" in p.stderr or "no_such_db" in p.stderr, (args, p.stderr)     # the options passed: the run went on to open the database


def test_usage_lists_the_options():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    for o in ("--adapter <SEQ", "--adapter2", "--adapter-overlap", "--adapter-errors", "illumina", "nextera", "smallrna", "AGATCGGAAGAGC",
              "CTGTCTCTTATACACATCT", "TGGAATTCTCGGGTGCCAAGG", "adapter_reads", "adapter1.<SEQ>"):
        assert o in text, o
