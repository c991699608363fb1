"""CPU only: the option errors of `phage_filter query --abundance` / `--abundance-iters`.  Each ends with status 101 like the
existing option errors, names what is wrong, and is raised before any device is used: with `--devices all` the first device
call (pfq_device_count) would otherwise answer first, with a libpfq message, and nothing is created in --out."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")


def run(tmp_path, *extra):
    out = tmp_path / "out"
    p = subprocess.run([CLI, "query", "-r", FASTQ, "-o", str(out), "-d", str(tmp_path / "no_db"), "--devices", "all", *extra],
                       capture_output=True, text=True, timeout=60)
    assert not out.exists(), extra
    return p


@pytest.mark.parametrize("extra,msg", [
    (["--abundance", "--shard-depth", "1"], "'--abundance' cannot be used with '--shard-depth'"),
    (["--abundance", "--abundance-iters", "3", "--shard-depth", "0"], "'--abundance' cannot be used with '--shard-depth'"),
    (["--abundance-iters", "5"], "'--abundance-iters' needs '--abundance'"),
    (["--abundance-iters", "5", "--scores"], "'--abundance-iters' needs '--abundance'"),
    (["--abundance", "--abundance-iters", "x"], "invalid value 'x' for '--abundance-iters'"),
    (["--abundance", "--abundance-iters", "0"], "invalid value '0' for '--abundance-iters'"),
    (["--abundance", "--abundance-iters", "-3"], "invalid value '-3' for '--abundance-iters'"),
])
def test_abundance_option_errors_before_any_device(tmp_path, extra, msg):
    p = run(tmp_path, *extra)
    assert p.returncode == 101 and msg in p.stderr, (extra, p.stderr)
    assert "libpfq" not in p.stderr, p.stderr                       # no library call answered first


def test_shard_depth_error_names_the_limitation(tmp_path):
    p = run(tmp_path, "--abundance", "--shard-depth", "1")
    assert p.returncode == 101 and "shard" in p.stderr and "partial" in p.stderr, p.stderr


def test_abundance_iters_needs_a_value(tmp_path):
    p = run(tmp_path, "--abundance", "--abundance-iters")
    assert p.returncode == 101 and "value is required" in p.stderr, p.stderr


def test_usage_lists_abundance_options():
    p = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert "--abundance:" in p.stderr and "--abundance-iters <N>" in p.stderr and "ABUNDANCE.tsv" in p.stderr
    assert "hit-list rate" in p.stderr and "--shard-depth" in p.stderr
