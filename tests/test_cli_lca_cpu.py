"""CPU only: the option errors of `phage_filter query --lca` / `--lca-reads`.  Each ends with status 101 like the existing
option errors, names what is wrong, and is raised before any device is used: with `--devices all` the first device call
(pfq_device_count) would otherwise answer first, with a libpfq message, and nothing is created in --out."""
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
    (["--lca", "deepest"], "invalid value 'deepest' for '--lca' [possible values: all, best]"),
    (["--lca", ""], "possible values: all, best"),
    (["--lca", "ALL"], "possible values: all, best"),
    (["--lca-reads"], "'--lca-reads' needs '--lca <all|best>'"),
    (["--lca-reads", "--scores"], "'--lca-reads' needs '--lca <all|best>'"),
    (["--lca", "all", "--shard-depth", "2"], "'--lca' cannot be used with '--shard-depth'"),
    (["--lca", "best", "--lca-reads", "--shard-depth", "0"], "'--lca' cannot be used with '--shard-depth'"),
])
def test_lca_option_errors_before_any_device(tmp_path, extra, msg):
    p = run(tmp_path, *extra)
    assert p.returncode == 101 and msg in p.stderr, (extra, p.stderr)
    assert "libpfq" not in p.stderr, p.stderr                       # no library call answered first


def test_shard_depth_error_names_the_limitation(tmp_path):
    p = run(tmp_path, "--lca", "all", "--shard-depth", "1")
    assert p.returncode == 101 and "shard" in p.stderr and "whole tree" in p.stderr, p.stderr


def test_lca_needs_a_value(tmp_path):
    p = run(tmp_path, "--lca")
    assert p.returncode == 101 and "value is required" in p.stderr, p.stderr


def test_usage_lists_lca_options():
    p = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert "--lca <all|best>" in p.stderr and "--lca-reads" in p.stderr and "CLADE_COUNTS.tsv" in p.stderr
    assert "READ_LCA.tsv" in p.stderr and "--lca best" in p.stderr
