"""CPU only: `phage_filter query --deplete` refuses, before any device, read or output directory is touched (status 101), the modes
preprocessing does not serve with a message that names --deplete, --deplete-threshold on its own or with a value that is no
number, a fifth screen and a screen directory without a readable tree.bin; the usage text describes the option."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")
# (no device may be touched: one that is asked for does not exist)
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")

REFUSED = [["--device-parse"], ["--frame", "500"], ["--shard-depth", "1"], ["--device-output", "--neg-filter"]]


def refused(tmp_path, *args):
    out = str(tmp_path / "out")
    p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), *args],
                       capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101, (args, p.returncode, p.stderr)
    assert not os.path.exists(out), "refused before the output directory is touched"
    return p.stderr


@pytest.fixture
def screen(tmp_path):
    """A directory that passes for a screen until it is opened: these runs end before that."""
    d = tmp_path / "screen"
    d.mkdir()
    (d / "tree.bin").write_bytes(b"")
    return str(d)


@pytest.mark.parametrize("other", REFUSED, ids=[o[0] for o in REFUSED])
def test_refused_combinations(tmp_path, screen, other):
    for args in ([*other, "--deplete", screen], ["--deplete", screen, *other], ["--trim-quality", "20", "--deplete", screen, *other]):
        err = refused(tmp_path, *args)
        assert "'--deplete'" in err and f"'{other[0]}'" in err, err


def test_threshold_needs_a_screen_and_a_number(tmp_path, screen):
    err = refused(tmp_path, "--deplete-threshold", "0.7")
    assert "'--deplete-threshold'" in err and "'--deplete <DIR>'" in err, err
    err = refused(tmp_path, "--deplete", screen, "--deplete-threshold", "x")
    assert "'x'" in err and "deplete-threshold" in err, err


def test_at_most_four_screens(tmp_path, screen):
    err = refused(tmp_path, *(["--deplete", screen] * 5))
    assert "'--deplete'" in err and "5 times" in err and "at most 4" in err, err


def test_a_screen_without_tree_bin_fails_before_any_read_is_parsed(tmp_path, screen):
    empty = tmp_path / "empty"
    empty.mkdir()
    for missing in (str(empty), str(tmp_path / "nowhere")):
        err = refused(tmp_path, "--deplete", screen, "--deplete", missing)
        assert "'--deplete'" in err and missing + "/tree.bin" in err, err
    # ... and a malformed read file is never looked at
    bad = tmp_path / "bad.fq"
    bad.write_bytes(b"@r\nACGT\n+\nII\n")
    out = str(tmp_path / "out")
    p = subprocess.run([CLI, "query", "--reads", str(bad), "--out", out, "--db-path", str(tmp_path / "no_such_db"), "--deplete", str(empty)],
                       capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101 and "tree.bin" in p.stderr and not os.path.exists(out)


def test_usage_describes_the_option():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    for word in ("--deplete <DIR>", "--deplete-threshold <T>", "DEPLETION.csv", "DEPLETION_1.csv", "once per replica", "depleted_units", "depleted_reads",
                 "depleted_bases", "deplete_db", "deplete_threshold"):
        assert word in text, word
