"""CPU only: `phage_filter query` with the mate correction options refuses runs without --mate-overlap, the modes that refuse
--mate-overlap and values it cannot take before any device or output directory is touched (status 101, a message that names the
options), and the usage text lists the options."""
import os
import subprocess

import pytest

from test_cli_overlap_cpu import CLI, ENV, FASTQ, REFUSED, refused

OVERLAP = ["--mate-overlap", "30"]
OPTIONS = [["--mate-correct"], ["--mate-correct", "--mate-correct-quality", "25,10"]]


def test_needs_the_mate_overlap(tmp_path):
    for pairs in ([], ["--interleaved"], ["--reads2", FASTQ]):
        for option in OPTIONS:
            err = refused(tmp_path, *option, *pairs)
            assert "'--mate-correct'" in err and "'--mate-overlap <O>'" in err and "needs" in err, err
        err = refused(tmp_path, "--mate-correct", "--trim-quality", "20", "--adapter", "illumina", *pairs)
        assert "'--mate-correct'" in err and "'--mate-overlap <O>'" in err and "needs" in err, err


def test_the_quality_needs_the_flag(tmp_path):
    for more in ([], OVERLAP, [*OVERLAP, "--interleaved"]):
        err = refused(tmp_path, "--mate-correct-quality", "30", *more)
        assert "'--mate-correct-quality'" in err and "'--mate-correct'" in err and "needs" in err, err
    err = refused(tmp_path, *OVERLAP, "--interleaved", "--mate-correct", "--mate-correct-quality")
    assert "a value is required" in err and "--mate-correct-quality" in err


def test_needs_pairs_as_the_overlap_does(tmp_path):
    for option in OPTIONS:
        err = refused(tmp_path, *OVERLAP, *option)
        assert "'--mate-overlap'" in err and "--reads2" in err and "--interleaved" in err and "needs" in err, err


@pytest.mark.parametrize("other", REFUSED, ids=[o[0] for o in REFUSED])
@pytest.mark.parametrize("option", OPTIONS, ids=["flag", "quality"])
def test_refused_where_the_overlap_is(tmp_path, option, other):
    for args in ([*other, *OVERLAP, *option], [*option, *OVERLAP, *other]):
        err = refused(tmp_path, *args)
        assert f"'{other[0]}'" in err and "cannot be used with" in err and ("'--mate-overlap'" in err or "'--mate-correct" in err), err
    err = refused(tmp_path, *option, *OVERLAP, "--interleaved", *other)
    assert f"'{other[0]}'" in err and "cannot be used with" in err, err
    if other[0] == "--device-output":                                 # named itself where it stands alone with it
        err = refused(tmp_path, *other, *option)
        assert "'--device-output'" in err and "'--mate-correct" in err and "cannot be used with" in err, err


@pytest.mark.parametrize("value", ["0", "94", "30,30", "30,31", "14", "10,", ",5", "x", "30,y", "-3", "", "30,14,2", "30;14", "1,1"])
def test_values_that_cannot_be_taken(tmp_path, value):
    err = refused(tmp_path, *OVERLAP, "--interleaved", "--mate-correct", "--mate-correct-quality", value)
    assert f"'{value}'" in err and "--mate-correct-quality" in err and "invalid value" in err and "HI[,LO]" in err, err


def test_valid_options_reach_the_database(tmp_path):
    for args in (["--mate-correct"], ["--mate-correct", "--mate-correct-quality", "30,14"], ["--mate-correct", "--mate-correct-quality=93,92"],
                 ["--mate-correct", "--mate-correct-quality", "1,0"], ["--mate-correct", "--mate-correct-quality", "15"],
                 ["--mate-correct", "--adapter", "illumina", "--trim-quality", "20", "--pos-filter", "--scores"]):
        for pairs in (["--interleaved"], ["--reads2", FASTQ]):
            out = str(tmp_path / "out")
            p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), *OVERLAP, *args, *pairs],
                               capture_output=True, text=True, env=ENV, timeout=60)
            assert p.returncode != 0 and not os.path.exists(out), args
            assert not any(w in p.stderr for w in ("invalid value", "cannot be used", "needs '", "unexpected argument", "a value is required")), (args, p.stderr)
            assert "no HIP device" in p.stderr or "no_such_db" in p.stderr, (args, p.stderr)


def test_usage_lists_the_options():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    for o in ("--mate-correct [--mate-correct-quality <HI[,LO]>]", "corrected_fragments", "corrected_bases", "correct_unresolved", "correct_no_quality",
              "mate_correct_quality", "mate_correct_low", "default 30", "default 14"):
        assert o in text, o
