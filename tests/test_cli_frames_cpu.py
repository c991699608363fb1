"""CPU only: the options of `phage_filter query --frame F [--frame-step S]` are checked before any device is used (status 101,
a message that names both options), and the usage text lists them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")
# (no device may be touched: one that is asked for does not exist)
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


def refused(tmp_path, *args):
    out = str(tmp_path / "out")
    p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), *args],
                       capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101, (args, p.returncode, p.stderr)
    assert not os.path.exists(out), "refused before the output directory is touched"
    return p.stderr


@pytest.mark.parametrize("other", [["--reads2", FASTQ], ["--interleaved"], ["--scores"], ["--lca", "all"], ["--lca", "best"],
                                   ["--abundance"], ["--coverage"], ["--shard-depth", "1"], ["--pos-filter"], ["--neg-filter"]])
def test_frame_refuses_the_other_modes(tmp_path, other):
    err = refused(tmp_path, "--frame", "500", *other)
    assert "'--frame'" in err and f"'{other[0]}'" in err, err
    err = refused(tmp_path, *other, "--frame", "500", "--frame-step", "100")
    assert "'--frame'" in err and f"'{other[0]}'" in err, err


def test_frame_step_needs_frame(tmp_path):
    err = refused(tmp_path, "--frame-step", "100")
    assert "'--frame-step'" in err and "'--frame <F>'" in err, err


@pytest.mark.parametrize("name,value", [("frame", "0"), ("frame", "-5"), ("frame", "abc"), ("frame", "12.5"), ("frame", ""), ("frame", "4294967296"),
                                        ("frame-step", "0"), ("frame-step", "-1"), ("frame-step", "1e3"), ("frame-step", "7x")])
def test_values_are_positive_integers(tmp_path, name, value):
    args = ["--frame", value] if name == "frame" else ["--frame", "500", "--frame-step", value]
    err = refused(tmp_path, *args)
    assert f"'--{name}'" in err and f"'{value}'" in err, err


def test_step_larger_than_frame(tmp_path):
    err = refused(tmp_path, "--frame", "100", "--frame-step", "101")
    assert "'--frame-step 101'" in err and "'--frame 100'" in err, err


def test_usage_lists_the_options():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    assert "--frame <F>" in text and "--frame-step <S>" in text and "SEGMENTS.tsv" in text
    assert "sequence<TAB>genome<TAB>begin<TAB>end<TAB>match_begin<TAB>match_end<TAB>frames<TAB>kmers<TAB>matched<TAB>longest_run" in text
