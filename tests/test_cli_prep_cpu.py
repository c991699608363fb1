"""CPU only: `phage_filter query` with the preprocessing options refuses the modes it does not serve and values out of range before
any device or output directory is touched (status 101, a message that names both options), and the usage text lists the options."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")
# (no device may be touched: one that is asked for does not exist)
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")

OPTIONS = [["--trim-quality", "20"], ["--trim-window", "8"], ["--trim-poly-x", "10"], ["--min-length", "30"], ["--max-n", "3"], ["--min-complexity", "30"]]
REFUSED = [["--device-parse"], ["--frame", "500"], ["--shard-depth", "1"]]


def refused(tmp_path, *args):
    out = str(tmp_path / "out")
    p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), *args],
                       capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101, (args, p.returncode, p.stderr)
    assert not os.path.exists(out), "refused before the output directory is touched"
    return p.stderr


@pytest.mark.parametrize("other", REFUSED, ids=[o[0] for o in REFUSED])
@pytest.mark.parametrize("option", OPTIONS, ids=[o[0] for o in OPTIONS])
def test_refused_combinations(tmp_path, option, other):
    for args in ([*other, *option], [*option, *other]):
        err = refused(tmp_path, *args)
        assert f"'{option[0]}'" in err and f"'{other[0]}'" in err, err


@pytest.mark.parametrize("args", [["--trim-quality", "94"], ["--trim-window", "0"], ["--trim-quality", "20", "--trim-window", "1025"],
                                  ["--min-complexity", "101"], ["--min-length", "0"], ["--max-n", "-1"], ["--trim-quality", "x"],
                                  ["--trim-poly-x", ""]], ids=lambda a: " ".join(a))
def test_values_out_of_range(tmp_path, args):
    err = refused(tmp_path, *args)
    assert f"'{args[-1]}'" in err and f"'{args[-2]}'" in err, err


def test_usage_lists_the_options():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    for o in OPTIONS:
        assert o[0] in text, o[0]
    assert "PREPROCESS.tsv" in text and "before it is classified" in text
