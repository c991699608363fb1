"""CPU only: `phage_filter query --device-parse` serves the runs that only count.  Every other mode is refused before any device
is used (status 101, a message that names both options, no output directory), and the usage text lists the option."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")
# (no device may be touched: one that is asked for does not exist)
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")

REFUSED = [["--pos-filter"], ["--neg-filter"], ["--scores"], ["--lca", "best"], ["--lca", "all", "--lca-reads"], ["--reads2", FASTQ],
           ["--interleaved"], ["--abundance"], ["--coverage"], ["--frame", "500"], ["--shard-depth", "1"]]


def refused(tmp_path, *args):
    out = str(tmp_path / "out")
    p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), *args],
                       capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101, (args, p.returncode, p.stderr)
    assert not os.path.exists(out), "refused before the output directory is touched"
    return p.stderr


@pytest.mark.parametrize("other", REFUSED, ids=[" ".join(o[:2]) if o[0] == "--lca" else o[0] for o in REFUSED])
def test_device_parse_refuses_the_other_modes(tmp_path, other):
    named = "'--lca best'" if other[:2] == ["--lca", "best"] else f"'{other[-1] if other[0] == '--lca' else other[0]}'"
    for args in ([*other, "--device-parse"], ["--device-parse", *other]):
        err = refused(tmp_path, *args)
        assert "'--device-parse'" in err and named in err, err


def test_usage_lists_the_option():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    assert "--device-parse" in text and "parsed on the GPU" in text
