"""CPU only: `phage_filter query` with the mate overlap options refuses runs without pairs, the modes preprocessing does not serve
and values it cannot take before any device or output directory is touched (status 101, a message that names the options), and
the usage text lists the options."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")
# (no device may be touched: one that is asked for does not exist)
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")

OPTIONS = [["--mate-overlap", "30"], ["--mate-overlap=20", "--mate-overlap-errors", "5"]]
REFUSED = [["--device-parse"], ["--device-output", "--pos-filter"], ["--frame", "500"], ["--shard-depth", "1"]]


def refused(tmp_path, *args):
    out = str(tmp_path / "out")
    p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), *args],
                       capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101, (args, p.returncode, p.stderr)
    assert not os.path.exists(out), "refused before the output directory is touched"
    return p.stderr


@pytest.mark.parametrize("other", REFUSED, ids=[o[0] for o in REFUSED])
@pytest.mark.parametrize("option", OPTIONS, ids=["overlap", "errors"])
def test_refused_combinations(tmp_path, option, other):
    for args in ([*other, *option], [*option, *other]):
        err = refused(tmp_path, *args)
        assert "'--mate-overlap'" in err and f"'{other[0]}'" in err and "cannot be used with" in err, err
    if other[0] != "--shard-depth":                                   # with pairs these modes refuse the pairs themselves
        for pairs in (["--interleaved"], ["--reads2", FASTQ]):
            err = refused(tmp_path, *option, *pairs, *other)
            assert f"'{other[0]}'" in err and "cannot be used with" in err, err
    else:
        err = refused(tmp_path, *option, "--interleaved", *other)
        assert "'--mate-overlap'" in err and "'--shard-depth'" in err and "cannot be used with" in err, err


def test_needs_pairs(tmp_path):
    for option in OPTIONS:
        err = refused(tmp_path, *option)
        assert "'--mate-overlap'" in err and "--reads2" in err and "--interleaved" in err and "needs" in err, err
        err = refused(tmp_path, *option, "--adapter", "illumina", "--trim-quality", "20")
        assert "'--mate-overlap'" in err and "--reads2" in err and "--interleaved" in err, err


def test_options_that_need_another(tmp_path):
    for pairs in ([], ["--interleaved"]):
        err = refused(tmp_path, "--mate-overlap-errors", "7", *pairs)
        assert "'--mate-overlap-errors'" in err and "'--mate-overlap <O>'" in err and "needs" in err, err
    err = refused(tmp_path, "--mate-overlap")
    assert "a value is required" in err and "--mate-overlap" in err


@pytest.mark.parametrize("args,named", [
    (["--mate-overlap", "0"], "'0'"),
    (["--mate-overlap", "513"], "'513'"),
    (["--mate-overlap", "x"], "'x'"),
    (["--mate-overlap", "-3"], "'-3'"),
    (["--mate-overlap", ""], "''"),
    (["--mate-overlap", "30", "--mate-overlap-errors", "51"], "'51'"),
    (["--mate-overlap", "30", "--mate-overlap-errors", "-1"], "'-1'"),
    (["--mate-overlap", "30", "--mate-overlap-errors", "ten"], "'ten'"),
], ids=lambda a: " ".join(a)[:60] if isinstance(a, list) else None)
def test_values_that_cannot_be_taken(tmp_path, args, named):
    err = refused(tmp_path, *args, "--interleaved")
    assert named in err and args[-2] in err and "invalid value" in err, err


def test_valid_options_reach_the_database(tmp_path):
    """Accepted: the bounds of O and E, both ways of giving pairs, adapters and trim options on top — the run then goes on to open
    the database and fails there, at the device that is hidden or the directory that is missing (still no output directory)."""
    for args in (["--mate-overlap", "30", "--interleaved"], ["--mate-overlap", "1", "--mate-overlap-errors", "0", "--reads2", FASTQ],
                 ["--mate-overlap=512", "--mate-overlap-errors=50", "--interleaved"],
                 ["--mate-overlap", "30", "--adapter", "illumina", "--adapter2", "nextera", "--trim-quality", "20", "--min-length", "40", "--reads2", FASTQ]):
        out = str(tmp_path / "out")
        p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), *args],
                           capture_output=True, text=True, env=ENV, timeout=60)
        assert p.returncode != 0 and not os.path.exists(out), args
        assert not any(w in p.stderr for w in ("invalid value", "cannot be used", "needs '", "unexpected argument", "a value is required")), (args, p.stderr)
        assert "no HIP device" in p.stderr or "no_such_db" in p.stderr, (args, p.stderr)     # the options passed: the run went on to open the database


def test_usage_lists_the_options():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    for o in ("--mate-overlap <O>", "--mate-overlap-errors <E>", "INSERT_SIZES.tsv", "insert<TAB>fragments", "overlap_fragments", "overlap_skipped",
              "overlap_found", "overlap_readthrough", "overlap_reads", "overlap_bases", "mate_overlap_errors"):
        assert o in text, o
