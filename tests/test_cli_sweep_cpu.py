"""CPU only: the option errors of `phage_filter query --sweep`.  It is refused with the modes that give no whole scored rows of
single reads, with a list that is no strictly ascending list of 1 to 16 numbers, and with a value below -f; every refusal comes
before any device is used (status 101, a message that names the option, no output directory), and the usage text explains the
option and names its two files."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")
# (no device may be touched: one that is asked for does not exist)
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
GOOD = ["--sweep", "0.3,0.5,0.7"]

# (other options, what the message must name beside '--sweep')
REFUSED = [(["--reads2", FASTQ], "'--reads2'"), (["--interleaved"], "'--interleaved'"), (["--shard-depth", "1"], "'--shard-depth'"),
           (["--frame", "500"], "'--frame'"), (["--device-parse"], "'--device-parse'"), (["--pos-filter", "--shard-depth", "2"], "'--shard-depth'")]
# (the list, what the message must say)
BAD_LISTS = [("", "empty item"), ("0.3,,0.5", "empty item"), ("0.3,0.5,", "empty item"), (",0.3", "empty item"), ("0.3,nan", "not a number"),
             ("0.3,abc", "invalid value 'abc'"), ("0.5,0.3", "strictly ascending"), ("0.3,0.3", "strictly ascending"),
             (",".join(f"{0.3 + 0.01 * i:.2f}" for i in range(17)), "at most 16")]


def refused(tmp_path, *args, thr="0.3"):
    out = str(tmp_path / "out")
    p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), "-f", thr, *args],
                       capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101, (args, p.returncode, p.stderr)
    assert not os.path.exists(out), "refused before the output directory is touched"
    return p.stderr


@pytest.mark.parametrize("other,named", REFUSED, ids=[" ".join(o[:1]) for o, _ in REFUSED])
def test_sweep_is_refused_with(tmp_path, other, named):
    for args in ([*other, *GOOD], [*GOOD, *other]):
        err = refused(tmp_path, *args)
        assert "'--sweep'" in err and named in err, err


@pytest.mark.parametrize("spec,says", BAD_LISTS, ids=[s[:24] or "empty" for s, _ in BAD_LISTS])
def test_bad_lists(tmp_path, spec, says):
    for args in (["--sweep", spec, "--pos-filter"], ["--pos-filter", "--sweep", spec]):
        err = refused(tmp_path, *args)
        assert "'--sweep'" in err and says in err, err


@pytest.mark.parametrize("thr,spec", [("0.3", "0.2,0.5"), ("1.0", "0.3,0.5,1.0"), ("nan", "0.3,0.5")])
def test_a_value_below_the_filter_threshold(tmp_path, thr, spec):
    """Also without -f: its default is 1.0."""
    err = refused(tmp_path, "--sweep", spec, thr=thr)
    assert "'--sweep " + spec.split(",")[0] + "'" in err and "'--filter-threshold " + thr + "'" in err and "-f" in err, err
    if thr == "1.0":
        out = str(tmp_path / "out")
        p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), "--sweep", spec],
                           capture_output=True, text=True, env=ENV, timeout=60)
        assert p.returncode == 101 and "'--filter-threshold 1.0'" in p.stderr and not os.path.exists(out), p.stderr


def test_usage_explains_the_option():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    assert "--sweep <T1,T2,..>" in text and "THRESHOLDS.tsv" in text and "THRESHOLD_GENOMES.tsv" in text
    assert "#threshold<TAB>reads<TAB>reads_hit<TAB>\nreads_unique<TAB>assignments<TAB>genomes_hit" in text
    assert "Not with --reads2, --interleaved, --shard-depth,\n--frame or --device-parse" in text
