"""CPU only: the option errors of `phage_filter query --best-hits`.  It needs one of the outputs it changes and is refused
with the modes that give no whole scored rows; every refusal comes before any device is used (status 101, a message that names
the option, no output directory), and the usage text explains the option."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")
# (no device may be touched: one that is asked for does not exist)
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")

# (other options, what the message must name beside '--best-hits')
NEEDS = [([], "'--taxonomy <FILE>', '--abundance', '--coverage'"), (["--scores"], "'--abundance'"), (["--lca", "best", "--lca-reads"], "'--coverage'"),
         (["--pos-filter", "--neg-filter"], "'--taxonomy <FILE>'")]
REFUSED = [(["--coverage", "--shard-depth", "1"], "'--shard-depth'"), (["--abundance", "--shard-depth", "2"], "'--shard-depth'"),
           (["--taxonomy", "no_such_file.tsv", "--shard-depth", "1"], "'--shard-depth'"),
           (["--abundance", "--device-parse"], "'--device-parse'"), (["--coverage", "--device-parse"], "'--device-parse'"),
           (["--taxonomy", "no_such_file.tsv", "--device-parse"], "'--device-parse'"),
           (["--coverage", "--frame", "500"], "'--frame'"), (["--abundance", "--frame", "500", "--frame-step", "100"], "'--frame'"),
           (["--taxonomy", "no_such_file.tsv", "--frame", "500"], "'--frame'")]


def refused(tmp_path, *args):
    out = str(tmp_path / "out")
    p = subprocess.run([CLI, "query", "--reads", FASTQ, "--out", out, "--db-path", str(tmp_path / "no_such_db"), "-f", "0.7", *args],
                       capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101, (args, p.returncode, p.stderr)
    assert not os.path.exists(out), "refused before the output directory is touched"
    return p.stderr


@pytest.mark.parametrize("other,named", NEEDS + REFUSED, ids=[" ".join(o) or "alone" for o, _ in NEEDS + REFUSED])
def test_best_hits_option_errors(tmp_path, other, named):
    for args in ([*other, "--best-hits"], ["--best-hits", *other]):
        err = refused(tmp_path, *args)
        assert "'--best-hits'" in err and named in err, err


def test_usage_explains_the_option():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    assert "--best-hits" in text and "best-scoring" in text and "TAXON_COUNTS.tsv, READ_TAXA.tsv, ABUNDANCE.tsv" in text
    assert "Not with --shard-depth, --frame or\n--device-parse" in text
