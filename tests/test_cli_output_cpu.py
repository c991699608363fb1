"""CPU only: `phage_filter query --device-output` serves POS / NEG filtering of single reads and nothing else.  Without a filter
option, with every other mode `--device-parse` refuses, with `--device-parse` itself, with the preprocessing options and with a
block size the device cannot decide, it is refused before any device is used (status 101, a message that names both options, no
output directory), and the usage text lists the option."""
import subprocess

import pytest

from test_cli_text_cpu import CLI, ENV, FASTQ, refused

REFUSED = [["--scores"], ["--lca", "best"], ["--lca", "all", "--lca-reads"], ["--reads2", FASTQ], ["--interleaved"], ["--abundance"], ["--coverage"],
           ["--frame", "500"], ["--shard-depth", "1"], ["--device-parse"], ["--trim-quality", "20"], ["--trim-window", "4"], ["--trim-poly-x", "10"],
           ["--min-length", "30"], ["--max-n", "3"], ["--min-complexity", "30"], ["--sweep", "1.0"], ["--taxonomy", FASTQ]]


@pytest.mark.parametrize("other", REFUSED, ids=[" ".join(o[:2]) if o[0] == "--lca" else o[0] for o in REFUSED])
def test_device_output_refuses_the_other_modes(tmp_path, other):
    named = "'--lca best'" if other[:2] == ["--lca", "best"] else f"'{other[-1] if other[0] == '--lca' else other[0]}'"
    for args in ([*other, "--pos-filter", "--neg-filter", "--device-output"], ["--device-output", "--pos-filter", *other]):
        err = refused(tmp_path, *args)
        assert "'--device-output'" in err and named in err, err


def test_needs_a_filter_option(tmp_path):
    err = refused(tmp_path, "--device-output")
    assert "'--device-output'" in err and "'--pos-filter'" in err and "'--neg-filter'" in err, err


@pytest.mark.parametrize("block,named", [("0", "'--block-size-reads 0'"), ("8193", "'--block-size-reads 8193'")])
def test_block_sizes_the_device_cannot_decide(tmp_path, block, named):
    err = refused(tmp_path, "--pos-filter", "--device-output", "-b", block)
    assert "'--device-output'" in err and named in err, err
    if block == "8193":
        assert "8192" in err                                           # the message says the limit


def test_usage_lists_the_option():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    assert "--device-output" in text and "formatted on the GPU" in text
