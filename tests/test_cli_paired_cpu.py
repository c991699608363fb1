"""CPU only: paired-end input of `phage_filter ingest-check` / `query` (`--reads2`, `--interleaved`).  The fragments come out
as `query` pairs them, mates adjacent; mate ids must agree once a trailing /1 and /2 are stripped; a mismatch, one stream
ending first or an odd interleaved input is fatal (status 101) after the fragments before it; the options are checked before
any device is used."""
import gzip
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FASTQ = os.path.join(ROOT, "tests", "golden", "examples", "reads", "sim_reads_c10000_n5_e0.01.fq")
ENV = dict(os.environ, PFQ_INGEST_CHUNK_BYTES="3000")


def fastq(path):
    lines = open(path).read().splitlines()
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def write(path, recs, fq=True):
    text = "".join(f"@{h}\n{s}\n+\n{q}\n" if fq else f">{h}\n{s}\n" for h, s, q in recs)
    if path.endswith(".gz"):
        with gzip.open(path, "wt") as f:
            f.write(text)
    else:
        open(path, "w").write(text)
    return path


@pytest.fixture(scope="module")
def pairs():
    recs = fastq(FASTQ)
    return [((f"frag{i}/1", recs[2 * i][1], recs[2 * i][2]), (f"frag{i}/2 run=7", recs[2 * i + 1][1], recs[2 * i + 1][2]))
            for i in range(len(recs) // 2)]


def check(*args, rc=0):
    p = subprocess.run([CLI, "ingest-check", "--dump", *args], capture_output=True, text=True, env=ENV, timeout=120)
    assert p.returncode == rc, p.stderr
    return p.stdout.splitlines()[:-1], p.stderr


def expected(pairs, fq=True):
    out = []
    for m1, m2 in pairs:
        for h, s, q in (m1, m2):
            out.append(f"{'@' if fq else '>'}{h.split(' ')[0]}\x01{s}\x01{q if fq else ''}")
    return out


@pytest.mark.parametrize("threads,block", [("1", "1000"), ("4", "3"), ("8", "7")])
def test_reads2_and_interleaved_give_the_fragments(pairs, tmp_path, threads, block):
    r1 = write(str(tmp_path / "r1.fq"), [m1 for m1, _ in pairs])
    r2 = write(str(tmp_path / "r2.fq.gz"), [m2 for _, m2 in pairs])
    il = write(str(tmp_path / "il.fq"), [m for p in pairs for m in p])
    want = expected(pairs)
    a, _ = check("-r", r1, "--reads2", r2, "-t", threads, "-b", block)
    b, _ = check("-r", il, "--interleaved", "-t", threads, "-b", block)
    assert a == want and b == want


def test_fasta_pairs_from_directories(pairs, tmp_path):
    d1, d2 = tmp_path / "R1", tmp_path / "R2"
    d1.mkdir()
    d2.mkdir()
    half = len(pairs) // 2                                          # two files per side, consumed in the same order
    write(str(d1 / "a.fa"), [m1 for m1, _ in pairs[:half]], fq=False)
    write(str(d1 / "b.fa"), [m1 for m1, _ in pairs[half:]], fq=False)
    write(str(d2 / "a.fa"), [m2 for _, m2 in pairs[:half]], fq=False)
    write(str(d2 / "b.fa"), [m2 for _, m2 in pairs[half:]], fq=False)
    got, _ = check("-r", str(d1), "--reads2", str(d2), "-t", "4")
    assert sorted(got) == sorted(expected(pairs, fq=False)) and len(got) == 2 * len(pairs)
    assert all(x.split("\x01")[0][:-2] == y.split("\x01")[0][:-2] for x, y in zip(got[::2], got[1::2]))


def test_ids_without_mate_suffix_pair_up(pairs, tmp_path):
    strip = [((h[:-2], s, q), (h2.split(" ")[0][:-2], s2, q2)) for (h, s, q), (h2, s2, q2) in pairs[:50]]
    r1 = write(str(tmp_path / "r1.fq"), [m1 for m1, _ in strip])
    r2 = write(str(tmp_path / "r2.fq"), [m2 for _, m2 in strip])
    got, _ = check("-r", r1, "--reads2", r2)
    assert got == expected(strip)


@pytest.mark.parametrize("where", [0, 37])
def test_id_mismatch_is_fatal_after_the_fragments_before_it(pairs, tmp_path, where):
    bad = list(pairs)
    (h, s, q) = bad[where][1]
    bad[where] = (bad[where][0], ("other" + h, s, q))
    r1 = write(str(tmp_path / "r1.fq"), [m1 for m1, _ in bad])
    r2 = write(str(tmp_path / "r2.fq"), [m2 for _, m2 in bad])
    got, err = check("-r", r1, "--reads2", r2, "-b", "5", rc=101)
    assert got == expected(pairs[:where]) and "differ" in err
    il = write(str(tmp_path / "il.fq"), [m for p in bad for m in p])
    got, err = check("-r", il, "--interleaved", "-b", "5", rc=101)
    assert got == expected(pairs[:where]) and "differ" in err


@pytest.mark.parametrize("short", ["r1", "r2"])
def test_one_stream_ending_first_is_fatal(pairs, tmp_path, short):
    n = 41
    m1s = [m1 for m1, _ in pairs][:n] if short == "r1" else [m1 for m1, _ in pairs]
    m2s = [m2 for _, m2 in pairs][:n] if short == "r2" else [m2 for _, m2 in pairs]
    r1 = write(str(tmp_path / "r1.fq"), m1s)
    r2 = write(str(tmp_path / "r2.fq"), m2s)
    for block in ("1000", "41", "6"):
        got, err = check("-r", r1, "--reads2", r2, "-b", block, rc=101)
        assert got == expected(pairs[:n]) and "ends after" in err, block


def test_odd_interleaved_input_is_fatal(pairs, tmp_path):
    il = write(str(tmp_path / "il.fq"), [m for p in pairs[:20] for m in p] + [pairs[20][0]])
    got, err = check("-r", il, "--interleaved", rc=101)
    assert got == expected(pairs[:20]) and "odd number" in err


def test_argument_errors(pairs, tmp_path):
    r1 = write(str(tmp_path / "r1.fq"), [m1 for m1, _ in pairs[:4]])
    r2 = write(str(tmp_path / "r2.fq"), [m2 for _, m2 in pairs[:4]])
    _, err = check("-r", r1, "--reads2", r2, "--interleaved", rc=101)
    assert "cannot be used with" in err
    _, err = check("-r", r1, "--reads2", r2, "--count", rc=101)
    assert "--count" in err
    base = [CLI, "query", "-r", r1, "-o", str(tmp_path / "out"), "-d", str(tmp_path / "no_db")]
    for extra, msg in ((["--reads2", r2, "--interleaved"], "cannot be used with"), (["--pair-mode", "both"], "needs"),
                       (["--reads2", r2, "--pair-mode", "all"], "possible values"), (["--reads2"], "value is required")):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 101 and msg in p.stderr, (extra, p.stderr)


def test_usage_lists_paired_options():
    p = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert "--reads2" in p.stderr and "--interleaved" in p.stderr and "--pair-mode" in p.stderr
