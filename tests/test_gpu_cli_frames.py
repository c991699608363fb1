"""`phage_filter query --frame`: SEGMENTS.tsv and CLASSIFICATION.csv against tests/frames_ref.py over the oracle, on the database
the CLI's own `build` makes of the example genomes.  The input is a FASTA of multi-line contigs, each two stretches of example
genomes joined by random sequence.  The files must not depend on the device list, -t or the batch size."""
import os
import subprocess

import numpy as np
import pytest

import frames_ref as fr
from oracle import pfq_format as fmt
from test_gpu_cli_lca import CLI, EX, SEEDS, TIMEOUT, query

pytestmark = pytest.mark.gpu

HEADER = "sequence\tgenome\tbegin\tend\tmatch_begin\tmatch_end\tframes\tkmers\tmatched\tlongest_run\n"


def read_fasta(path):
    return b"".join(l.strip() for l in open(path, "rb") if not l.startswith(b">"))


@pytest.fixture(scope="module")
def examples(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frames_cli")
    db = str(tmp / "db")
    p = subprocess.run([CLI, "build", "--genomes", os.path.join(EX, "genomes"), "--db-path", db, "--seed1", str(SEEDS[0]),
                        "--seed2", str(SEEDS[1])], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    ot = fmt.read_db(db)
    gdir = os.path.join(EX, "genomes")
    genomes = [read_fasta(os.path.join(gdir, f)) for f in sorted(os.listdir(gdir))]
    rng = np.random.default_rng(99)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    contigs = []
    for i in range(10):
        a, b = genomes[i % len(genomes)], genomes[(3 * i + 1) % len(genomes)]
        oa, ob = int(rng.integers(0, len(a) - 1500)), int(rng.integers(0, len(b) - 1200))
        gap = acgt[rng.integers(0, 4, 700 + 13 * i)].tobytes()
        contigs.append((f"contig{i}", a[oa:oa + 1500] + gap + b[ob:ob + 1200] + gap[:200 + i]))
    contigs.append(("empty_of_genomes", acgt[rng.integers(0, 4, 900)].tobytes()))
    fasta = str(tmp / "contigs.fa")
    with open(fasta, "wb") as f:
        for name, s in contigs:
            f.write(b">" + name.encode() + b" assembled\n" + b"".join(s[j:j + 70] + b"\n" for j in range(0, len(s), 70)))
    return db, ot, [ot.tax_id[v] for v in ot.leaves_dfs()], contigs, fasta


def reference_text(ot, names, contigs, F, S, thr):
    per, _, counts, _ = fr.Ref(ot).query([s for _, s in contigs], F, S, thr)
    lines = [HEADER]
    for (name, _), segs in zip(contigs, per):
        for s in segs:
            lines.append(f"{name}\t{names[s['leaf']]}\t{s['begin']}\t{s['end']}\t{s['match_begin']}\t{s['match_end']}\t{s['n_frames']}\t"
                         f"{s['kmers']}\t{s['matched']}\t{s['longest_run']}\n")
    csv = "".join(f"{n},{c}\n" for n, c in zip(names, counts) if c)
    return "".join(lines).encode(), csv.encode(), per


@pytest.mark.parametrize("thr", ["1.0", "0.6"])
def test_segments_and_counts(examples, tmp_path, thr):
    db, ot, names, contigs, fasta = examples
    tsv, csv, per = reference_text(ot, names, contigs, 500, 250, float(thr))
    assert sum(1 for segs in per if segs) >= 8 and not per[-1] and any(len({s["leaf"] for s in segs}) >= 2 for segs in per)
    _, got = query(db, str(tmp_path / "a"), "--reads", fasta, "--frame", "500", thr=thr)        # (the default step is F / 2)
    assert sorted(got) == ["CLASSIFICATION.csv", "SEGMENTS.tsv"]
    assert got["SEGMENTS.tsv"] == tsv and got["CLASSIFICATION.csv"] == csv
    for i, extra in enumerate((["--devices", "0"], ["--devices", "0,0"], ["--devices", "0,0,0"])):
        for threads in ("1", "4"):
            _, other = query(db, str(tmp_path / f"d{i}{threads}"), "--reads", fasta, "--frame", "500", "--frame-step", "250", *extra, thr=thr,
                             threads=threads, block="3")
            assert other == got, (extra, threads)
    env = dict(os.environ, PFQ_CLI_BATCH_READS="1")
    out = str(tmp_path / "tiny")
    p = subprocess.run([CLI, "query", "--out", out, "--db-path", db, "--block-size-reads", "1", "--filter-threshold", thr, "--reads", fasta,
                        "--frame", "500", "--frame-step", "250"], capture_output=True, text=True, env=env, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    assert {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))} == got


def test_other_frames(examples, tmp_path):
    db, ot, names, contigs, fasta = examples
    tsv, csv, _ = reference_text(ot, names, contigs, 333, 111, 1.0)
    _, got = query(db, str(tmp_path / "a"), "--reads", fasta, "--frame", "333", "--frame-step", "111", "--devices", "0,0")
    assert got["SEGMENTS.tsv"] == tsv and got["CLASSIFICATION.csv"] == csv


def test_frame_shorter_than_k(examples, tmp_path):
    db, ot, _, _, fasta = examples
    assert ot.kmer_size > 5
    p = subprocess.run([CLI, "query", "--out", str(tmp_path / "o"), "--db-path", db, "--reads", fasta, "--frame", "5"], capture_output=True, text=True,
                       timeout=TIMEOUT)
    assert p.returncode == 101 and f"k = {ot.kmer_size}" in p.stderr and "'--frame 5'" in p.stderr, p.stderr
