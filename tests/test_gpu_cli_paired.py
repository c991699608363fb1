"""`phage_filter query --reads2 / --interleaved`: paired-end reads classified as fragments on the examples database.
CLASSIFICATION.csv, the POS/NEG files and READ_SCORES.tsv must equal what the oracle's per-mate query_batch gives once the
mates are combined (union / intersection); --reads2 and --interleaved must agree; replicas and shards must not change them."""
import collections
import gzip
import os
import subprocess

import pytest

from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from test_gpu_scores import Contains

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "examples")
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
TIMEOUT = 300
ENV = dict(os.environ, PFQ_CLI_BATCH_READS="64", PFQ_INGEST_CHUNK_BYTES="20000")
FASTQ = os.path.join(EX, "reads", "sim_reads_c10000_n5_e0.01.fq")


def fastq(path):
    lines = open(path).read().splitlines()
    return [(lines[i][1:].split(" ")[0], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def write(path, recs, fq):
    text = "".join(f"@{h}\n{s}\n+\n{q}\n" if fq else f">{h} desc\n{s}\n" for h, s, q in recs)
    with (gzip.open(path, "wt") if path.endswith(".gz") else open(path, "w")) as f:
        f.write(text)
    return path


def records(path):
    """(header line, sequence) of every record of a POS/NEG file."""
    lines = open(path).read().splitlines()
    if lines and lines[0].startswith("@"):
        return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines), 4)]
    return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines), 2)]


@pytest.fixture(scope="module")
def db(gpu, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("paired_cli") / "db")
    p = subprocess.run([CLI, "build-balanced", "--genomes", os.path.join(EX, "genomes"), "--db-path", d],
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    return d


@pytest.fixture(scope="module")
def pairs():
    """Fragments from the examples' reads: mates from one genome (R2 reverse-complemented), from two genomes, a foreign
    mate, a mate shorter than k, a lowercase mate."""
    recs = fastq(FASTQ)
    out = []
    for i in range(len(recs) // 2):
        (h1, s1, q1), (h2, s2, q2) = recs[2 * i], recs[2 * i + 1]
        if i % 5 == 1:
            s2 = orc.revcomp(s1.encode()).decode()
        elif i % 5 == 2:
            s2 = ("ACGTTGCAAC" * 15)[:len(q2)]
        elif i % 5 == 3:
            s2, q2 = s2[:12], q2[:12]
        elif i % 5 == 4:
            s1 = s1.lower()
        out.append(((f"f{i}/1", s1, q1), (f"f{i}/2", s2, q2)))
    return out


def run(db, out, args, thr, *extra):
    p = subprocess.run([CLI, "query", *args, "--out", out, "--db-path", db, "-b", "16", "-t", "4", "-f", thr, *extra],
                       capture_output=True, text=True, env=ENV, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    return {f: os.path.join(out, f) for f in os.listdir(out)}


def expected(db, pairs, thr, mode):
    ot = fmt.read_db(db)
    reads = [m[1].encode() for p in pairs for m in p]
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    hits, _, _ = orc.query_batch(ot, reads, thr)
    leaves = ot.leaves_dfs()
    col = {v: i for i, v in enumerate(leaves)}
    sets = [set() for _ in reads]
    for r, v in hits:
        sets[r].add(col[v])
    frag = [sets[2 * f] | sets[2 * f + 1] if mode == "either" else sets[2 * f] & sets[2 * f + 1] for f in range(len(pairs))]
    names = [ot.tax_id[v] for v in leaves]
    counts = collections.Counter(c for s in frag for c in s)
    csv = "".join(f"{names[c]},{counts[c]}\n" for c in range(len(names)) if counts[c])
    cont = Contains(ot)
    tsv = ["#read_id\tkmers\tgenome\tmatched_kmers\n"]
    for f, s in enumerate(frag):
        km = [orc.get_kmers(reads[2 * f], ot.kmer_size), orc.get_kmers(reads[2 * f + 1], ot.kmer_size)]
        scored = sorted((-(cont.count(ot.filter_of[leaves[c]], km[0]) + cont.count(ot.filter_of[leaves[c]], km[1])), c) for c in s)
        for neg, c in scored:
            tsv.append(f"{pairs[f][0][0]}\t{len(km[0]) + len(km[1])}\t{names[c]}\t{-neg}\n")
    return frag, names, csv, "".join(tsv)


@pytest.mark.parametrize("kind", ["fq", "fa.gz"])
@pytest.mark.parametrize("thr,mode", [("1.0", "either"), ("0.3", "either"), ("0.3", "both")])
def test_paired_query_equals_oracle(db, pairs, tmp_path, kind, thr, mode):
    fq = kind == "fq"
    r1 = write(str(tmp_path / f"r1.{kind}"), [m1 for m1, _ in pairs], fq)
    r2 = write(str(tmp_path / f"r2.{kind}"), [m2 for _, m2 in pairs], fq)
    il = write(str(tmp_path / f"il.{kind}"), [m for p in pairs for m in p], fq)
    frag, names, csv, tsv = expected(db, pairs, float(thr), mode)
    ext = "fq" if fq else "fa"
    flags = ["--pos-filter", "--neg-filter", "--scores", "--pair-mode", mode]
    a = run(db, str(tmp_path / "a"), ["-r", r1, "--reads2", r2], thr, *flags)
    b = run(db, str(tmp_path / "b"), ["-r", il, "--interleaved"], thr, *flags)
    assert open(a["CLASSIFICATION.csv"]).read() == csv == open(b["CLASSIFICATION.csv"]).read()
    assert open(a["READ_SCORES.tsv"]).read() == tsv == open(b["READ_SCORES.tsv"]).read()
    pos1, pos2 = records(a[f"POS_FILTERING_1.{ext}"]), records(a[f"POS_FILTERING_2.{ext}"])
    neg1, neg2 = records(a[f"NEG_FILTERING_1.{ext}"]), records(a[f"NEG_FILTERING_2.{ext}"])
    assert len(pos1) == len(pos2) and len(neg1) == len(neg2)
    for (x, _), (y, _) in zip(pos1 + neg1, pos2 + neg2):              # mate for mate
        assert x.split(" ")[0][:-2] == y.split(" ")[0][:-2]
    il_pos, il_neg = records(b[f"POS_FILTERING.{ext}"]), records(b[f"NEG_FILTERING.{ext}"])
    assert il_pos == [r for p in zip(pos1, pos2) for r in p] and il_neg == [r for p in zip(neg1, neg2) for r in p]
    want_pos, want_neg = [], []                                       # POS iff the fragment's set is non-empty, both mates
    for f, ((h1, s1, _), (h2, s2, _)) in enumerate(pairs):
        g = ",".join(names[c] for c in sorted(frag[f]))
        if frag[f]:
            want_pos.append(((f"{h1} |{g}", s1.upper()), (f"{h2} |{g}", s2.upper())))
        else:
            want_neg.append(((h1, s1.upper()), (h2, s2.upper())))
    assert list(zip(pos1, pos2)) == want_pos and list(zip(neg1, neg2)) == want_neg
    assert want_pos and (want_neg or thr != "1.0")                  # (below 1 every fragment may find a genome)


@pytest.mark.parametrize("mode", ["either", "both"])
def test_paired_devices_and_shards_agree(db, pairs, tmp_path, mode):
    r1 = write(str(tmp_path / "r1.fq"), [m1 for m1, _ in pairs], True)
    r2 = write(str(tmp_path / "r2.fq"), [m2 for _, m2 in pairs], True)
    flags = ["--pos-filter", "--neg-filter", "--scores", "--pair-mode", mode]
    base = run(db, str(tmp_path / "base"), ["-r", r1, "--reads2", r2], "0.5", *flags)
    for i, extra in enumerate((["--devices", "0,0"], ["--devices", "0,0", "--shard-depth", "1"])):
        got = run(db, str(tmp_path / f"v{i}"), ["-r", r1, "--reads2", r2], "0.5", *flags, *extra)
        assert sorted(got) == sorted(base)
        assert open(got["CLASSIFICATION.csv"], "rb").read() == open(base["CLASSIFICATION.csv"], "rb").read(), extra
        for f in base:   # (fragments are written in input order whatever classified them)
            assert open(got[f], "rb").read() == open(base[f], "rb").read(), (extra, f)
    counts_only = run(db, str(tmp_path / "counts"), ["-r", r1, "--reads2", r2], "0.5", "--pair-mode", mode, "--devices", "0,0")
    assert open(counts_only["CLASSIFICATION.csv"], "rb").read() == open(base["CLASSIFICATION.csv"], "rb").read()
