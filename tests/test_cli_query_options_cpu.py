"""CPU only: what `phage_filter query` answers to its options before any device is used, pinned byte for byte.

Every refusal of `query` (an option that cannot be used with another, one that needs another, a value out of range, a bad list)
is issued before a device is touched and before the output directory is created.  The corpus below runs the binary once per
argument list, with no visible device, and compares exit status, stderr and stdout with tests/golden/cli_query_refusals.json.
Lists that pass every check end in `no HIP device available` or `cannot read no_such_db/tree.bin`: they pin that a legal
combination stays legal.

The fixture was recorded from the binary of the commit BEFORE `cmd_query` was reorganised around `QueryOptions` and the refusal
table, and is not to be recorded again from the code it checks.  A new option adds its cases to the corpus as groups of
their own (its values, its pairs with SINGLES) and their results to the fixture:
`python tests/test_cli_query_options_cpu.py --record <phage_filter>` runs only the groups whose cases the fixture does not hold
and keeps every answer that it holds.  At recording time every case exited with status 101 (one exception: no arguments at all
prints the usage text and exits with 2), none created `out`, two passes were identical and no message held the working
directory's path.  No case of the corpus had to be dropped.

The corpus: (a) nothing, each of 42 option instances, every ordered pair of them; (b) every option that takes a number, with
what it needs beside it, at malformed values and at and around its bounds; (c) the lists of --sweep, --adapter,
--mate-correct-quality, --deplete and --devices; (d) the shapes of a command line; (e) triples whose refusal depends on the
order of the checks."""
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
FIXTURE = os.path.join(ROOT, "tests", "golden", "cli_query_refusals.json")
BASE = ["query", "--reads", "reads.fq", "--out", "out", "--db-path", "no_such_db"]
U32, U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF

# (a) the option instances
SINGLES = [["--pos-filter"], ["--neg-filter"], ["--scores"], ["--reads2", "r2.fq"], ["--interleaved"], ["--pair-mode", "both"], ["--lca", "all"],
           ["--lca", "best"], ["--lca-reads"], ["--abundance"], ["--abundance-iters", "5"], ["--coverage"], ["--coverage-precision", "10"],
           ["--frame", "500"], ["--frame-step", "100"], ["--device-parse"], ["--device-inflate"], ["--device-output"], ["--taxonomy", "tax.tsv"],
           ["--taxon-reads"], ["--best-hits"], ["--sweep", "1.0"], ["--trim-quality", "20"], ["--trim-window", "8"], ["--trim-poly-x", "10"],
           ["--min-length", "30"], ["--max-n", "3"], ["--min-complexity", "30"], ["--adapter", "illumina"], ["--adapter2", "nextera"],
           ["--adapter-overlap", "6"], ["--adapter-errors", "5"], ["--mate-overlap", "30"], ["--mate-overlap-errors", "5"], ["--deplete", "screen"],
           ["--deplete-threshold", "0.7"], ["--mate-correct"], ["--mate-correct-quality", "30,10"], ["--shard-depth", "1"], ["--search-depth", "2"],
           ["--devices", "0"], ["--block-size-reads", "0"]]
# the options that turn preprocessing on, in the order in which a refusal looks for the first one given
PREP = [s for s in SINGLES if s[0] in ("--trim-quality", "--trim-window", "--trim-poly-x", "--min-length", "--max-n", "--min-complexity", "--adapter",
                                        "--adapter2", "--adapter-overlap", "--adapter-errors", "--mate-overlap", "--mate-overlap-errors")]
MATES = ["--interleaved", "--mate-overlap", "30"]
# (b) option, what it needs beside it, lower and upper bound (None: a real number, no bounds)
NUMBERS = [("threads", [], 0, U64), ("cache-size", [], 0, U64), ("block-size-reads", [], 0, U64), ("search-depth", [], 0, U64),
           ("shard-depth", [], 0, U64), ("devices", [], 0, U64), ("abundance-iters", ["--abundance"], 1, U32),
           ("filter-threshold", [], None, None), ("deplete-threshold", ["--deplete", "screen"], None, None),
           ("coverage-precision", ["--coverage"], 4, 16), ("frame", [], 1, U32), ("frame-step", ["--frame", "500"], 1, U32),
           ("trim-quality", [], 0, 93), ("trim-window", [], 1, 1024), ("trim-poly-x", [], 0, U32), ("min-length", [], 1, U32), ("max-n", [], 0, U32 - 1),
           ("min-complexity", [], 0, 100), ("adapter-overlap", ["--adapter", "illumina"], 1, 64), ("adapter-errors", ["--adapter", "illumina"], 0, 50),
           ("mate-overlap", ["--interleaved"], 1, 512), ("mate-overlap-errors", MATES, 0, 50),
           ("mate-correct-quality", [*MATES, "--mate-correct"], 1, 93)]
MALFORMED = ["", "x", "-1", "+1", " 1", "1 ", "1x", "0x10"]
# (c) the lists of tests/test_cli_sweep_cpu.py
SWEEP_LISTS = ["0.3,0.5,0.7", "", "0.3,,0.5", "0.3,0.5,", ",0.3", "0.3,nan", "0.3,abc", "0.5,0.3", "0.3,0.3",
               ",".join(f"{0.3 + 0.01 * i:.2f}" for i in range(17)), ",".join(f"{0.3 + 0.01 * i:.2f}" for i in range(16))]
SWEEP_BELOW = [("0.3", "0.2,0.5"), ("1.0", "0.3,0.5,1.0"), ("nan", "0.3,0.5"), ("0.5", "0.5,0.4"), ("0.5", "0.6,0.4")]


def values_of(lo, hi):
    v = list(MALFORMED)
    if lo is not None:
        v += [str(lo - 1), str(lo), str(hi), str(hi + 1)]
    v.append("18446744073709551616")
    return list(dict.fromkeys(v))


def corpus():
    """The groups of argument lists (behind BASE, unless a list starts with None: then it is the whole command line), in a fixed order."""
    groups = {"singles": [[]] + SINGLES}
    for a in SINGLES:
        groups["pairs " + " ".join(a)] = [a + b for b in SINGLES]  # (with itself too: the option given twice)
    for name, needs, lo, hi in NUMBERS:
        groups["values --" + name] = [c for v in values_of(lo, hi) for c in ([[*needs, "--" + name, v], ["--" + name, v, *needs]] if needs else [["--" + name, v]])]
    sweep = [c for s in SWEEP_LISTS for c in (["-f", "0.3", "--sweep", s, "--pos-filter"], ["--pos-filter", "-f", "0.3", "--sweep", s])]
    sweep += [["-f", thr, "--sweep", s] for thr, s in SWEEP_BELOW] + [["--sweep", "0.3,0.5,1.0"], ["--sweep", "1.0,1.5"]]
    acgt = "ACGTTGCA"
    adapters = ["illumina", "nextera", "smallrna", "Illumina", "acgtacgt", "ACGNACGT", "ACGT", "ACGT,illumina", "illumina,", ",illumina", "",
                acgt * 8, acgt * 8 + "A", ",".join([acgt] * 8), ",".join([acgt] * 9)]
    lists = [["--adapter", s] for s in adapters] + [["--interleaved", "--adapter", "illumina", "--adapter2", s] for s in adapters]
    lists += [["--adapter", "ACGTACG", "--adapter-overlap", "8"], ["--adapter", "ACGTACGT", "--adapter-overlap", "8"],
              ["--adapter", "illumina", "--adapter-overlap", "14"], ["--adapter", acgt] * 5, ["--adapter", acgt, "--adapter2", acgt],
              ["--reads2", "r2.fq", "--adapter", acgt, "--adapter2", "nextera", "--adapter2", acgt]]
    lists += [[*MATES, "--mate-correct", "--mate-correct-quality", v] for v in ("30", "30,30", "0,0", "94,1", "30,", ",10", "30,10,5", "93,92", "1,0", "30,-1")]
    lists += [["--deplete", "screen"] * n for n in (2, 4, 5)] + [["--deplete", "nodir"], ["--deplete", "screen", "--deplete", "nodir"],
                                                                   ["--deplete", "screen,screen"], ["--deplete", "screen,"], ["--deplete", ""]]
    lists += [["--devices", v] for v in ("0,,1", "x", "all", "0,1", "0,x", ",", "")]
    groups["lists --sweep"] = sweep
    groups["lists"] = lists
    groups["shapes"] = [[None], [None, "query"], *[[None, *BASE[:k], *BASE[k + 2:]] for k in (1, 3, 5)],
                        ["--bogus"], ["-Z"], ["--bogus=1"], ["stray"], ["--reads"], ["-f"], ["--filter-threshold=0.5"], ["-f0.5"], ["-f=0.5"],
                        ["--filter-threshold=0.5", "--sweep", "0.4"], ["-f0.5", "--sweep", "0.4"], ["-f=0.5", "--sweep", "0.4"], ["-t4", "-b", "7", "-c=3"],
                        ["-vq", "--verbose", "--quiet"], ["--format", "bogus"], ["-F", "fasta"], ["--pair-mode", "bogus", "--interleaved"],
                        ["--pair-mode", "bogus"], ["--lca", "bogus"], ["--lca=best", "--lca-reads"]]
    triples = []
    for third in PREP + [["--deplete", "screen"], ["--deplete-threshold", "0.7"], ["--mate-correct"], ["--mate-correct-quality", "30,10"]]:
        triples += [["--device-output", "--neg-filter", *third], [*third, "--neg-filter", "--device-output"]]
    for a, b in list(zip(PREP, PREP[1:])) + [(a, ["--deplete", "screen"]) for a in PREP]:  # which preprocessing option a refusal names
        for first, second in ((a, b), (b, a)):
            triples += [[*first, *second, *x] for x in (["--device-parse"], ["--device-output"], ["--frame", "500"], ["--shard-depth", "1"])]
    for third in (["--shard-depth", "1"], ["--device-parse"], ["--frame", "500"]):
        triples += [["--best-hits", "--abundance", *third], [*third, "--abundance", "--best-hits"]]
    triples += [["--mate-correct", *m, *x] for m in ([], ["--mate-overlap", "30"], MATES) for x in ([], ["--device-parse"], ["--device-output", "--pos-filter"])]
    groups["triples"] = triples
    return groups


CORPUS = corpus()
ENV = {k: v for k, v in os.environ.items() if not k.startswith("PFQ_")}
ENV.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # (no device may be touched: one that is asked for does not exist)


def digest(cases):
    return hashlib.sha256(json.dumps(cases).encode()).hexdigest()[:16]


def run_group(cli, cwd, cases):
    """[(status, stderr, stdout)] of the cases, run in `cwd`, which holds an empty screen/tree.bin and nothing else."""
    os.makedirs(os.path.join(cwd, "screen"), exist_ok=True)
    open(os.path.join(cwd, "screen", "tree.bin"), "wb").close()

    def one(case):
        argv = case[1:] if case and case[0] is None else BASE + case
        p = subprocess.run([cli, *argv], cwd=cwd, env=ENV, capture_output=True, timeout=60)
        assert not os.path.exists(os.path.join(cwd, "out")), (argv, "refused before the output directory is touched")
        return p.returncode, p.stderr.decode("utf-8", "surrogateescape"), p.stdout.decode("utf-8", "surrogateescape")

    with ThreadPoolExecutor(4) as pool:
        return list(pool.map(one, cases))


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_corpus_is_the_fixtures(recorded):
    assert list(recorded["groups"]) == list(CORPUS)
    assert sum(len(c) for c in CORPUS.values()) == sum(len(g["status"]) for g in recorded["groups"].values()) == recorded["cases"]
    assert len(SINGLES) == 42 and len(CORPUS["singles"]) + sum(len(c) for n, c in CORPUS.items() if n.startswith("pairs ")) == 1 + 42 + 42 * 42


@pytest.mark.parametrize("group", list(CORPUS))
def test_every_answer_is_the_recorded_one(tmp_path, recorded, group):
    cases, want = CORPUS[group], recorded["groups"][group]
    assert len(cases) == len(want["status"]) == len(want["stderr"]) == len(want["stdout"]) and digest(cases) == want["digest"], "corpus and fixture drifted apart"
    text = recorded["texts"]
    for case, (status, err, out), w_status, w_err, w_out in zip(cases, run_group(CLI, str(tmp_path), cases), want["status"], want["stderr"], want["stdout"]):
        assert (status, err, out) == (w_status, text[w_err], text[w_out]), case


def record(cli):
    """Adds to the fixture the groups it does not hold; a group it holds, with the same cases, keeps its recorded answers."""
    import tempfile
    old = json.load(open(FIXTURE))
    texts = list(old["texts"])
    index = {t: i for i, t in enumerate(texts)}
    groups = {}
    for name, cases in CORPUS.items():
        if old["groups"].get(name, {}).get("digest") == digest(cases):
            groups[name] = old["groups"][name]
            continue
        passes = []
        for _ in range(2):
            with tempfile.TemporaryDirectory() as cwd:
                passes.append(run_group(cli, cwd, cases))
                for case, (status, err, out) in zip(cases, passes[-1]):
                    assert cwd not in err + out and os.path.basename(cwd) not in err + out, (case, "a message holds the working directory")
                    assert status == 101 or case == [None], (case, status, err)
        assert passes[0] == passes[1], "two passes differ"
        for t in (t for res in passes[0] for t in res[1:]):
            if t not in index:
                index[t] = len(texts)
                texts.append(t)
        groups[name] = {"digest": digest(cases), "status": [r[0] for r in passes[0]], "stderr": [index[r[1]] for r in passes[0]],
                        "stdout": [index[r[2]] for r in passes[0]]}
    with open(FIXTURE, "w") as f:
        json.dump({"cases": sum(len(g["status"]) for g in groups.values()), "texts": texts, "groups": groups}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{sum(len(g['status']) for g in groups.values())} cases, {len(texts)} texts, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    record(os.path.abspath(sys.argv[2]))
