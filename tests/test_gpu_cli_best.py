"""`phage_filter query --best-hits`: TAXON_COUNTS.tsv, READ_TAXA.tsv, ABUNDANCE.tsv and COVERAGE.tsv must equal the text built
here from the references over every read's best-scoring genomes (oracle rows, expected_scores / pair_scores, best_sets), and
every other output must be byte-identical to the run without the option.  The database is the CLI's own `build` of workload W's
genomes (tests/test_gpu_lca.py): nested families, on which the reduction is known to bite — the twelve unrelated example phages
would leave it nothing to do."""
import os
import subprocess

import pytest

import cover_ref
import tax_ref
from oracle import pfq_format as fmt
from test_gpu_cli_abund import check_tsv as check_abundance_tsv
from test_gpu_cli_cover import check_tsv as check_coverage_tsv
from test_gpu_cli_lca import CLI, SEEDS, TIMEOUT, query, write_fasta
from test_gpu_cli_tax import counts_tsv, reads_tsv
from test_gpu_lca import K, W, best_sets, csr_of, oracle_sets, pair_scores
from test_gpu_paired import combine, mate_sets
from test_gpu_scores import Contains, expected_scores
from test_gpu_tax import random_taxonomy

pytestmark = pytest.mark.gpu

THR = "0.7"
CHANGED = ("TAXON_COUNTS.tsv", "READ_TAXA.tsv", "ABUNDANCE.tsv", "COVERAGE.tsv")


def lineage_file(names, tax):
    """random_taxonomy's (taxon_parent, taxon_names, leaf_taxon) as a taxonomy file: one line per genome, its taxon's path."""
    parent, tnames, leaf_taxon = tax
    def path(t):
        out = []
        while t > 0:
            out.append(tnames[t])
            t = parent[t]
        return ";".join(reversed(out))
    return "".join(f"{g}\t{path(leaf_taxon[l])}\n" for l, g in enumerate(names)).encode()


@pytest.fixture(scope="module")
def wdb(gpu, tmp_path_factory):
    """W's genomes as FASTA files, built by the CLI; its reads as FASTQ (the empty read left out: a record needs a sequence);
    the database read back for the oracle; a taxonomy file over its genomes; the unpaired expectations, computed once."""
    base = tmp_path_factory.mktemp("best_cli")
    w = W(device=False)
    gdir = base / "genomes"
    gdir.mkdir()
    for i, g in zip(w.ids, w.genomes):
        write_fasta(gdir / f"{i}.fa", [(i, g)])
    db = str(base / "db")
    p = subprocess.run([CLI, "build", "--genomes", str(gdir), "--db-path", db, "--kmer-size", str(K), "--false-pos-rate", "0.001",
                        "--largest-genome", "3000", "--seed1", str(SEEDS[0]), "--seed2", str(SEEDS[1])], capture_output=True, text=True,
                       timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    ot = fmt.read_db(db)
    names = [ot.tax_id[v] for v in ot.leaves_dfs()]
    assert sorted(names) == sorted(w.ids)
    recs = [(f"r{i}", r) for i, r in enumerate(w.reads) if r]
    fastq = base / "reads.fq"
    fastq.write_bytes(b"".join(b"@" + rid.encode() + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for rid, s in recs))
    data = lineage_file(names, random_taxonomy(101, len(names)))
    tax = base / "taxonomy.tsv"
    tax.write_bytes(data)
    parent, tnames, leaf_taxon, _ = tax_ref.parse(data, names)
    x = dict(db=db, ot=ot, names=names, recs=recs, fastq=str(fastq), tax=str(tax), ref=tax_ref.Nodes(names, parent, tnames, leaf_taxon),
             contains=Contains(ot), cache=cover_ref.TreeSketcher(ot), w=w)
    reads = [s for _, s in recs]
    sets = oracle_sets(ot, reads, float(THR))
    offs, leaves = csr_of(sets)
    best = best_sets(sets, expected_scores(ot, reads, offs, leaves, x["contains"]))
    n_hit = sum(1 for s in sets if s)
    differ = sum(1 for s, b in zip(sets, best) if s != b)
    print(f"theta {THR}: hit {n_hit}, best rows differ from the whole rows for {differ}")
    assert differ >= 0.1 * n_hit
    x.update(sets=sets, best=best, sketch=cover_ref.TreeSketcher(ot, share=x["cache"]).add_reads([sorted(b) for b in best], reads))
    return x


def options(x):
    return ["--pos-filter", "--neg-filter", "--scores", "--lca", "best", "--lca-reads", "--taxonomy", x["tax"], "--taxon-reads", "--abundance",
            "--coverage"]


def check_changed(x, got, ids, sets, best, sketch):
    """The four outputs the option changes, popped from `got`, against the references over `best`; `sets`: the whole rows."""
    est = check_abundance_tsv(got.pop("ABUNDANCE.tsv"), best, x["names"])
    assert est["n_ambiguous"] > 0 and est["n_unique"] > 0
    want_counts, last, _ = counts_tsv(x["ref"], best, est["mass"])
    assert got.pop("TAXON_COUNTS.tsv") == want_counts
    assert got.pop("READ_TAXA.tsv") == reads_tsv(x["ref"], ids, sets, last)   # (hits: the size of the whole hit set)
    check_coverage_tsv(got.pop("COVERAGE.tsv"), sketch, x["names"])


def test_unpaired_against_the_references_and_the_plain_run(wdb, tmp_path):
    x = wdb
    src = ["--reads", x["fastq"], *options(x)]
    out0, plain = query(x["db"], str(tmp_path / "p"), *src, thr=THR)
    out1, got = query(x["db"], str(tmp_path / "b"), *src, "--best-hits", thr=THR)
    assert sorted(got) == sorted(plain) and len(plain) == 10, sorted(plain)
    whole = {f: plain.pop(f) for f in CHANGED}
    assert all(got[f] != whole[f] for f in CHANGED)                    # the option does something here
    check_changed(x, got, [rid for rid, _ in x["recs"]], x["sets"], x["best"], x["sketch"])
    assert got == plain and out1 == out0                               # CLASSIFICATION.csv, POS / NEG, READ_SCORES, CLADE_COUNTS, READ_LCA
    # --lca all beside it, and no other per-read output at all
    lean = ["--reads", x["fastq"], "--lca", "all", "--taxonomy", x["tax"], "--abundance", "--coverage"]
    _, plain = query(x["db"], str(tmp_path / "q"), *lean, thr=THR)
    _, got = query(x["db"], str(tmp_path / "c"), *lean, "--best-hits", thr=THR)
    got["READ_TAXA.tsv"] = reads_tsv(x["ref"], [rid for rid, _ in x["recs"]], x["sets"], x["ref"].counts(x["best"])[0])   # (not asked for)
    check_changed(x, got, [rid for rid, _ in x["recs"]], x["sets"], x["best"], x["sketch"])
    for f in CHANGED:
        plain.pop(f, None)
    assert got == plain and sorted(plain) == ["CLADE_COUNTS.tsv", "CLASSIFICATION.csv"]


def test_two_replicas_on_one_device(wdb, tmp_path):
    x = wdb
    src = ["--reads", x["fastq"], *options(x)]
    _, plain = query(x["db"], str(tmp_path / "p"), *src, "--devices", "0,0", thr=THR, threads="3", block="17")
    _, got = query(x["db"], str(tmp_path / "d"), *src, "--best-hits", "--devices", "0,0", thr=THR, threads="3", block="17")
    check_changed(x, got, [rid for rid, _ in x["recs"]], x["sets"], x["best"], x["sketch"])
    for f in CHANGED:
        plain.pop(f)
    assert got == plain


def test_reads2_takes_the_fragments_best_rows(wdb, tmp_path):
    x = wdb
    ot, w = x["ot"], x["w"]
    pairs = [p for p in w.pairs() if p[0] and p[1]]
    preads = [m for p in pairs for m in p]
    r1 = write_fasta(tmp_path / "r1.fa", [(f"f{i}/1", p[0]) for i, p in enumerate(pairs)])
    r2 = write_fasta(tmp_path / "r2.fa", [(f"f{i}/2", p[1]) for i, p in enumerate(pairs)])
    frag = combine(mate_sets(ot, preads, float(THR)), "either")
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    best = best_sets(frag, pair_scores(ot, preads, frag, x["contains"]))
    assert sum(1 for s, b in zip(frag, best) if s != b) >= 0.1 * sum(1 for s in frag if s)
    sketch = cover_ref.TreeSketcher(ot, share=x["cache"]).add_pairs([sorted(b) for b in best], pairs)
    src = ["--reads", r1, "--reads2", r2, "--pair-mode", "either", *options(x)]
    _, plain = query(x["db"], str(tmp_path / "p"), *src, thr=THR)
    _, got = query(x["db"], str(tmp_path / "b"), *src, "--best-hits", thr=THR)
    check_changed(x, got, [f"f{i}/1" for i in range(len(pairs))], frag, best, sketch)
    for f in CHANGED:
        plain.pop(f)
    assert got == plain and len(plain) >= 8
