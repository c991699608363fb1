"""`phage_filter query --taxonomy FILE [--taxon-reads]`: TAXON_COUNTS.tsv and READ_TAXA.tsv must equal the text built here from
the oracle's hit sets (orc.query_batch) and tests/tax_ref.py, on the database the CLI's own `build` makes of the example
genomes, with a taxonomy file written here; reads_any of the genome lines must be CLASSIFICATION.csv's counts; the `estimated`
column of --abundance comes from tests/abund_ref.py; CLASSIFICATION.csv and every other output must be byte-identical to the
run without the option; --reads2 counts fragments; two replicas on one device must give what one gives."""
import os
import subprocess

import pytest

import abund_ref
import tax_ref
from oracle import pfq_format as fmt
from test_gpu_cli_lca import CLI, EX, FASTQ, SEEDS, TIMEOUT, fastq_records, query, write_fasta
from test_gpu_lca import oracle_sets
from test_gpu_paired import combine, mate_sets

pytestmark = pytest.mark.gpu

HEADER = "#node\tparent\tdepth\tkind\tgenomes\tname\treads_here\treads_below\treads_any"


@pytest.fixture(scope="module")
def examples(gpu, tmp_path_factory):
    """The examples database by the CLI's own greedy `build`, read back for the oracle; a taxonomy file over its genomes:
    nested lineages, one genome under the root by an empty lineage and one by having no line, lines for genomes that are
    not there, a comment, CRLF and a third column."""
    base = tmp_path_factory.mktemp("tax_cli")
    db = str(base / "db")
    p = subprocess.run([CLI, "build", "--genomes", os.path.join(EX, "genomes"), "--db-path", db, "--seed1", str(SEEDS[0]),
                        "--seed2", str(SEEDS[1])], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr
    ot = fmt.read_db(db)
    names = [ot.tax_id[v] for v in ot.leaves_dfs()]
    assert len(names) >= 4
    lineages = ["Caudoviricetes;Autographiviridae;Teseptimavirus", "Caudoviricetes;Autographiviridae", "Caudoviricetes; Straboviridae ;Tequatrovirus",
                "Caudoviricetes", "", "Microviridae;Sinsheimervirus"]
    lines = ["# genome\tlineage\taccession\r\n", "not_in_this_database\tCaudoviricetes;Elsewhere\r\n"]
    for i, g in enumerate(sorted(names)[:-1]):                      # the last one has no line
        lines.append(f"{g}\t{lineages[i % len(lineages)]}\tACC{i}\r\n")
    lines.append("another_absent_genome\t\r\n")
    data = "".join(lines).encode()
    path = base / "taxonomy.tsv"
    path.write_bytes(data)
    parent, tnames, leaf_taxon, info = tax_ref.parse(data, names)
    assert info["lines_other"] == 2 and info["leaves_without_line"] == 1
    return db, ot, names, fastq_records(FASTQ), str(path), tax_ref.Nodes(names, parent, tnames, leaf_taxon)


def counts_tsv(ref, sets, mass=None):
    last, here, below, any_ = ref.counts(sets)
    lines = [HEADER + ("\testimated" if mass is not None else "") + "\n"]
    node_mass = [0] * ref.n
    if mass is not None:
        for l, v in enumerate(ref.leaf_node):
            for t in ref.ancestors(v):
                node_mass[t] += mass[l]
    for v, (parent, depth, _, n_leaves, leaf, name) in enumerate(ref.table):
        if any_[v]:
            line = f"{v}\t{'-' if parent < 0 else parent}\t{depth}\t{'genome' if leaf >= 0 else 'taxon'}\t{n_leaves}\t{name}\t{int(here[v])}\t{int(below[v])}\t{int(any_[v])}"
            if mass is not None:
                milli = (node_mass[v] * 1000 + 32768) >> 16
                line += f"\t{milli // 1000}.{milli % 1000:03d}"
            lines.append(line + "\n")
    return "".join(lines).encode(), last, any_


def reads_tsv(ref, ids, sets, last):
    lines = ["#read_id\thits\tnode\tname\n"]
    for rid, s, v in zip(ids, sets, last):
        if s:
            lines.append(f"{rid}\t{len(s)}\t{int(v)}\t{ref.table[int(v)][5]}\n")
    return "".join(lines).encode()


def classification(names, ref, any_):
    return "".join(f"{g},{int(any_[ref.leaf_node[l]])}\n" for l, g in enumerate(names) if any_[ref.leaf_node[l]]).encode()


@pytest.mark.parametrize("thr", ["1.0", "0.3"])
def test_examples_database(examples, tmp_path, thr):
    db, ot, names, recs, tax, ref = examples
    sets = oracle_sets(ot, [s for _, s in recs], float(thr))
    want_counts, last, any_ = counts_tsv(ref, sets)
    want_reads = reads_tsv(ref, [rid for rid, _ in recs], sets, last)
    assert sum(1 for s in sets if len(s) > 1) > 0
    r = ["--reads", FASTQ]
    # alone (what would be the counts-only mode): TAXON_COUNTS.tsv next to an unchanged CLASSIFICATION.csv
    out0, plain = query(db, str(tmp_path / "p0"), *r, thr=thr)
    out1, got = query(db, str(tmp_path / "t0"), *r, "--taxonomy", tax, thr=thr)
    assert got.pop("TAXON_COUNTS.tsv") == want_counts, thr
    assert got == plain and out1 == out0
    assert plain["CLASSIFICATION.csv"] == classification(names, ref, any_)      # reads_any of the genome lines
    # with --taxon-reads and every other per-read output
    extra = ["--pos-filter", "--neg-filter", "--scores", "--lca", "all", "--lca-reads", "--coverage"]
    out0, plain = query(db, str(tmp_path / "p1"), *r, *extra, thr=thr)
    out1, got = query(db, str(tmp_path / "t1"), *r, *extra, "--taxonomy", tax, "--taxon-reads", thr=thr)
    assert got.pop("TAXON_COUNTS.tsv") == want_counts, thr
    assert got.pop("READ_TAXA.tsv") == want_reads, thr
    assert got == plain and out1 == out0 and len(plain) == 7
    # --abundance: one more column, the EM masses of the genomes below each node
    est = abund_ref.estimate(abund_ref.classify([sorted(s) for s in sets], len(names)), 200, 65)
    _, plain = query(db, str(tmp_path / "p2"), *r, "--abundance", thr=thr)
    _, got = query(db, str(tmp_path / "t2"), *r, "--abundance", "--taxonomy", tax, thr=thr)
    assert got.pop("TAXON_COUNTS.tsv") == counts_tsv(ref, sets, est["mass"])[0], thr
    assert got == plain
    # two replicas on one device: each counts its own reads, the sums are one device's
    _, two = query(db, str(tmp_path / "d"), *r, "--taxonomy", tax, "--taxon-reads", "--devices", "0,0", thr=thr, threads="3", block="17")
    assert two["TAXON_COUNTS.tsv"] == want_counts and two["READ_TAXA.tsv"] == want_reads
    assert two["CLASSIFICATION.csv"] == plain["CLASSIFICATION.csv"]


@pytest.mark.parametrize("pair_mode", ["either", "both"])
def test_reads2_counts_fragments(examples, tmp_path, pair_mode):
    db, ot, names, recs, tax, ref = examples
    recs = recs[:2 * (min(len(recs), 3000) // 2)]
    pairs = [(recs[2 * i][1], recs[2 * i + 1][1]) for i in range(len(recs) // 2)]
    r1 = write_fasta(tmp_path / "r1.fa", [(f"f{i}/1", p[0]) for i, p in enumerate(pairs)])
    r2 = write_fasta(tmp_path / "r2.fa", [(f"f{i}/2", p[1]) for i, p in enumerate(pairs)])
    thr = "0.5"
    frag = combine(mate_sets(ot, [m for p in pairs for m in p], float(thr)), pair_mode)
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    want_counts, last, any_ = counts_tsv(ref, frag)
    want_reads = reads_tsv(ref, [f"f{i}/1" for i in range(len(pairs))], frag, last)
    src = ["--reads", r1, "--reads2", r2, "--pair-mode", pair_mode]
    _, plain = query(db, str(tmp_path / "p"), *src, "--pos-filter", "--neg-filter", thr=thr)
    _, got = query(db, str(tmp_path / "t"), *src, "--pos-filter", "--neg-filter", "--taxonomy", tax, "--taxon-reads", thr=thr)
    assert got.pop("TAXON_COUNTS.tsv") == want_counts and got.pop("READ_TAXA.tsv") == want_reads
    assert got == plain and plain["CLASSIFICATION.csv"] == classification(names, ref, any_)
    _, alone = query(db, str(tmp_path / "c"), *src, "--taxonomy", tax, thr=thr)                   # no other per-read output
    assert sorted(alone) == ["CLASSIFICATION.csv", "TAXON_COUNTS.tsv"] and alone["TAXON_COUNTS.tsv"] == want_counts
    assert alone["CLASSIFICATION.csv"] == plain["CLASSIFICATION.csv"]
    _, two = query(db, str(tmp_path / "d"), *src, "--taxonomy", tax, "--taxon-reads", "--devices", "0,0", thr=thr, block="16")
    assert two["TAXON_COUNTS.tsv"] == want_counts and two["READ_TAXA.tsv"] == want_reads
