"""`build` / `add` on the device against the oracle's greedy insertion, at the sizes where the insertion kernels' own code
paths run: k_greedy_insert's 4-wide streaming loop and its tail at every grid size the walk may use, k_insert's grid-stride
loop on long genomes, the device copy of the topology regrowing, the host walk and the device walk taking turns on one
tree; and an insertion that fails stays failed (include/pfq.h, pfq_tree_insert).

Every case compares the device tree with orc.build_greedy_tree / orc.greedy_insert on the same genomes and seeds: topology,
names and leaf order (tree.bin of a save, byte for byte) and every node's filter (pfq_debug_node_filter, pre-order)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree, PfqError, pack_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
PFQ_ERR_FORMAT = -3
ONE_CHILD = "Node with only one child encountered - should not happen."
INSERT_PASS = 1024 * 4 * 64          # k-mers launch_insert_one covers per grid pass (blocks x waves x window)


def _dna(rng, n):
    return ACGT[rng.integers(0, 4, int(n))].tobytes()


def _mutate(rng, g, n_subs):
    g = bytearray(g)
    for p in rng.integers(0, len(g), int(n_subs)):
        g[int(p)] = ACGT[(ACGT.tobytes().find(bytes([g[int(p)]])) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(g)


def _families(rng, n, n_fam, lengths, sub_rate):
    """n genomes in n_fam families of mutated copies (the distances within a family are close); genome i has length
    lengths[i] (a prefix or an extension of its family's base)."""
    base = [_dna(rng, max(lengths)) for _ in range(n_fam)]
    out = []
    for i in range(n):
        g = base[int(rng.integers(0, n_fam))][: int(lengths[i])]
        out.append(_mutate(rng, g, rng.binomial(len(g), sub_rate)) if g else g)
    return out


def _assert_same_tree(gt, ot, tmp_path, name, keep=False):
    """The device tree == the oracle tree (renumbered into pre-order here): tree.bin of a save byte for byte (topology,
    names, leaf order, counters, parameters) and every node's filter.  The saved directory is removed unless `keep`."""
    orc.renumber_preorder(ot)
    info = gt.info()
    assert (info.n_nodes, info.n_leaves, info.nbits, info.num_hashes) == \
        (ot.n_nodes, len(ot.leaves_dfs()), ot.nbits, ot.num_hashes)
    assert info.superset_verified == 1
    for v in range(ot.n_nodes):
        assert np.array_equal(gt.node_filter(v), ot.bits[ot.filter_of[v]]), (name, v, ot.tax_id[v])
    d = tmp_path / name
    gt.save(str(d))
    assert (d / "tree.bin").read_bytes() == fmt.encode_tree(ot), name
    assert sorted(os.listdir(d)) == sorted(set(ot.bf_path) | {"tree.bin"})
    if not keep:
        shutil.rmtree(d)
    return d


def _check_query(gt, ot, reads, thr):
    """Per-leaf counts and per-read hit sets of one query call == the oracle's DFS; counters cleared afterwards."""
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    gt.reset_counts()
    seq, off = pack_reads(reads)
    offs, leaves = gt.query_packed(seq, off, thr, want_hits=True)
    ohits, _, _ = orc.query_batch(ot, reads, thr)
    col = {v: i for i, v in enumerate(ot.leaves_dfs())}
    got = sorted((r, int(leaves[j])) for r in range(len(reads)) for j in range(int(offs[r]), int(offs[r + 1])))
    assert gt.get_leaf_counts() == ot.leaf_counts(), thr
    assert got == sorted((r, col[v]) for r, v in ohits), thr
    assert len(ohits) > 0
    gt.reset_counts()
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0


def _reads(rng, genomes, n, length):
    out = []
    for _ in range(n):
        g = genomes[int(rng.integers(0, len(genomes)))]
        if len(g) < length:
            continue
        o = int(rng.integers(0, len(g) - length + 1))
        r = g[o:o + length]
        out.append(orc.revcomp(r) if rng.random() < 0.5 else r)
    return out + [_dna(rng, length) for _ in range(n // 4)]


def _cu_count():
    hip = C.CDLL("libamdhip64.so")
    v, warp = C.c_int(0), C.c_int(0)
    # hipDeviceAttributeMultiprocessorCount = 63, hipDeviceAttributeWarpSize = 87 (hip_runtime_api.h)
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0 and hip.hipDeviceGetAttribute(C.byref(warp), 87, 0) == 0
    assert warp.value == 64 and v.value > 0, (v.value, warp.value)   # (the enum's numbering is the one above)
    return v.value


class _GreedyBlocks:
    """PFQ_GREEDY_BLOCKS for the trees whose first insertion happens inside the block (it is read once per tree)."""

    def __init__(self, blocks):
        self.blocks = blocks

    def __enter__(self):
        self.old = os.environ.get("PFQ_GREEDY_BLOCKS")
        if self.blocks is None:
            os.environ.pop("PFQ_GREEDY_BLOCKS", None)
        else:
            os.environ["PFQ_GREEDY_BLOCKS"] = str(self.blocks)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("PFQ_GREEDY_BLOCKS", None)
        else:
            os.environ["PFQ_GREEDY_BLOCKS"] = self.old


# ---------------------------------------------------------------------------------------------------------------
# the geometry of the README's build rate: 71 887 936 bits, 10 hashes, 1 123 249 words per filter
# ---------------------------------------------------------------------------------------------------------------
def test_full_geometry_build_then_add(gpu, tmp_path):
    """48 genomes of ~50 kbp in families (1 % apart) with the default grid: every thread runs the 4-wide loop twice, then
    the tail.  The first three are one genome (the third meets a tie at the root: distance 0 to both children, it goes
    left); one genome of 300 kbp (k_insert's second grid pass) and one shorter than k (an empty filter).  Then save,
    reload and add."""
    rng = np.random.default_rng(20261015)
    k, fpr, largest = 21, 0.001, 5_000_000
    lengths = rng.integers(45_000, 55_000, 48)
    genomes = _families(rng, 48, 8, lengths, 0.01)
    genomes[1] = genomes[0]
    genomes[2] = genomes[0]
    genomes[30] = genomes[0]
    genomes[12] = _dna(rng, INSERT_PASS + 37_000)
    genomes[20] = genomes[5][: k - 1]
    more = _families(rng, 4, 2, rng.integers(45_000, 55_000, 4), 0.01)
    more[1] = genomes[0]
    ids = [f"F{i:02d}" for i in range(len(genomes))]
    more_ids = [f"A{i}" for i in range(len(more))]
    gt = BloomTree.new(k, fpr, largest, *SEEDS)
    assert (gt.info().nbits, gt.info().num_hashes) == (71887936, 10)
    ot = orc.OracleTree(k, 71887936, 10, *SEEDS, fpr, largest)
    orc.reserve_rows(ot, 2 * (len(genomes) + len(more)) - 1)     # (host memory: no copy while the rows grow)
    for g, i in zip(genomes, ids):
        gt.insert(g, i)
        orc.greedy_insert(ot, g, i)
    db = _assert_same_tree(gt, ot, tmp_path, "built", keep=True)
    gt.close()
    gt = BloomTree.load(str(db))
    shutil.rmtree(db)
    for g, i in zip(more, more_ids):
        gt.insert(g, i)
        orc.greedy_insert(ot, g, i)
    _assert_same_tree(gt, ot, tmp_path, "added")
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# k_greedy_insert's loop shapes and grid barrier at small sizes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [1, 3, 16, 17, None])
def test_greedy_loop_and_barrier_shapes(gpu, tmp_path, blocks):
    """A balanced start, then greedy insertions, with PFQ_GREEDY_BLOCKS = blocks (None: the library's default, half the
    CUs) and T = blocks x 1024 threads: filters of 3T - 1, 3T and 3T + 1 words (the 4-wide loop runs for no thread, for
    none, for thread 0 alone), 4T and 4T + 1 (once for every thread, then the tail) and 7T + 5 (twice for the first five
    threads).  One to sixteen groups at the barrier, and groups of unequal size (3, 17 blocks)."""
    n_blocks = blocks if blocks is not None else min(256, _cu_count(), _cu_count() // 2)
    T = n_blocks * 1024
    rng = np.random.default_rng(1000 + n_blocks)
    k, h = 17, 4
    for j, n_words in enumerate((3 * T - 1, 3 * T, 3 * T + 1, 4 * T, 4 * T + 1, 7 * T + 5)):
        nbits = 64 * n_words - (0 if j % 2 else 1 + 13 * j)
        genomes = _families(rng, 14, 3, rng.integers(2000, 6000, 14), 0.01)
        genomes[9] = genomes[6]
        genomes[11] = genomes[6]                             # (identical copies: distance 0)
        ids = [f"s{i}" for i in range(len(genomes))]
        start = 5
        with _GreedyBlocks(blocks):
            gt = BloomTree.build_balanced(genomes[:start], ids[:start], k, nbits, h, *SEEDS)
            ot = orc.build_balanced_tree(genomes[:start], ids[:start], k, nbits, h, *SEEDS)
            for g, i in zip(genomes[start:], ids[start:]):
                gt.insert(g, i, internal_name=f"in_{i}")
                orc.greedy_insert(ot, g, i, internal_name=f"in_{i}")
        _assert_same_tree(gt, ot, tmp_path, f"b{n_blocks}_w{n_words}")
        gt.close()


# ---------------------------------------------------------------------------------------------------------------
# leaf filters of long and edge-length genomes through `insert`
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 21, 31])
def test_insert_leaf_filters_edge_lengths(gpu, tmp_path, k):
    """Genomes of 0, k - 1 (no k-mer), k (one), k + 63, k + 64 (a window of 64 k-mers and one more), 2^18 + k - 1 (one
    full grid pass of k_insert exactly), 2^18 + k (one k-mer in a second pass) and 1 000 003 bases (four passes), and one
    with N, lowercase and other IUPAC bytes."""
    rng = np.random.default_rng(31 * k)
    lengths = [k - 1, k, k + 63, k + 64, INSERT_PASS + k - 1, INSERT_PASS + k, 1_000_003, 0]
    genomes = [_dna(rng, n) for n in lengths]
    iupac = bytearray(_dna(rng, 6000))
    for p in rng.integers(0, len(iupac), 300):
        iupac[int(p)] = b"NnacgtRYKMSWBDHV"[int(rng.integers(0, 16))]
    iupac[100:180] = iupac[100:180].lower()
    genomes.append(bytes(iupac))
    genomes.append(genomes[6][: 2 * INSERT_PASS])             # a long genome that shares half of its k-mers with another
    ids = [f"e{i}" for i in range(len(genomes))]
    gt = BloomTree.new(k, 0.05, 1_000_003, *SEEDS)
    ot = orc.OracleTree(k, gt.info().nbits, gt.info().num_hashes, *SEEDS, 0.05, 1_000_003)
    assert (ot.nbits, ot.num_hashes) == (orc.needed_bits(0.05, 1_000_003), orc.optimal_num_hashes(ot.nbits, 1_000_003))
    for g, i in zip(genomes, ids):
        gt.insert(g, i)
        orc.greedy_insert(ot, g, i)
    _assert_same_tree(gt, ot, tmp_path, "edge")
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# many insertions on one tree: the device topology regrows, filter rows and staging buffers reallocate
# ---------------------------------------------------------------------------------------------------------------
def test_many_insertions_regrow_topology(gpu, tmp_path):
    """700 genomes of 200 - 2000 bases (families; lengths that grow from one insertion to the next, so the four staging
    slots reallocate while the insertions before are in flight) cross the 1024 nodes d_topo starts with and several
    growths of the filter rows; then save, reload and add 300 more."""
    rng = np.random.default_rng(700)
    n1, n2 = 700, 300
    lengths = np.linspace(200, 2000, n1 + n2).astype(int)
    genomes = _families(rng, n1 + n2, 40, lengths, 0.02)
    genomes[1] = genomes[0]
    genomes[2] = genomes[0]                                   # (a tie at the root)
    genomes[500] = genomes[400]
    genomes[801] = genomes[400]
    ids = [f"m{i:04d}" for i in range(n1 + n2)]
    k, fpr, largest = 15, 0.01, 3000
    gt = BloomTree.new(k, fpr, largest, *SEEDS)
    ot = orc.OracleTree(k, gt.info().nbits, gt.info().num_hashes, *SEEDS, fpr, largest)
    for g, i in zip(genomes[:n1], ids[:n1]):
        gt.insert(g, i)
        orc.greedy_insert(ot, g, i)
    db = _assert_same_tree(gt, ot, tmp_path, "built", keep=True)
    gt.close()
    gt = BloomTree.load(str(db))
    for g, i in zip(genomes[n1:], ids[n1:]):
        gt.insert(g, i)
        orc.greedy_insert(ot, g, i)
    _assert_same_tree(gt, ot, tmp_path, "added")
    _check_query(gt, ot, _reads(rng, genomes, 400, 100), 1.0)
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# insertions, queries, filter reads and saves interleaved on one tree; the host walk and the device walk take turns
# ---------------------------------------------------------------------------------------------------------------
def test_interleaved_insert_query_save_and_walks(gpu, tmp_path):
    rng = np.random.default_rng(4242)
    genomes = _families(rng, 60, 6, rng.integers(500, 2500, 60), 0.02)
    genomes[1] = genomes[0]
    genomes[2] = genomes[0]
    genomes[33] = genomes[0]
    ids = [f"x{i:02d}" for i in range(len(genomes))]
    k, fpr, largest = 17, 0.01, 2500
    gt = BloomTree.new(k, fpr, largest, *SEEDS)
    ot = orc.OracleTree(k, gt.info().nbits, gt.info().num_hashes, *SEEDS, fpr, largest)
    it = iter(zip(genomes, ids))

    def insert(n, host):
        gt.set_option("PFQ_GREEDY_HOST", "1" if host else None)
        for _ in range(n):
            g, i = next(it)
            gt.insert(g, i)
            orc.greedy_insert(ot, g, i)

    insert(12, False)
    orc.renumber_preorder(ot)
    _check_query(gt, ot, _reads(rng, genomes[:12], 200, 120), 1.0)
    insert(8, True)                                     # (after a query: the layout is rebuilt, the walk on the host)
    orc.renumber_preorder(ot)
    for v in range(ot.n_nodes):
        assert np.array_equal(gt.node_filter(v), ot.bits[ot.filter_of[v]]), v
    insert(10, False)                                   # the device walk takes over the shape the host walk left
    _assert_same_tree(gt, ot, tmp_path, "saved")
    insert(6, False)
    insert(6, True)
    _check_query(gt, ot, _reads(rng, genomes[:42], 200, 120), 0.7)
    insert(1, False)
    insert(1, True)
    insert(16, False)
    _assert_same_tree(gt, ot, tmp_path, "last")
    _check_query(gt, ot, _reads(rng, genomes, 300, 120), 1.0)
    gt.close()


# ---------------------------------------------------------------------------------------------------------------
# a failed insertion is sticky
# ---------------------------------------------------------------------------------------------------------------
def _one_child_db(directory, deep):
    """A database with a node of one child, which the reference's walk panics on (bloom_tree.rs:209), and the genome that
    walks into it: at the root (deep = False), or two levels down under two full nodes that absorb the new leaf on the
    way (deep = True: root = (P, X), P = (Q, Y), Q = (A, -))."""
    rng = np.random.default_rng(5 + deep)
    k, nbits, h = 15, 40000, 4
    g = {n: _dna(rng, 1500) for n in "AXY"}
    t = orc.OracleTree(k, nbits, h, *SEEDS)
    rows = {}

    def leaf(n):
        rows[n] = len(rows)
        return t.add_node(n, f"{n}.bf", rows[n])

    def inner(n, left, right):
        rows[n] = len(rows)
        return t.add_node(n, f"{n}.bf", rows[n], left, right)

    if deep:
        t.root = inner("R", -1, -1)
        p = inner("P", -1, -1)
        q = inner("Q", -1, -1)
        a = leaf("A")
        t.left[q] = a
        y = leaf("Y")
        t.left[p], t.right[p] = q, y
        x = leaf("X")
        t.left[t.root], t.right[t.root] = p, x
    else:
        t.root = inner("R", -1, -1)
        t.left[t.root] = leaf("A")
    t.bits = np.zeros((len(rows), t.n_words), dtype=np.uint64)
    for n in ("A", "X", "Y"):
        if n in rows:
            orc.insert_sequence(t, rows[n], g[n])
    if deep:
        t.bits[rows["Q"]] = t.bits[rows["A"]]
        t.bits[rows["P"]] = t.bits[rows["Q"]] | t.bits[rows["Y"]]
        t.bits[rows["R"]] = t.bits[rows["P"]] | t.bits[rows["X"]]
    else:
        t.bits[rows["R"]] = t.bits[rows["A"]]
    fmt.write_db(t, str(directory))
    # the oracle's walk meets the one-child node (with the ancestors' unions done on the way)
    with pytest.raises(RuntimeError, match="only one child"):
        orc.greedy_insert(fmt.read_db(str(directory)), g["A"], "new")
    return g["A"]


def _snapshot(directory):
    return {n: (directory / n).read_bytes() for n in sorted(os.listdir(directory))}


@pytest.mark.parametrize("host_walk", [False, True])
@pytest.mark.parametrize("deep", [False, True])
def test_failed_insertion_is_sticky(gpu, tmp_path, deep, host_walk):
    db = tmp_path / "db"
    genome = _one_child_db(db, deep)
    before = _snapshot(db)
    gt = BloomTree.load(str(db))
    gt.set_option("PFQ_GREEDY_HOST", "1" if host_walk else None)
    out = tmp_path / "out"
    err = None
    try:
        gt.insert(genome, "new")
    except PfqError as e:
        err = e
    if host_walk:
        assert err is not None                      # the host walk meets the one-child node inside pfq_tree_insert
    else:
        assert err is None                          # the device walk's failure surfaces at the next call needing the shape
        with pytest.raises(PfqError) as first:
            gt.save(str(out))
        err = first.value
    assert err.code == PFQ_ERR_FORMAT and ONE_CHILD in str(err), err
    info = gt.info()                                # still answers
    assert (info.kmer_size, info.nbits) == (15, 40000)
    seq, off = pack_reads([genome[:100], genome[200:350]])
    calls = [("save", lambda: gt.save(str(out))), ("query", lambda: gt.query_packed(seq, off, 1.0)),
             ("query hits", lambda: gt.query_packed(seq, off, 0.5, want_hits=True)),
             ("insert", lambda: gt.insert(genome[:700], "other")), ("leaf counts", gt.get_leaf_counts),
             ("save leaf counts", lambda: gt.save_leaf_counts(str(tmp_path / "c.csv"))),
             ("prune", lambda: gt.prune_tree(1)), ("save again", lambda: gt.save(str(out)))]
    for name, call in calls:
        with pytest.raises(PfqError) as e:
            call()
        assert e.value.code == PFQ_ERR_FORMAT and ONE_CHILD in str(e.value), name
    assert gt.info().nbits == 40000
    gt.close()
    assert not out.exists() or os.listdir(out) == []
    assert not (tmp_path / "c.csv").exists()
    assert _snapshot(db) == before


@pytest.mark.parametrize("host_walk", [False, True])
@pytest.mark.parametrize("deep", [False, True])
def test_cli_add_onto_one_child_node_panics(gpu, tmp_path, deep, host_walk):
    """`phage_filter add` onto such a database: the reference's panic (status 101, its message), the database untouched."""
    db = tmp_path / "db"
    genome = _one_child_db(db, deep)
    before = _snapshot(db)
    fa = tmp_path / "more.fa"
    fa.write_bytes(b">new\n" + genome + b"\n>later\n" + genome[:900] + b"\n")
    env = dict(os.environ)
    env.pop("PFQ_GREEDY_HOST", None)
    if host_walk:
        env["PFQ_GREEDY_HOST"] = "1"
    p = subprocess.run([CLI, "add", "-g", str(fa), "-d", str(db)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 101 and ONE_CHILD in p.stderr, (p.returncode, p.stderr)
    assert _snapshot(db) == before
