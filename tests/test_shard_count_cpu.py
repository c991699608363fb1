"""`pfq_db_shard_count` / `BloomTree.shard_count` (the size of the depth-d frontier that pfq_tree_open_subtree indexes) and
the argument checks of `phage_filter query --shard-depth`, all without a device: only tree.bin is read."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pfq_format as fmt
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree
from phagefilter_amd._ffi import PfqError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
EX = os.path.join(ROOT, "tests", "golden", "examples")
PFQ_ERR_IO, PFQ_ERR_FORMAT = -2, -3


def _dna(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).astype(np.uint8))


def greedy_genomes(seed=0):
    """One base genome, a long unrelated one, then variants of the base: the greedy descent keeps the unrelated genome
    at depth 1 and stacks the variants on the other side (leaves from depth 1 to 5)."""
    rng = np.random.default_rng(seed)
    base = _dna(rng, 900)

    def mut(g, m):
        g = bytearray(g)
        for _ in range(m):
            g[int(rng.integers(0, len(g)))] = ord("ACGT"[int(rng.integers(0, 4))])
        return bytes(g)

    genomes = [base, _dna(rng, 2000)] + [mut(base, 2 * i) for i in range(1, 10)]
    return genomes, [f"g{i}" for i in range(len(genomes))]


def leaf_depths(t):
    out, st = [], [(t.root, 0)]
    while st:
        v, d = st.pop()
        if t.is_leaf(v):
            out.append(d)
        st += [(c, d + 1) for c in (t.left[v], t.right[v]) if c >= 0]
    return out


def oracle_frontier_size(t, depth):
    n = 0
    while True:
        try:
            orc.subtree_shard(t, depth, n)
        except IndexError:
            return n
        n += 1


def balanced_db(directory, n_leaves):
    t = orc.balanced_topology([f"L{i}" for i in range(n_leaves)], 15, 1024, 3, 1, 2, 0.01, 2000)
    fmt.write_db(t, directory)
    return t


@pytest.fixture(scope="module")
def dbs(tmp_path_factory):
    base = tmp_path_factory.mktemp("shards")
    out = {"balanced12": balanced_db(str(base / "balanced12"), 12), "single": balanced_db(str(base / "single"), 1)}
    genomes, ids = greedy_genomes()
    g = orc.build_greedy_tree(genomes, ids, 15, 0.01, 2000, 5, 10)
    fmt.write_db(g, str(base / "greedy"))
    out["greedy"] = g
    return base, out


def test_shard_count_equals_the_oracle_frontier(dbs):
    base, trees = dbs
    assert min(leaf_depths(trees["greedy"])) < 2 < max(leaf_depths(trees["greedy"]))  # leaves above the depth-2 cut
    for name, t in trees.items():
        height = max(leaf_depths(t))
        for d in range(height + 3):
            assert BloomTree.shard_count(str(base / name), d) == oracle_frontier_size(t, d), (name, d)
    assert BloomTree.shard_count(str(base / "balanced12"), 1) == 2
    assert BloomTree.shard_count(str(base / "balanced12"), 10) == 12
    assert BloomTree.shard_count(str(base / "single"), 0) == 1 and BloomTree.shard_count(str(base / "single"), 5) == 1


def test_shard_count_errors(dbs, tmp_path):
    with pytest.raises(PfqError) as e:
        BloomTree.shard_count(str(tmp_path / "missing"), 1)
    assert e.value.code == PFQ_ERR_IO
    base, _ = dbs
    cut = tmp_path / "cut"
    cut.mkdir()
    raw = open(base / "balanced12" / "tree.bin", "rb").read()
    (cut / "tree.bin").write_bytes(raw[: len(raw) // 2])
    with pytest.raises(PfqError) as e:
        BloomTree.shard_count(str(cut), 1)
    assert e.value.code == PFQ_ERR_FORMAT


def test_cli_shard_depth_argument_checks(dbs, tmp_path):
    """Checked before any device is touched: fewer shards than devices, and a depth that is not an integer."""
    base, _ = dbs
    cmd = [CLI, "query", "--reads", os.path.join(EX, "reads"), "--out", str(tmp_path / "o"), "--db-path", str(base / "balanced12")]
    p = subprocess.run(cmd + ["--shard-depth", "1", "--devices", "0,0,0"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 101, p.stderr
    assert "2 subtree shards" in p.stderr and "3 devices" in p.stderr and "depth 1" in p.stderr, p.stderr
    assert p.stdout == ""
    p = subprocess.run(cmd + ["--shard-depth", "x"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 101 and "invalid value 'x' for '--shard-depth'" in p.stderr, p.stderr
    # the effective depth is min(--shard-depth, --search-depth): depth 0 has one shard, fewer than two devices
    p = subprocess.run(cmd + ["--shard-depth", "3", "--search-depth", "0", "--devices", "0,0"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 101 and "1 subtree shards at depth 0" in p.stderr, p.stderr
