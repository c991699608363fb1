"""pfq_prep_deplete with the screen in every regime the host can pick for its classification.  In depletion mode QueryRun reads
its cursors through the caller's stream (the depleted tree's copy stream) instead of the null stream, on every path: the direct
kernel, the pair pipeline with LDS tiles on and off, block mode, and under the knobs that change how tiles are listed, packed,
streamed and emitted.  Each case depletes one small block against a screen of the smallest size at which the rules of
tests/test_gpu_regimes.py (expected_regime) name another (path, tile_mode, n_slices, tile_bin_build), holds the result against
tests/deplete_ref.py and the screen's counters against the reference's, and asserts through pfq_last_stats of the screen that the
depletion's classification ran in the regime the case was written for."""
import pytest

import mixed_model as mm
import prep_ref
from oracle import pfq_oracle as orc
from phagefilter_amd import BloomTree
from test_gpu_deplete import HA, KA, SEEDS_A, Case, fragments, fresh
from test_gpu_prep import counts_of
from test_gpu_regimes import GEOMETRIES, KNOB_NBITS, expected_regime, regime_of, with_knobs

# screen sizes below 2^24 bits, from the tables of tests/test_gpu_regimes.py (its knob tree, its hash-count tree, its geometries)
SIZES = sorted({KNOB_NBITS, 1_048_573} | {g[0] for g in GEOMETRIES if g[0] < 1 << 24})
# the knob sets of the screen: those of mixed_model.KNOBS that touch a query, LDS tiles off, and the direct path
QUERY_KNOBS = [{name: value} for name, value in mm.KNOBS if not name.startswith(("PFQ_FMT", "PFQ_FRAME", "PFQ_SWEEP", "PFQ_SIM"))]
SETS = [({}, 1)] + [(k, 1) for k in QUERY_KNOBS] + [({"PFQ_TILE": "0"}, 1), ({}, 0)]


def pinned(knobs):
    """The knobs with block mode pinned: left to itself the host picks it from the candidates per read of earlier calls."""
    return dict({"PFQ_BLOCK": "0"}, **knobs)


def regime(nbits, thr, knobs, path):
    k = pinned(knobs)
    return expected_regime(nbits, HA, thr, path=path, block=k["PFQ_BLOCK"] == "1", knobs=k)


def sizes_for(thr, knobs, path):
    """The smallest size of SIZES for each distinct regime this (threshold, knobs, path) reaches on them."""
    first = {}
    for nbits in SIZES:
        first.setdefault(regime(nbits, thr, knobs, path), nbits)
    return sorted(first.values())


def test_the_sizes_reach_every_regime_below_2_24():
    """Judged without a device: together the cases name the direct kernel, the pair pipeline with and without tiles, block mode,
    and every k_tile_bin build expected_regime gives for a filter below 2^24 bits."""
    seen = {regime(n, thr, k, path) for thr in (1.0, 0.7) for k, path in SETS for n in sizes_for(thr, k, path)}
    every = {regime(n, thr, k, path) for thr in (1.0, 0.7) for k, path in SETS for n in SIZES}
    assert seen == every and len(seen) >= 7, sorted(seen, key=str)
    assert {r[1] for r in seen} == {0, 1, 2} and {r[0] for r in seen} == {0, 1}


class Screens(Case):
    """The block and the main tree of test_gpu_deplete.Case, and screen A's genomes at every size of SIZES, built when first asked
    for; the references per (size, threshold, paired) are computed once."""

    def __init__(self):
        super().__init__()
        self.ids_a = [f"A{i:02d}" for i in range(4)]
        self.trees, self.refs = {}, {}
        self.pairs = fragments(self)
        self.blocks = {False: (self.prep["kept_reads"], prep_ref.prep_block(self.prep["kept_reads"], None, min_length=5)),
                       True: (self.pairs, prep_ref.prep_block(self.pairs, None, paired=True, min_length=5))}

    def screen(self, nbits):
        if nbits not in self.trees:
            self.trees[nbits] = (orc.build_balanced_tree(self.a_g, self.ids_a, KA, nbits, HA, *SEEDS_A),
                                 BloomTree.build_balanced(self.a_g, self.ids_a, KA, nbits, HA, *SEEDS_A))
        return self.trees[nbits]

    def reference(self, nbits, thr, paired):
        key = (nbits, thr, paired)
        if key not in self.refs:
            self.refs[key] = self.deplete(self.blocks[paired][1], self.screen(nbits)[0], thr, paired=paired)
        return self.refs[key]


@pytest.fixture(scope="module")
def screens(gpu):
    x = Screens()
    yield x
    for t in [x.main, x.a, x.b] + [gt for _, gt in x.trees.values()]:
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,path", SETS, ids=[",".join(f"{k[4:]}={v}" for k, v in d.items()) or ("default" if p else "direct path") for d, p in SETS])
@pytest.mark.parametrize("paired", [False, True], ids=["reads", "fragments"])
@pytest.mark.parametrize("thr", [1.0, 0.7])
def test_screen_regimes(screens, thr, paired, knobs, path):
    main = screens.main
    reads, _ = screens.blocks[paired]
    for nbits in sizes_for(thr, knobs, path):
        _, gt = screens.screen(nbits)
        want = screens.reference(nbits, thr, paired)
        assert 0 < want["units_removed"] < want["n_units"], (nbits, want["units_removed"])
        fresh(gt)
        gt.set_path(path)

        def run():
            screens.prepare(reads, None, paired=paired, min_length=5)
            got = main.prep_deplete(gt, thr, paired=paired)
            return got, regime_of(gt.last_stats())
        try:
            got, ran_in = with_knobs(gt, pinned(knobs), run)
        finally:
            gt.set_path(-1)
        screens.check(got, want, (nbits, thr, paired, knobs, path))
        assert counts_of(gt).tolist() == want["leaf_counts"], (nbits, thr, paired, knobs, path)
        assert ran_in == regime(nbits, thr, knobs, path), (nbits, thr, paired, knobs, path, ran_in)
        fresh(gt)
