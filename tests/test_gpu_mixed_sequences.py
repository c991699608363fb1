"""One long-lived tree through every entry point, checked per call.  The features that came after tests/test_gpu_call_sequences.py
— text parse / query / format, read preprocessing with adapters and mate overlap, frames, the sweep, best rows, taxonomy,
abundance, coverage, similarity and recluster — share one pfq_tree: the copy stream, the hit rows, the hand-kept validity flags,
two double-buffered CSR pipelines, the workload hints and the accumulators.  Here a seeded deck (tests/mixed_model.py: every
operation at least twice, every adjacent pair of mixed_model.PAIRS) drives one tree through all of them, and every call, every
accumulator, every result of the last call and the validity of format_text are held against the model, whose expectations come
from the oracle and the *_ref modules and whose lifetime rules are those of include/pfq.h.  Since pfq_prep_deplete involves two
trees, a second long-lived tree, the screen, lives beside the first in every deck and in the tests beside the decks: prepared
blocks are depleted against it, it is queried on its own, and after every depletion both trees are held against their models.
PFQ_SEQUENCE_SEEDS sets the number of seeds (default 2)."""
import ctypes as C
import os

import numpy as np
import pytest

import abund_ref
import deplete_ref
import mixed_model as mm
import prep_ref
import sweep_ref
from hipbuf import stream_synchronize
from mixed_model import (PFQ_ERR_ARG, PFQ_ERR_STATE, PFQ_ERR_UNSUPPORTED, Play, Side, TreeModel, check_accumulators, check_format, check_last,
                         raises, rows_of)
from phagefilter_amd import BloomTree, _ffi, pack_reads
from phagefilter_amd.query import allreduce_counts
from test_gpu_call_sequences import K, Model, Runner, check_counts
from test_gpu_parity import gpu_tree
from test_gpu_tax import random_taxonomy
from test_gpu_text import wrap_fastq

pytestmark = pytest.mark.gpu

SEEDS = int(os.environ.get("PFQ_SEQUENCE_SEEDS", "2"))
SWEEP = (0.3, 0.7, 1.0)
ALL_ON = dict(hits=True, scores=True, lca="best", taxa=True, abundance=True, coverage=True, best=True, sweep=True)


def kw_of(f, paired=None):
    """The keywords of query_packed / query_text / query_prep for the model's flags."""
    out = {k: f.get(k, False) for k in ("abundance", "coverage", "taxa", "best", "sweep")}
    out.update(want_hits=f.get("hits", False), want_scores=f.get("scores", False), lca=f.get("lca"), paired=paired is not None, pair_mode=paired or "either")
    return out


@pytest.fixture(scope="module")
def balanced(gpu):
    return mm.balanced_case()


def greedy_tree(genomes, ids):
    gt = BloomTree.new(K, 0.001, 5000, 5, 10)
    for g, i in zip(genomes, ids):
        gt.insert(g, i)
    return gt


def balanced_screen_tree(world):
    """The balanced deck's screen on the device and its model."""
    s = mm.SCREEN_BALANCED
    ids, ot = mm.balanced_screen(world)
    return BloomTree.build_balanced(world.screen, ids, s["k"], s["nbits"], s["h"], *s["seeds"]), TreeModel(ot)


def greedy_screen_tree(world, seed):
    """The greedy deck's screen on the device, its model and the genome it still takes."""
    s = mm.SCREEN_GREEDY
    ids, ot, extra = mm.greedy_screen(world, seed)
    gt = BloomTree.new(s["k"], s["fpr"], s["largest"], *s["seeds"])
    for g, i in zip(world.screen, ids):
        gt.insert(g, i)
    return gt, TreeModel(ot), extra


def play_deck(gt, model, world, seed, d, extra=(), screen=None):
    """screen: (the second tree, its model, the genomes it still takes)."""
    runner, srunner = Runner(gt), Runner(screen[0])
    try:
        play = Play(model, world, seed, gt, runner, extra, mm.Side(screen[1], screen[0], srunner, screen[2]))
        play.run(d)                                                  # (ends with a full read-out of every accumulator of both trees)
        assert play.most_unsynced >= 2
    finally:
        runner.close()
        srunner.close()


# ---------------------------------------------------------------------------------------------------------------
# 1, 2. the decks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(SEEDS))
def test_balanced_tree_mixed_sequence(balanced, seed):
    genomes, ids, ot, world = balanced
    gt = gpu_tree(genomes, ids, K, 131071, 7)
    sgt, sm = balanced_screen_tree(world)
    try:
        play_deck(gt, TreeModel(ot), world, mm.BALANCED_SEED + seed, mm.deck(mm.BALANCED_SEED + seed), screen=(sgt, sm, ()))
    finally:
        gt.close()
        sgt.close()


@pytest.mark.parametrize("seed", range(SEEDS))
def test_greedy_tree_mixed_sequence_with_inserts_and_prune(gpu, seed):
    genomes, ids, ot, world, extra = mm.greedy_case(seed)
    gt = greedy_tree(genomes, ids)
    screen = greedy_screen_tree(world, seed)
    try:
        play_deck(gt, TreeModel(ot), world, mm.GREEDY_SEED + seed, mm.deck(mm.GREEDY_SEED + seed, greedy=True), extra, screen)
    finally:
        gt.close()
        screen[0].close()


# ---------------------------------------------------------------------------------------------------------------
# 3. the pipelines
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ahead", [False, True], ids=["in order", "two blocks ahead"])
def test_pipelines_without_a_synchronising_read(balanced, ahead):
    """Parse A, query_text, prep B, query_prep, host query C, all counts-only, over block sizes that make each CSR set grow while the
    other may still be read; every second prepared block is depleted against a second tree before its query_prep; no result is read
    until the end (a depletion returns its totals), then every counter of both trees against the oracle.  `ahead`: every parse and
    prep is issued twice in a row, so the block that is classified lies in the set the one before it did not take, and a set is
    written again only behind its own event."""
    genomes, ids, ot, world = balanced
    gt = gpu_tree(genomes, ids, K, 131071, 7)
    sgt, sm = balanced_screen_tree(world)
    model = Model(ot)
    params = mm.PREP_PARAMS[1]
    removed = 0
    try:
        for i, n in enumerate((200, 3000, 100, 3000, 50, 1500)):
            thr = (1.0, 0.7)[i % 2]
            for _ in range(2 if ahead else 1):
                a = world.varied(n, longs=())
                gt.parse_text(wrap_fastq(a), "fastq")
            model.query(a, thr)
            gt.query_text(thr)
            for _ in range(2 if ahead else 1):
                b, quals = world.prep_reads(n, True)
                seq, off, qual, hq = mm.pack_quals(b, quals)
                gt.prep_reads(seq, off, qual, hq, **params)
            kept = prep_ref.prep_block(b, quals, **params)["kept_reads"]
            if i % 2:                                                  # every second prepared block is depleted before its classification,
                ref = deplete_ref.deplete(kept, sm.ot, 0.7)            # while the one of the block before is still queued on the other set
                got = gt.prep_deplete(sgt, 0.7)
                assert [got[k] for k in deplete_ref.TOTALS] == [ref[k] for k in deplete_ref.TOTALS], (i, got)
                for c, x in enumerate(ref["leaf_counts"]):
                    sm.total[sm.names()[c]] += x
                kept, removed = ref["survivors"], removed + ref["units_removed"]
            model.query(kept, thr)
            gt.query_prep(thr)
            c = world.varied(n, longs=())
            model.query(c, thr)
            gt.query_packed(*pack_reads(c), thr)
        check_counts(gt, model)
        check_counts(sgt, sm)
        assert sum(model.total.values()) > 0 and removed > 0
    finally:
        gt.close()
        sgt.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. what each call invalidates
# ---------------------------------------------------------------------------------------------------------------
def establish(gt, m, play):
    """A valid format_text state with scores, LCA, taxa and best rows of the last call all valid, and checked."""
    if m.nodes is None:
        tax = random_taxonomy(int(play.rng.integers(0, 1 << 30)), m.n_leaves)
        gt.set_taxonomy(*tax)
        m.set_taxonomy(tax)
    reads = play.w.screen_reads(40) if play.screen is not None and m is play.screen.m else play.w.reads(play.rng, True)
    data = mm.fc.fastq(reads[:len(reads) - len(reads) % 2])           # (an even block: it can also be queried as fragments)
    m.parse(data, True, None)
    gt.parse_text(data, "fastq")
    f = dict(hits=True, scores=True, lca="best", taxa=True, best=True)
    exp = m.classify(m.text["reads"], 0.7, **f)
    res = gt.query_text(0.7, **kw_of(f))
    assert np.array_equal(res[0], exp["offs"]) and np.array_equal(res[1], exp["leaves"])
    m.fmt_valid, m.fmt_rows = True, rows_of(exp["sets"])
    assert all(m.last[k] is not None for k in ("lca", "taxa", "best", "scores"))
    check_last(gt, m, "established")
    assert check_format(gt, m, 3, 7, "established") is not None


def test_what_each_call_invalidates(gpu):
    genomes, ids, ot, world, extra = mm.greedy_case(7)
    gt = greedy_tree(genomes, ids)
    m = TreeModel(ot)
    runner = Runner(gt)
    sgt, sm, screen_extra = greedy_screen_tree(world, 7)
    srunner = Runner(sgt)
    play = Play(m, world, 8400, gt, runner, extra, Side(sm, sgt, srunner, screen_extra))
    reads = world.reads(play.rng, True)
    seq, off = pack_reads(reads)

    def host():
        m.classify(reads, 1.0)
        gt.query_packed(seq, off, 1.0)

    def device():
        m.classify(reads, 1.0)
        d_seq, d_off, total = runner.device(seq, off, "streams")
        runner.last_stream = runner.streams[0]
        gt.query_device(d_seq, d_off, len(reads), total, 1.0, stream=runner.streams[0])
        stream_synchronize(runner.streams[0])

    def paired_text():
        assert len(m.text["reads"]) % 2 == 0 and len(m.text["reads"]) >= 2
        exp = m.classify(m.text["reads"], 0.7, paired="either", hits=True)   # a successful query_text with hits, and yet no format_text
        offs, leaves = gt.query_text(0.7, want_hits=True, paired=True)
        assert np.array_equal(offs, exp["offs"]) and np.array_equal(leaves, exp["leaves"]) and len(leaves) > 0

    def text_without_hits():
        m.classify(m.text["reads"], 1.0)
        gt.query_text(1.0)

    def prep_query():
        play.op_prep(None)
        check_format(gt, m, 3, 7, "prep_reads alone")                  # (the prep itself changes nothing)
        m.classify(m.prep["reads"], 1.0)
        gt.query_prep(1.0)

    def reset_counts():
        gt.reset_counts()
        m.reset()

    def deplete(paired):
        (play.op_prep_paired if paired else play.op_prep)(None)
        check_format(gt, m, 3, 7, "prep_reads before the depletion")
        play.op_deplete("either" if paired else "first")
        assert m.prep["last_deplete"][1] == ("either" if paired else None)

    def knob(name, value):
        gt.set_option(name, value)
        try:
            check_format(gt, m, 3, 7, (name, value))
        finally:
            gt.set_option(name, None)

    # (kind, the call, whether what the last call left stays readable, whether format_text stays valid), by pfq.h: a query call
    # ends both ("valid until the next query call on the tree", "text output"); a parse, an insertion and a prune end format_text
    # alone; everything else changes nothing
    kinds = [("host query", host, False, False), ("device query", device, False, False), ("paired text query", paired_text, False, False),
             ("text query without hits", text_without_hits, False, False), ("parse_text", lambda: play.op_parse(None), True, False),
             ("prep_reads", lambda: play.op_prep(None), True, True), ("paired prep_reads", lambda: play.op_prep_paired(None), True, True),
             ("query_prep", prep_query, False, False), ("query_frames", lambda: play.op_frames(None), False, False),
             ("query_frames_device", lambda: play.op_frames_dev(None), False, False), ("reset_counts", reset_counts, True, True),
             ("insert", lambda: play.op_insert(None), True, False), ("insert again", lambda: play.op_insert(None), True, False),
             ("prune_tree", lambda: play.op_prune(None), True, False),
             # a depletion is a query call on the screen alone: on the tree whose block it depletes everything stays
             ("prep_deplete", lambda: deplete(False), True, True), ("paired prep_deplete", lambda: deplete(True), True, True),
             ("set_mate_correct", lambda: play.op_set_mate_correct(None), True, True),
             # adapters and mate overlap do not depend on the leaves: insert and prune kept them
             ("prep_reads after insert and prune", lambda: play.op_prep(None), True, True),
             ("paired prep_reads after insert and prune", lambda: play.op_prep_paired(None), True, True),
             ("format_text", lambda: play.op_format(None), True, True), ("similarity", lambda: play.op_similarity(None), True, True),
             ("recluster", lambda: play.op_recluster(None), True, True), ("read-outs", lambda: play.op_readout(None), True, True),
             ("delta", lambda: play.op_delta(None), True, True)]
    kinds += [(f"{name}={value}", lambda name=name, value=value: knob(name, value), True, True) for name, value in mm.KNOBS]
    try:
        play.op_set_adapters("on")
        play.op_set_mate_overlap("on")
        for kind, call, last_stays, format_stays in kinds:
            establish(gt, m, play)
            before = dict(m.last)
            call()
            assert all((m.last[k] is before[k]) if last_stays else (m.last[k] is None) for k in before), kind
            assert m.fmt_valid == format_stays, kind
            runner.sync()
            check_last(gt, m, kind)
            check_format(gt, m, 3, 7, kind)
            check_accumulators(gt, m, kind)
        assert m.adapters is not None and m.overlap is not None and m.seen.get("adapter found") and m.seen.get("insert found")
        assert m.seen.get("unit removed", 0) >= 2

        # the same on the screen: a depletion ends everything there, a refused one nothing on either tree, and the screen's own
        # prep_reads, parse_text and reset_counts behave as on any tree
        block = world.screen_reads(30)

        def refused_deplete():
            play.op_prep(None)
            raises(PFQ_ERR_ARG, gt.prep_deplete, sgt, 0.7, paired=True)     # PFQ_PAIRED on an unpaired block

        def screen_prep():
            sm.prepare(block, None, False, {})
            assert sgt.prep_reads(*pack_reads(block))["n_kept"] == sm.prep["want"]["n_kept"]

        def screen_parse():
            data = mm.fc.fastq(block)
            sm.parse(data, True, None)
            sgt.parse_text(data, "fastq")

        def screen_reset():
            sgt.reset_counts()
            sm.reset()
        screen_kinds = [("prep_deplete", lambda: deplete(False), False, False), ("paired prep_deplete", lambda: deplete(True), False, False),
                        ("refused prep_deplete", refused_deplete, True, True), ("the screen's prep_reads", screen_prep, True, True),
                        ("the screen's parse_text", screen_parse, True, False), ("the screen's reset_counts", screen_reset, True, True)]
        for kind, call, last_stays, format_stays in screen_kinds:
            establish(gt, m, play)
            establish(sgt, sm, play)
            before, main_before = dict(sm.last), dict(m.last)
            call()
            assert all((sm.last[k] is before[k]) if last_stays else (sm.last[k] is None) for k in before), kind
            assert sm.fmt_valid == format_stays, kind
            assert all(m.last[k] is main_before[k] for k in main_before) and m.fmt_valid, kind      # the depleted tree: everything stays
            for side in (play.main, play.screen):
                side.runner.sync()
                check_last(side.gt, side.m, (kind, "screen table"))
                check_format(side.gt, side.m, 3, 7, (kind, "screen table"))
                check_accumulators(side.gt, side.m, (kind, "screen table"))
    finally:
        runner.close()
        srunner.close()
        gt.close()
        sgt.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. the accumulators across entry points and replicas
# ---------------------------------------------------------------------------------------------------------------
DEPLETE_THR = 0.7


def feed(gt, runner, entry, part, thr, f, paired=None, screen=None):
    """One part through one entry point with the flags f ("deplete": prepared, depleted against `screen`, then classified)."""
    if entry == "host":
        return gt.query_packed(*pack_reads(part), thr, **kw_of(f, paired))
    if entry == "streams":
        seq, off = pack_reads(part)
        d_seq, d_off, total = runner.device(seq, off, "streams")
        kw = kw_of(f, paired)
        kw.pop("want_hits")
        return gt.query_device_hits(d_seq, d_off, len(part), total, thr, stream=runner.streams[1], **kw)
    if entry == "text":
        gt.parse_text(wrap_fastq(part), "fastq")
        return gt.query_text(thr, **kw_of(f, paired))
    seq, off = pack_reads(part)
    kept = gt.prep_reads(seq, off, paired=paired is not None)
    assert kept["n_kept"] == len(part)                                 # (untrimmed parameters: every read is kept whole)
    if entry == "deplete":
        gt.prep_deplete(screen, DEPLETE_THR, paired=paired is not None, pair_mode=paired or "either")
    return gt.query_prep(thr, **kw_of(f, paired))


def test_accumulators_across_entry_points_and_replicas(balanced, tmp_path):
    """One read set in seven parts through the host, device-stream, text, prep, prep-and-deplete, paired-prep and
    paired-prep-and-deplete entry points of one tree, and in one call per kind of unit through a second tree loaded from the saved
    database, which receives the reference's survivors of the two depleted parts: every read-out is the same and the references',
    and the screen's counters are the reference's.  (The fragments of the paired parts make a call of their own there, and go
    without the sweep, which refuses fragments.)  Then the parts dealt over the two trees: absorbing and reducing gives the
    one-tree result."""
    genomes, ids, ot, world = balanced
    a = gpu_tree(genomes, ids, K, 131071, 7)
    db = str(tmp_path / "db")
    a.save(db)
    b = BloomTree.load(db)
    runner = Runner(a)
    sgt, sm = balanced_screen_tree(world)
    rng = np.random.default_rng(8500)
    parts = [world.reads(rng, True)[:50] for _ in range(4)] + [world.screen_reads(20) + world.reads(rng, True)[:30], world.pairs(20), world.pairs(20)]
    entries = ("host", "streams", "text", "prep", "deplete", "prep", "deplete")
    first_paired = 5

    def units_of(i, part, model):
        """What part i's query call classifies: the part, or the reference's survivors of its depletion (the screen's model grows)."""
        if entries[i] != "deplete":
            return part
        paired = i >= first_paired
        model.prepare(part, None, paired, {})
        ref = model.deplete(sm, DEPLETE_THR, "either" if paired else None)
        assert 0 < ref["units_removed"] < ref["n_units"], (i, ref["units_removed"])
        return ref["survivors"]
    tax = random_taxonomy(8501, len(ids))
    thr = 0.3
    pf = dict(ALL_ON, sweep=False)
    try:
        m = TreeModel(ot)
        for gt in (a, b):
            gt.set_taxonomy(*tax)
            gt.set_sweep(SWEEP)
        m.set_taxonomy(tax)
        m.set_sweep(SWEEP)
        units = []
        for i, (entry, part) in enumerate(zip(entries, parts)):
            paired = "either" if i >= first_paired else None
            units.append(units_of(i, part, m))
            exp = m.classify(units[i], thr, paired=paired, **(pf if paired else ALL_ON))
            res = feed(a, runner, entry, part, thr, pf if paired else ALL_ON, paired, sgt)
            assert np.array_equal(res[0], exp["offs"]) and np.array_equal(res[1], exp["leaves"]) and np.array_equal(np.asarray(res[2]).astype(np.int64), exp["scores"]), entry
            check_last(a, m, entry)
        whole = [r for u in units[:first_paired] for r in u]
        fragments = [r for u in units[first_paired:] for r in u]
        b.query_packed(*pack_reads(whole), thr, **kw_of(ALL_ON))
        b.query_packed(*pack_reads(fragments), thr, **kw_of(pf, "either"))
        check_accumulators(a, m, "seven entry points")
        check_accumulators(b, m, "one call per kind of unit")
        check_counts(sgt, sm)                                          # the screen's counters: the reference's, of both depletions
        assert sum(sm.total.values()) > 0
        assert m.log["n_ambiguous"] > 0 and m.sw["n_units"] == len(whole) and m.sketcher.sk.n_units == len(whole) + len(fragments) // 2
        # the parts dealt over two replicas
        for gt in (a, b):
            gt.reset_counts()
        m.reset()
        for i, (entry, part) in enumerate(zip(entries, parts)):
            paired = "either" if i >= first_paired else None
            m.classify(units[i], thr, paired=paired, **(pf if paired else ALL_ON))
            feed(b if i % 2 else a, runner, "host" if i % 2 else entry, units[i] if i % 2 else part, thr, pf if paired else ALL_ON, paired, sgt)
        a.abundance_absorb(b)
        a.coverage_absorb(b)
        a.sweep_absorb(b)
        allreduce_counts([a, b])
        check_counts(a, m)
        check_counts(b, m)
        mm.same_abundance(a.abundance(200, 0), abund_ref.estimate(m.log, 200, 0), "absorbed")
        mm.same_coverage(a.coverage(), m.sketcher, "absorbed")
        sweep_ref.same(a.sweep(), m.sweep_state(), "absorbed")
        assert b.abundance()["n_units"] == 0 and b.coverage()["n_units"] == 0 and b.sweep()["n_units"] == 0   # (moved, not copied)
    finally:
        runner.close()
        a.close()
        b.close()
        sgt.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. refused calls
# ---------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_no_accumulator_and_end_what_the_last_call_left(balanced):
    """The documented refusals of well-formed inputs, one after another, on a tree with every accumulator non-zero: query_text,
    query_prep and format_text before any parse / prep; taxa without a taxonomy; the sweep without a list, above the list's lowest
    threshold and of fragments; a paired query of a block prepared unpaired; scores without hits; rows that exceed PFQ_ABUND_SLOTS.
    The code is the documented one and every accumulator is what it was.  The refused depletions (before any prep, PFQ_PAIRED on an
    unpaired block, the screen being the tree itself, a flag other than the three allowed) are a kind of their own: no query call
    on either tree, so both trees' accumulators, last results and format_text are what they were.  Each of them but format_text is a query call that was
    refused, and pfq.h ("a query call") counts it as the next query call: what the call before it left and format_text are no
    longer valid.  The next good call is right."""
    genomes, ids, ot, world = balanced
    fresh = gpu_tree(genomes, ids, K, 131071, 7)
    sgt, sm = balanced_screen_tree(world)
    try:                                                               # before any parse / prep on a fresh tree
        raises(PFQ_ERR_STATE, fresh.query_text, 1.0)
        raises(PFQ_ERR_STATE, fresh.query_prep, 1.0)
        raises(PFQ_ERR_STATE, fresh.format_text)
        raises(PFQ_ERR_STATE, fresh.prep_deplete, sgt, 1.0)
        assert not any(c for _, c in fresh.get_leaf_counts()) and not any(c for _, c in sgt.get_leaf_counts())
    finally:
        fresh.close()
    gt = gpu_tree(genomes, ids, K, 131071, 7)
    m = TreeModel(ot)
    runner, srunner = Runner(gt), Runner(sgt)
    play = Play(m, world, 8600, gt, runner, screen=Side(sm, sgt, srunner))
    try:
        play.classify("host", world.screen_reads(40), "scores", side=play.screen)   # the screen's accumulators are not zero either
        assert sum(sm.total.values()) > 0
        gt.set_sweep(SWEEP)
        m.set_sweep(SWEEP)
        reads = world.reads(play.rng, True)
        m.classify(reads, 0.3, **dict(ALL_ON, taxa=False))
        gt.query_packed(*pack_reads(reads), 0.3, **kw_of(dict(ALL_ON, taxa=False)))
        done = set()

        def refuse_all():
            for name, code, call in play.refusals():
                if name in done:
                    continue
                done.add(name)
                establish(gt, m, play) if m.nodes is not None else None
                m.refused_query()
                raises(code, call, gt)
                runner.sync()
                check_accumulators(gt, m, name)
                check_last(gt, m, name)
                check_format(gt, m, 0, 7, name)
            for name, code, call in play.deplete_refusals():           # no query calls: nothing ends, on either tree
                if name in done:
                    continue
                done.add(name)
                establish(gt, m, play) if m.nodes is not None else None
                establish(sgt, sm, play)
                raises(code, call, gt, sgt)
                assert all(v is not None for v in sm.last.values()) and sm.fmt_valid
                play.check_both(name)
        refuse_all()                                                   # without a taxonomy
        assert "taxa without a taxonomy" in done
        play.op_set_taxonomy(None)
        m.classify(reads, 0.3, **ALL_ON)
        gt.query_packed(*pack_reads(reads), 0.3, **kw_of(ALL_ON))
        assert m.tax_here.any() and m.clade_here.any() and m.log["n_units"] and m.sketcher.sk.n_units and m.sw["n_units"] and sum(m.total.values())
        play.op_prep(None)
        refuse_all()                                                   # the rest, an unpaired prepared block among them
        gt.set_sweep([])
        m.set_sweep(None)
        refuse_all()                                                   # without a list
        assert done >= {"sweep without a list", "sweep above the list's lowest", "sweep of fragments", "paired query of an unpaired block", "scores without hits",
                        "depletion before any prep", "paired depletion of an unpaired block", "the screen is the tree itself",
                        "a depletion flag other than the three allowed"}
        # a call whose rows exceed PFQ_ABUND_SLOTS: every other result of the call stands, the log is incomplete until it is reset
        establish(gt, m, play)
        held = abund_ref.estimate(m.log, 200, 0)
        fam = [world.fam[0][i:i + 150] for i in range(0, 1500, 50)]
        seq, off = pack_reads(fam)
        exp = m.classify(fam, 0.7, hits=True, lca="all", abundance=True, log_fits=False)
        assert abund_ref.classify(rows_of(exp["sets"]), m.n_leaves)["n_entries"] > 1
        hits = _ffi.Hits()
        gt.set_option("PFQ_ABUND_SLOTS", 1)
        try:
            rc = _ffi.lib().pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, len(fam), 0.7,
                                            _ffi.WANT_HITS | _ffi.WANT_LCA | _ffi.WANT_ABUNDANCE, C.byref(hits))
            assert rc == PFQ_ERR_UNSUPPORTED and b"abundance log" in _ffi.lib().pfq_last_error()
            assert np.array_equal(np.ctypeslib.as_array(hits.offsets, shape=(len(fam) + 1,)), exp["offs"])
            assert np.array_equal(np.ctypeslib.as_array(hits.leaves, shape=(int(exp["offs"][-1]),)), exp["leaves"])
        finally:
            gt.set_option("PFQ_ABUND_SLOTS", None)
        m.log_ok = False
        check_last(gt, m, "abundance log full")
        check_accumulators(gt, m, "abundance log full")               # (the estimate is refused: PFQ_ERR_STATE)
        gt.abundance_reset()
        m.abundance_reset()
        assert held["n_units"] > 0
        check_accumulators(gt, m, "log reset")
        play.classify("host", reads, "hits")                           # the next good call is right
        play.op_readout(None)
    finally:
        runner.close()
        srunner.close()
        gt.close()
        sgt.close()
