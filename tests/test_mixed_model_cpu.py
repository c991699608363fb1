"""The model side of tests/test_gpu_mixed_sequences.py without a device: the deck of every seed the GPU test uses holds every
operation at least twice and every run of mixed_model.PAIRS, and the whole oracle-and-reference side runs over it with expectations
that are not vacuous — each condition of mixed_model.NOT_VACUOUS is met inside one sequence, judged from the references alone.  The
screen's model, the second tree of every deck, runs beside the main one."""
import os

import pytest

import mixed_model as mm

SEEDS = int(os.environ.get("PFQ_SEQUENCE_SEEDS", "2"))


@pytest.mark.parametrize("greedy", [False, True], ids=["balanced", "greedy"])
@pytest.mark.parametrize("seed", range(SEEDS))
def test_deck_holds_every_operation_twice_and_every_pair(seed, greedy):
    d = mm.deck((mm.GREEDY_SEED if greedy else mm.BALANCED_SEED) + seed, greedy)
    count, missing = mm.coverage_of(d)
    print(f"seed {seed} {'greedy' if greedy else 'balanced'}: {len(d)} operations", count, "missing pairs:", missing)
    assert not [op for op in mm.OPS if count[op] < 2], count           # the cap on what a seed may leave out: nothing
    assert not missing
    if greedy:
        ops = [e[0] for e in d]
        assert ops.count("insert") == 2 and ops.count("prune") == 2 and ops.index("prune") > len(d) * 3 // 4
        assert ops.count("screen_insert") == 1
        assert all(mm.has_run(d, run) for run in mm.GREEDY_RUNS)       # blocks older than either tree's leaves are queried and depleted
    else:
        assert "screen_insert" not in [e[0] for e in d]
    assert mm.has_run(d, [("parse", "even"), ("text", "paired"), ("format", None)])
    assert mm.deck(mm.BALANCED_SEED + seed) == mm.deck(mm.BALANCED_SEED + seed)   # a deck is a function of its seed


def run_model(model, world, seed, d, extra=(), screen=None):
    play = mm.Play(model, world, seed, extra=extra, screen=screen)
    play.run(d)
    print(f"seed {seed}: {len(d)} operations, the longest stretch of calls without a read: {play.most_unsynced}", dict(sorted(model.seen.items())))
    assert not [k for k in mm.NOT_VACUOUS if not model.seen.get(k)], model.seen
    run = mm.PAIRS["counts-only -> non-query -> counts-only"]      # ... with no read in between: neither call of the run was read
    at = [i for i in range(len(d) - 2) if all(d[i + j] == e for j, e in enumerate(run))]
    assert at and not any(i in play.read_steps or i + 2 in play.read_steps for i in at), (at, sorted(play.read_steps))
    assert play.most_unsynced >= 2                                       # stretches of several unsynchronised counts-only calls
    assert sum(model.total.values()) > 0


@pytest.mark.parametrize("seed", range(SEEDS))
def test_balanced_model_runs_the_deck_and_is_not_vacuous(seed):
    genomes, ids, ot, world = mm.balanced_case()
    screen = mm.TreeModel(mm.balanced_screen(world)[1])
    run_model(mm.TreeModel(ot), world, mm.BALANCED_SEED + seed, mm.deck(mm.BALANCED_SEED + seed), screen=mm.Side(screen))
    assert sum(screen.total.values()) > 0                               # the screen's counters grew, by its own queries and by the depletions


@pytest.mark.parametrize("seed", range(SEEDS))
def test_greedy_model_runs_the_deck_with_inserts_and_prune(seed):
    genomes, ids, ot, world, extra = mm.greedy_case(seed)
    model = mm.TreeModel(ot)
    before = model.n_leaves
    _, screen_ot, screen_extra = mm.greedy_screen(world, seed)
    screen = mm.TreeModel(screen_ot)
    leaves = screen.n_leaves
    run_model(model, world, mm.GREEDY_SEED + seed, mm.deck(mm.GREEDY_SEED + seed, greedy=True), extra, mm.Side(screen, extra=screen_extra))
    assert screen.n_leaves == leaves + 1                                # the screen grew by its spare genome
    assert 2 <= model.n_leaves < before + 2                             # grown by two, then pruned
    assert model.seen.get("parsed block queried after the leaves changed", 0) >= 3 and model.seen.get("prepared block queried after the leaves changed", 0) >= 3
