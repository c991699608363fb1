"""tests/frames_ref.py on hand-made cases: the frame starts at every length where the rule changes, the run fields on literal
match masks, and the partial results as a monoid (a mask split anywhere and joined gives the whole)."""
import itertools

import pytest

import frames_ref as fr

K = 21


def test_frame_starts_by_hand():
    F, S = 100, 30
    assert fr.frame_starts(0, F, S) == [(0, 0)]
    assert fr.frame_starts(K - 1, F, S) == [(0, K - 1)]
    assert fr.frame_starts(K, F, S) == [(0, K)]
    assert fr.frame_starts(F - 1, F, S) == [(0, 99)]
    assert fr.frame_starts(F, F, S) == [(0, 100)]
    assert fr.frame_starts(F + 1, F, S) == [(0, 100), (1, 100)]                      # the last frame is flush with the end
    assert fr.frame_starts(F + S, F, S) == [(0, 100), (30, 100)]
    assert fr.frame_starts(F + S + 1, F, S) == [(0, 100), (30, 100), (31, 100)]
    assert fr.frame_starts(F + 3 * S, F, S) == [(0, 100), (30, 100), (60, 100), (90, 100)]           # a multiple of S beyond F
    assert fr.frame_starts(F + 3 * S + 7, F, S) == [(0, 100), (30, 100), (60, 100), (90, 100), (97, 100)]  # and not one


@pytest.mark.parametrize("F,S", [(100, 30), (84, 84), (85, 17), (21, 1), (301, 7), (5, 5)])
def test_frame_starts_properties(F, S):
    for L in list(range(0, 3 * F + 2 * S + 3)) + [10 * F + 1]:
        frames = fr.frame_starts(L, F, S)
        if L <= F:
            assert frames == [(0, L)]
            continue
        assert len(frames) == -(-(L - F) // S) + 1
        assert frames[0] == (0, F) and frames[-1] == (L - F, F) and all(n == F for _, n in frames)
        starts = [s for s, _ in frames]
        assert all(0 < b - a <= S for a, b in zip(starts, starts[1:]))           # no gap wider than S, no frame twice
        assert all(b - a == S for a, b in zip(starts[:-2], starts[1:-1]))


def bits(text):
    return [c == "1" for c in text]


def test_run_fields_on_literal_masks():
    assert fr.run_fields([]) == (0, None, None, 0)
    assert fr.run_fields(bits("0000")) == (0, None, None, 0)
    assert fr.run_fields(bits("1111")) == (4, 0, 3, 4)
    assert fr.run_fields(bits("0110100")) == (3, 1, 4, 2)
    assert fr.run_fields(bits("1000001")) == (2, 0, 6, 1)
    assert fr.run_fields(bits("0011101111")) == (7, 2, 9, 4)
    assert fr.part(bits("1101011")) == (7, 5, 0, 6, 2, 2, 2)
    assert fr.part(bits("111")) == (3, 3, 0, 2, 3, 3, 3)
    assert fr.part(bits("000")) == (3, 0, None, None, 0, 0, 0)
    assert fr.part([]) == (0, 0, None, None, 0, 0, 0)


def test_join_is_the_whole_at_every_split():
    masks = [bits(t) for t in ("", "0", "1", "0110100", "1111111", "0000000", "1101011", "0011101111", "1" * 70 + "0" + "1" * 64)]
    masks += [list(m) for m in itertools.product([False, True], repeat=6)]
    for m in masks:
        whole = fr.part(m)
        for cut in range(len(m) + 1):
            assert fr.join(fr.part(m[:cut]), fr.part(m[cut:])) == whole, (m, cut)
    m = bits("0011101111" * 20)                                                    # three pieces of uneven length, both groupings
    a, b, c = fr.part(m[:64]), fr.part(m[64:67]), fr.part(m[67:])
    assert fr.join(fr.join(a, b), c) == fr.join(a, fr.join(b, c)) == fr.part(m)
    assert fr.join(fr.part([]), a) == a == fr.join(a, fr.part([]))               # the empty stretch is the unit
