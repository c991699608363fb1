"""The numpy restatement of the packed entry format (entry_pack_ref) against a brute-force reading of the vectors as
128-bit strings: run lengths 1..11, ids 0 and 15, offsets 0 and 2^20 - 1, rounds 0 and 255."""
import itertools

import numpy as np
import pytest

import entry_pack_ref as ref

RNG = np.random.default_rng(20261019)
EDGE_IDS, EDGE_OFFSETS, EDGE_ROUNDS = (0, 15), (0, (1 << 20) - 1), (0, 255)


def brute_entries(vec):
    return [(vec >> (24 * j)) & 0xFFFFFF for j in range(5)], vec >> 120


def runs():
    """(entries, round) of every run length 1..11: all edge entries cycled through every position, and random ones."""
    edge = [ref.entry(i, o) for i, o in itertools.product(EDGE_IDS, EDGE_OFFSETS)]
    for n in range(1, 12):
        for rho in EDGE_ROUNDS + (int(RNG.integers(1, 255)),):
            for shift in range(len(edge)):
                yield [edge[(shift + j) % len(edge)] for j in range(n)], rho
            yield [ref.entry(int(RNG.integers(0, 16)), int(RNG.integers(0, 1 << 20))) for _ in range(n)], rho


@pytest.mark.parametrize("n", range(1, 12))
def test_pack_against_bit_strings(n):
    seen = 0
    for entries, rho in runs():
        if len(entries) != n:
            continue
        seen += 1
        words = ref.pack_run(entries, rho)
        n_vec = (n + 4) // 5
        assert words.dtype == np.uint32 and len(words) == 4 * n_vec
        padded = entries + [entries[-1]] * (5 * n_vec - n)
        for v, vec in enumerate(ref.bit_string(words)):
            got, tag = brute_entries(vec)
            assert got == padded[5 * v:5 * v + 5] and tag == rho, (entries, rho, v)
            assert 0 <= vec < 1 << 128
    assert seen >= 15


@pytest.mark.parametrize("n", range(1, 12))
def test_unpack_inverts_pack(n):
    for entries, rho in runs():
        if len(entries) != n:
            continue
        e, tags = ref.unpack(ref.pack_run(entries, rho))
        flat = e.reshape(-1)
        assert flat[:n].tolist() == entries and (flat[n:] == entries[-1]).all() and len(flat) - n < 5
        assert (tags == rho).all()
        ids, offs = ref.split(flat[:n])
        assert [ref.entry(int(i), int(o)) for i, o in zip(ids, offs)] == entries


def test_edges_in_every_position():
    """ids 0 / 15, offsets 0 / 2^20 - 1 and rounds 0 / 255 in each of the five places of a vector; all ones is a legal entry."""
    for j, i, o, rho in itertools.product(range(5), EDGE_IDS, EDGE_OFFSETS, EDGE_ROUNDS):
        other = ref.entry(15 - i, (1 << 20) - 1 - o)
        entries = [other] * 5
        entries[j] = ref.entry(i, o)
        vec, = ref.bit_string(ref.pack_run(entries, rho))
        got, tag = brute_entries(vec)
        assert got == entries and tag == rho
    assert ref.entry(15, (1 << 20) - 1) == 0xFFFFFF


def test_concatenated_runs():
    """A bucket is runs back to back: the tags tell them apart, the padding stays inside its run."""
    lens, words, want = [3, 5, 11, 1, 7], [], []
    for r, n in enumerate(lens):
        entries = [ref.entry(int(RNG.integers(0, 16)), int(RNG.integers(0, 1 << 20))) for _ in range(n)]
        words.append(ref.pack_run(entries, 254 + r))
        want.append(entries)
    e, tags = ref.unpack(np.concatenate(words))
    at = 0
    for r, n in enumerate(lens):
        nv = (n + 4) // 5
        assert (tags[at:at + nv] == ((254 + r) & 255)).all()
        flat = e[at:at + nv].reshape(-1)
        assert flat[:n].tolist() == want[r] and (flat[n:] == want[r][-1]).all()
        at += nv
    assert at == len(tags)
