"""The slot contract of the position lists, on the numpy reference alone (tile_lists_ref.py): known bit patterns, a filter whose
length is no multiple of the tile, an all-zero tile, the cap on both sides."""
import numpy as np
import pytest

import tile_lists_ref as ref


def words_with(bits, n_words):
    w = np.zeros(n_words, dtype=np.uint64)
    for b in bits:
        w[b // 64] |= np.uint64(1) << np.uint64(b % 64)
    return w


def test_known_patterns_small_tiles():
    """Tiles of 2^8 bits: bit 0, a word's top bit, a tile's last bit, the first bit of the next tile."""
    bits = [0, 63, 64, 255, 256, 300, 767]
    w = words_with(bits, 12)                                   # 768 bits = 3 tiles
    assert ref.n_tiles(12, 8) == 3
    assert list(ref.tile_popcounts(w, 8)) == [4, 2, 1]
    assert list(ref.tile_positions(w, 0, 8)) == [0, 63, 64, 255]
    assert list(ref.tile_positions(w, 1, 8)) == [0, 44]
    assert list(ref.tile_positions(w, 2, 8)) == [255]
    slot = ref.make_slot(w, 1, cap=4, tile_log2=8)
    assert list(slot) == [0, 44, ref.TILE_LIST_NONE, ref.TILE_LIST_NONE]
    ref.check_slot(slot, w, 1, cap=4, tile_log2=8)
    ref.check_slot(slot[::-1].copy(), w, 1, cap=4, tile_log2=8)        # any order
    tile = ref.rebuild_tile(slot, 8)
    assert tile.shape == (8,) and tile[0] == 1 and tile[1] == 1 << 12 and not tile[2:].any()


def test_partial_last_tile_and_empty_tile():
    """2^9 + 64 bits at tiles of 2^8: the third tile has one word; the second is all zero."""
    w = words_with([3, 200, 512, 575], 9)
    assert ref.n_tiles(9, 8) == 3
    assert list(ref.tile_popcounts(w, 8)) == [2, 0, 2]
    assert list(ref.tile_positions(w, 2, 8)) == [0, 63]
    empty = ref.make_slot(w, 1, cap=8, tile_log2=8)
    assert (empty == ref.TILE_LIST_NONE).all()
    ref.check_slot(empty, w, 1, cap=8, tile_log2=8)
    assert not ref.rebuild_tile(empty, 8).any()
    ref.check_slot(ref.make_slot(w, 2, cap=8, tile_log2=8), w, 2, cap=8, tile_log2=8)


def test_cap_decides_per_column():
    w = words_with(range(0, 256, 2), 8)                        # 128 bits in tile 0, none in tile 1
    assert ref.is_sparse(w, cap=128, tile_log2=8)
    assert not ref.is_sparse(w, cap=127, tile_log2=8)
    with pytest.raises(ValueError):
        ref.make_slot(w, 0, cap=127, tile_log2=8)
    full = ref.make_slot(w, 0, cap=128, tile_log2=8)           # a slot without padding
    assert (full != ref.TILE_LIST_NONE).all()
    ref.check_slot(full, w, 0, cap=128, tile_log2=8)


def test_check_slot_rejects_wrong_slots():
    w = words_with([1, 2, 3], 4)
    good = ref.make_slot(w, 0, cap=8, tile_log2=8)
    for bad in (np.array([1, 2] + [ref.TILE_LIST_NONE] * 6, dtype=np.uint32),          # a bit missing
                np.array([1, 2, 3, 3] + [ref.TILE_LIST_NONE] * 4, dtype=np.uint32),    # listed twice
                np.array([1, 2, 4] + [ref.TILE_LIST_NONE] * 5, dtype=np.uint32),       # a bit that is not set
                good[:7]):                                                             # short
        with pytest.raises(AssertionError):
            ref.check_slot(bad, w, 0, cap=8, tile_log2=8)


def test_rebuild_equals_dense_tile_at_real_size():
    """Random 0.7 % fill at the real tile size, 2^21 + 12345 bits: every rebuilt tile equals the filter's own words."""
    rng = np.random.default_rng(7)
    nbits = (1 << 21) + 12345
    n_words = (nbits + 63) // 64
    w = words_with(rng.integers(0, nbits, 15000).tolist(), n_words)
    assert ref.n_tiles(n_words) == 3 and ref.is_sparse(w)
    w32 = np.concatenate([w.view(np.uint32), np.zeros(3 * (1 << 15) - 2 * n_words, dtype=np.uint32)])
    for t in range(3):
        slot = ref.make_slot(w, t)
        ref.check_slot(slot, w, t)
        assert np.array_equal(ref.rebuild_tile(slot), w32[t << 15:(t + 1) << 15]), t
