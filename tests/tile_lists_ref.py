"""numpy reference of the position slots of sparse filter tiles (pfq_tilelist.hip).

A filter is its Lsb0 u64 words (bit i = word i // 64, bit i % 64), cut into tiles of 2^TILE_LOG2 bits; the last tile may be
partial.  A column whose tiles all hold at most TILE_LIST_CAP set bits keeps one slot per tile: the tile-relative positions of
the set bits in any order, padded with TILE_LIST_NONE to TILE_LIST_CAP entries."""
import numpy as np

TILE_LOG2 = 20
TILE_LIST_CAP = 8192
TILE_LIST_NONE = 0xFFFFFFFF


def n_tiles(n_words, tile_log2=TILE_LOG2):
    return (int(n_words) * 64 + (1 << tile_log2) - 1) >> tile_log2


def filter_bits(words):
    """One 0/1 byte per bit of the words, bit 0 of word 0 first."""
    w = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(w.view(np.uint8), bitorder="little")


def tile_popcounts(words, tile_log2=TILE_LOG2):
    """Set bits of every tile."""
    bits = filter_bits(words)
    nt = n_tiles(len(words), tile_log2)
    return np.array([int(bits[t << tile_log2:(t + 1) << tile_log2].sum()) for t in range(nt)], dtype=np.int64)


def tile_positions(words, tile, tile_log2=TILE_LOG2):
    """Ascending tile-relative positions of the set bits of one tile."""
    bits = filter_bits(words)
    return np.flatnonzero(bits[tile << tile_log2:(tile + 1) << tile_log2]).astype(np.uint32)


def is_sparse(words, cap=TILE_LIST_CAP, tile_log2=TILE_LOG2):
    """The column gets slots: every tile within the cap."""
    return bool((tile_popcounts(words, tile_log2) <= cap).all())


def make_slot(words, tile, cap=TILE_LIST_CAP, tile_log2=TILE_LOG2):
    """A slot as the contract allows it (here: ascending positions, then the padding)."""
    pos = tile_positions(words, tile, tile_log2)
    if len(pos) > cap:
        raise ValueError(f"tile {tile} holds {len(pos)} set bits, more than a slot's {cap}")
    out = np.full(cap, TILE_LIST_NONE, dtype=np.uint32)
    out[:len(pos)] = pos
    return out


def check_slot(slot, words, tile, cap=TILE_LIST_CAP, tile_log2=TILE_LOG2):
    """Raises AssertionError unless `slot` is a valid slot of the tile: cap entries, every set bit listed exactly once, in any
    order, everything else TILE_LIST_NONE."""
    slot = np.asarray(slot)
    assert slot.shape == (cap,), slot.shape
    listed = slot[slot != TILE_LIST_NONE]
    want = tile_positions(words, tile, tile_log2)
    assert len(listed) == len(want), (tile, len(listed), len(want))
    assert np.array_equal(np.sort(listed), want), tile


def rebuild_tile(slot, tile_log2=TILE_LOG2):
    """What k_tile_test makes of a slot: the tile's u32 words with exactly the listed bits set."""
    out = np.zeros(1 << (tile_log2 - 5), dtype=np.uint32)
    listed = np.asarray(slot)[np.asarray(slot) != TILE_LIST_NONE].astype(np.int64)
    np.bitwise_or.at(out, listed >> 5, (np.uint32(1) << (listed & 31).astype(np.uint32)))
    return out
