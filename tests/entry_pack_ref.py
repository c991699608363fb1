"""The packed entry format of the LDS-tile passes at theta = 1, restated in numpy.

A 16-byte vector (four little-endian u32 words) holds five 24-bit entries and an 8-bit tag:

  entry j       bits 24 j .. 24 j + 23  = [pair of the round : 4][offset in tile : 20]
  tag           bits 120 .. 127         = number of the k_tile_bin round the run belongs to (rho & 255)

A run is the entries of one (round, tile); it is padded to a whole vector with copies of its last entry."""
import numpy as np

ENTRY_BITS, OFFSET_BITS, ID_BITS, TAG_BITS, PER_VECTOR = 24, 20, 4, 8, 5
PACK_PAIRS, PACK_ROUNDS = 1 << ID_BITS, 1 << TAG_BITS


def entry(pair_id, offset):
    assert 0 <= pair_id < PACK_PAIRS and 0 <= offset < (1 << OFFSET_BITS)
    return (pair_id << OFFSET_BITS) | offset


def pack_run(entries, rho):
    """The u32 words of one run: ceil(len / 5) vectors of four words."""
    e = [int(x) for x in entries]
    assert e and all(0 <= x < (1 << ENTRY_BITS) for x in e)
    e += [e[-1]] * (-len(e) % PER_VECTOR)
    e = np.array(e, dtype=np.uint64).reshape(-1, PER_VECTOR)
    tag = np.uint64(rho & (PACK_ROUNDS - 1))
    m32 = np.uint64(0xFFFFFFFF)
    w = np.empty((len(e), 4), dtype=np.uint64)
    w[:, 0] = (e[:, 0] | (e[:, 1] << np.uint64(24))) & m32
    w[:, 1] = ((e[:, 1] >> np.uint64(8)) | (e[:, 2] << np.uint64(16))) & m32
    w[:, 2] = ((e[:, 2] >> np.uint64(16)) | (e[:, 3] << np.uint64(8))) & m32
    w[:, 3] = e[:, 4] | (tag << np.uint64(24))
    return w.astype(np.uint32).reshape(-1)


def unpack(words):
    """(entries [vectors, 5], tags [vectors]) of a bucket's words (a multiple of four)."""
    w = np.asarray(words, dtype=np.uint32).astype(np.uint64).reshape(-1, 4)
    m24 = np.uint64(0xFFFFFF)
    e = np.empty((len(w), PER_VECTOR), dtype=np.int64)
    e[:, 0] = w[:, 0] & m24
    e[:, 1] = ((w[:, 0] >> np.uint64(24)) | (w[:, 1] << np.uint64(8))) & m24
    e[:, 2] = ((w[:, 1] >> np.uint64(16)) | (w[:, 2] << np.uint64(16))) & m24
    e[:, 3] = w[:, 2] >> np.uint64(8)
    e[:, 4] = w[:, 3] & m24
    return e, (w[:, 3] >> np.uint64(24)).astype(np.int64)


def split(entries):
    """(pair of the round, offset in tile) of entries."""
    entries = np.asarray(entries)
    return entries >> OFFSET_BITS, entries & ((1 << OFFSET_BITS) - 1)


def bit_string(words):
    """The vectors as integers of 128 bits (word 0 lowest): the brute-force reading of the format."""
    w = [int(x) for x in np.asarray(words, dtype=np.uint32)]
    assert len(w) % 4 == 0
    return [w[i] | (w[i + 1] << 32) | (w[i + 2] << 64) | (w[i + 3] << 96) for i in range(0, len(w), 4)]
