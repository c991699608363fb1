"""Host-side mirror of the reference's query interface over libpfq.

Names follow the reference: `BloomTree.load` (bloom_tree.rs:364-386), `prune_tree` (:302-330),
`query_batch` (query.rs:66-82), `get_leaf_counts` / `save_leaf_counts` (query.rs:173-218), `ResultMap`
(result_map.rs:9-46).  All filter work happens in the HIP kernels of libpfq; nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

from . import _ffi


class ResultMap:
    """result_map.rs:9-46 — read id -> set of genome ids for the current block."""

    def __init__(self) -> None:
        self.read_map: Dict[str, Set[str]] = {}

    def add_read_map(self, read_id: str, genome_id: str) -> None:
        self.read_map.setdefault(read_id, set()).add(genome_id)

    def get_ext_id(self, read_id: str) -> str:  # "{id} |{g1,g2}" (set order is unspecified in the reference too)
        return f"{read_id} |{','.join(self.read_map.get(read_id, ()))}"

    def read_mapped(self, read_id: str) -> bool:
        return read_id in self.read_map

    def empty_read_map(self) -> None:
        self.read_map.clear()


# one pfq_segment (include/pfq.h)
SEGMENT_DTYPE = np.dtype([(f, np.uint32) for f in ("leaf", "first_frame", "n_frames", "begin", "end", "match_begin", "match_end", "kmers",
                                                   "matched", "longest_run")])


# one pfq_merge (include/pfq.h)
MERGE_DTYPE = np.dtype([("node", np.uint32), ("left", np.uint32), ("right", np.uint32), ("round", np.uint32), ("n_leaves", np.uint32),
                        ("pad_", np.uint32), ("score_sum", np.uint64), ("pairs", np.uint64)])


def pack_reads(reads: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    seq = np.frombuffer(b"".join(reads) + b"\0" * 16, dtype=np.uint8).copy()
    return seq, off


class BloomTree:
    """A Sequence Bloom Tree resident in HBM (BloomTree, bloom_tree.rs:29-48)."""

    def __init__(self, handle: C.c_void_p, device: int):
        self._h = handle
        self.device = device
        self.last_n_frames = 0  # frames the last query_frames call classified

    # ---- construction
    @classmethod
    def load(cls, directory: str, device: int = 0) -> "BloomTree":
        h = C.c_void_p()
        _ffi.check(_ffi.lib().pfq_tree_open(directory.encode(), device, C.byref(h)))
        return cls(h, device)

    @classmethod
    def load_subtree(cls, directory: str, depth: int, index: int, device: int = 0) -> "BloomTree":
        """Shard `index` of the depth-`depth` frontier (pfq_tree_open_subtree): that node, its subtree and its
        ancestor chain.  For trees that do not fit one GPU: one shard per rank, every rank sees all reads."""
        h = C.c_void_p()
        _ffi.check(_ffi.lib().pfq_tree_open_subtree(directory.encode(), device, depth, index, C.byref(h)))
        return cls(h, device)

    @staticmethod
    def shard_count(directory: str, depth: int) -> int:
        """Number of subtree shards at depth `depth` (pfq_db_shard_count): the indices load_subtree accepts are
        0 .. shard_count - 1.  Reads tree.bin only; needs no device."""
        n = C.c_uint64()
        _ffi.check(_ffi.lib().pfq_db_shard_count(directory.encode(), depth, C.byref(n)))
        return n.value

    @classmethod
    def new(cls, kmer_size: int, false_pos_rate: float, largest_expected_genome: int, seed1: int, seed2: int,
            expected_genomes: int = 0, device: int = 0) -> "BloomTree":
        """BloomTree::new (bloom_tree.rs:100-118) with explicit hash seeds; fill it with insert()."""
        h = C.c_void_p()
        _ffi.check(_ffi.lib().pfq_tree_create(kmer_size, false_pos_rate, largest_expected_genome, seed1, seed2,
                                              expected_genomes, device, C.byref(h)))
        return cls(h, device)

    def insert(self, genome: bytes, tax_id: str, internal_name: Optional[str] = None) -> None:
        """BloomTree::insert (bloom_tree.rs:128-143): greedy placement by Hamming distance, on the device."""
        buf = np.frombuffer(genome, dtype=np.uint8) if len(genome) else np.zeros(1, dtype=np.uint8)
        _ffi.check(_ffi.lib().pfq_tree_insert(self._h, buf.ctypes.data, len(genome), tax_id.encode(),
                                              internal_name.encode() if internal_name is not None else None))

    @classmethod
    def build_balanced(cls, genomes: Sequence[bytes], tax_ids: Sequence[str], kmer_size: int, nbits: int,
                       num_hashes: int, seed1: int, seed2: int, false_pos_rate: float = 0.001,
                       largest_expected_genome: int = 1000000, device: int = 0) -> "BloomTree":
        seq, off = pack_reads(genomes)
        ids = (C.c_char_p * max(len(tax_ids), 1))(*[t.encode() for t in tax_ids])
        h = C.c_void_p()
        _ffi.check(_ffi.lib().pfq_tree_build_balanced(seq.ctypes.data, off.ctypes.data, len(genomes), ids, kmer_size,
                                                      nbits, num_hashes, seed1, seed2, false_pos_rate,
                                                      largest_expected_genome, device, C.byref(h)))
        return cls(h, device)

    @classmethod
    def build_balanced_device(cls, d_genomes: int, genome_len: int, n_genomes: int, tax_ids: Sequence[str],
                              kmer_size: int, nbits: int, num_hashes: int, seed1: int, seed2: int,
                              false_pos_rate: float = 0.001, largest_expected_genome: int = 1000000,
                              device: int = 0) -> "BloomTree":
        ids = (C.c_char_p * max(len(tax_ids), 1))(*[t.encode() for t in tax_ids])
        h = C.c_void_p()
        _ffi.check(_ffi.lib().pfq_tree_build_balanced_device(d_genomes, genome_len, n_genomes, ids, kmer_size, nbits,
                                                             num_hashes, seed1, seed2, false_pos_rate,
                                                             largest_expected_genome, device, C.byref(h)))
        return cls(h, device)

    @classmethod
    def build_balanced_subtree_device(cls, d_genomes: int, genome_len: int, n_genomes: int, tax_ids: Sequence[str],
                                      kmer_size: int, nbits: int, num_hashes: int, seed1: int, seed2: int, depth: int,
                                      index: int, false_pos_rate: float = 0.001, largest_expected_genome: int = 1000000,
                                      device: int = 0) -> "BloomTree":
        """Subtree shard `index` of the depth-`depth` frontier of the balanced tree over all `n_genomes` genomes
        (BASELINE config 5), built without the rest of the tree."""
        ids = (C.c_char_p * max(len(tax_ids), 1))(*[t.encode() for t in tax_ids])
        h = C.c_void_p()
        _ffi.check(_ffi.lib().pfq_tree_build_balanced_subtree_device(d_genomes, genome_len, n_genomes, ids, kmer_size,
                                                                     nbits, num_hashes, seed1, seed2, false_pos_rate,
                                                                     largest_expected_genome, depth, index, device,
                                                                     C.byref(h)))
        return cls(h, device)

    def close(self) -> None:
        if self._h:
            _ffi.lib().pfq_tree_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference surface
    def save(self, directory: str) -> None:
        import os
        os.makedirs(directory, exist_ok=True)
        _ffi.check(_ffi.lib().pfq_tree_save(self._h, directory.encode()))

    def prune_tree(self, search_depth: int) -> None:
        _ffi.check(_ffi.lib().pfq_tree_prune(self._h, search_depth))

    def info(self) -> _ffi.Info:
        i = _ffi.Info()
        _ffi.check(_ffi.lib().pfq_tree_info(self._h, C.byref(i)))
        return i

    @property
    def kmer_size(self) -> int:
        return int(self.info().kmer_size)

    def get_leaf_counts(self) -> List[Tuple[str, int]]:
        ids = C.POINTER(C.c_char_p)()
        cnt = C.POINTER(C.c_uint64)()
        n = C.c_uint64()
        _ffi.check(_ffi.lib().pfq_leaf_counts(self._h, C.byref(ids), C.byref(cnt), C.byref(n)))
        return [(ids[i].decode(), int(cnt[i])) for i in range(n.value)]

    def save_leaf_counts(self, path: str) -> None:
        _ffi.check(_ffi.lib().pfq_save_leaf_counts(self._h, path.encode()))

    def reset_counts(self) -> None:
        _ffi.check(_ffi.lib().pfq_leaf_counts_reset(self._h))

    # ---- measurement / test hooks
    def set_option(self, name: str, value: Optional[str]) -> None:
        """One tuning / test knob of this tree; None = the built-in choice."""
        _ffi.check(_ffi.lib().pfq_set_option(self._h, name.encode(), None if value is None else str(value).encode()))

    def set_path(self, path: int) -> None:
        _ffi.check(_ffi.lib().pfq_set_path(self._h, path))

    def last_stats(self) -> _ffi.Stats:
        s = _ffi.Stats()
        _ffi.check(_ffi.lib().pfq_last_stats(self._h, C.byref(s)))
        return s

    CAPACITY_FIELDS = ("pair_cursor", "pair_cap", "guard_cursor", "guard_cap", "miss_cursor", "miss_cap", "kmiss_used",
                       "kmiss_cap", "hit_cursor", "hit_cap", "attempts", "pairs_sorted")

    def last_capacity(self) -> dict:
        """Scratch capacities of the last query call and how far its kernels got into them (pfq_debug_last_capacity):
        a cursor above its cap means that buffer overflowed and the rest was certified inline; `hit_cursor` / `hit_cap`
        are the first attempt's, `attempts` is 2 when the hit buffer overflowed and the block ran again."""
        out = np.zeros(len(self.CAPACITY_FIELDS), dtype=np.uint64)
        _ffi.check(_ffi.lib().pfq_debug_last_capacity(self._h, out.ctypes.data, out.size))
        return {k: int(v) for k, v in zip(self.CAPACITY_FIELDS, out)}

    TILE_LIST_CAP = 8192
    TILE_LIST_NONE = 0xFFFFFFFF

    def tile_lists_info(self) -> dict:
        """Position slots of the sparse columns (pfq_tile_lists_info): `columns` that have them, the `bytes` they hold, and
        how many tiles k_tile_test<0> of the last query call built from slots (`list_tiles`) and loaded (`dense_tiles`)."""
        out = np.zeros(4, dtype=np.uint64)
        _ffi.check(_ffi.lib().pfq_tile_lists_info(self._h, out.ctypes.data))
        return {k: int(v) for k, v in zip(("columns", "bytes", "list_tiles", "dense_tiles"), out)}

    def screen_info(self) -> dict:
        """The dense screen at theta = 1 (pfq_screen_info): `kmers` a read the last query call's screen took (2: the lean build,
        4, 0: no such screen), the tree's `E` (expected false candidates a random read after four rows), `rw` and `groups`."""
        out = np.zeros(4, dtype=np.float64)
        _ffi.check(_ffi.lib().pfq_screen_info(self._h, out.ctypes.data))
        return {"kmers": int(out[0]), "E": float(out[1]), "rw": int(out[2]), "groups": int(out[3])}

    def pair_info(self) -> tuple:
        """The pair slots of the last query call's classify launches (pfq_pair_info): [1] the reservations a batched emission
        asks for beyond its pass (PFQ_PAIR_AHEAD as used; 0: no such emission ran), [2] the reservations the launches made;
        [0] and [3] are 0 (no kernel counts the buckets from the pair buffer)."""
        out = np.zeros(4, dtype=np.uint64)
        _ffi.check(_ffi.lib().pfq_pair_info(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def tile_list(self, col: int, tile: int) -> np.ndarray:
        """One slot (pfq_debug_tile_list): TILE_LIST_CAP u32, the tile-relative positions of the tile's set bits in any order,
        then TILE_LIST_NONE.  Raises PfqError for a column without slots."""
        out = np.zeros(self.TILE_LIST_CAP, dtype=np.uint32)
        _ffi.check(_ffi.lib().pfq_debug_tile_list(self._h, col, tile, out.ctypes.data, out.size))
        return out

    TILE_BUCKET_WORDS = 1296

    def tile_bucket(self, chunk: int, tile: int, max_words: int = 1 << 20) -> dict:
        """One probe bucket of the last call's LDS-tile passes at theta = 1 (pfq_debug_tile_bucket): the fill mark and
        capacity in 32-bit words, the chunk's `first` pair, pair count `n`, column `leaf` and `pass`, whether the entries are
        `packed`, the call's `n_chunks`, with packed entries the chunk's `n_rounds` and the first pair of each (`round_p0`),
        the read of each of the chunk's pairs (`reads`) and the bucket's `words`."""
        out = np.zeros(self.TILE_BUCKET_WORDS + max_words, dtype=np.uint32)
        _ffi.check(_ffi.lib().pfq_debug_tile_bucket(self._h, chunk, tile, out.ctypes.data, out.size))
        fill, cap, first, n, leaf, pas, packed, n_chunks, n_rounds = (int(v) for v in out[:9])
        return dict(fill=fill, cap=cap, first=first, n=n, leaf=leaf, **{"pass": pas}, packed=bool(packed), n_chunks=n_chunks, n_rounds=n_rounds,
                    round_p0=out[16:16 + n_rounds].astype(np.int64), reads=out[272:272 + n].astype(np.int64),
                    words=out[self.TILE_BUCKET_WORDS:self.TILE_BUCKET_WORDS + min(fill, cap, max_words)].copy())

    def profile_begin(self, max_calls: int) -> None:
        _ffi.check(_ffi.lib().pfq_profile_begin(self._h, max_calls))

    def profile_end(self) -> _ffi.Profile:
        p = _ffi.Profile()
        _ffi.check(_ffi.lib().pfq_profile_end(self._h, C.byref(p)))
        return p

    def kmer_indices(self, seq: bytes) -> np.ndarray:
        n = C.c_uint64()
        buf = np.frombuffer(seq + b"\0", dtype=np.uint8).copy()
        _ffi.check(_ffi.lib().pfq_debug_kmer_indices(self._h, buf.ctypes.data, len(seq), None, C.byref(n)))
        out = np.zeros((n.value, int(self.info().num_hashes)), dtype=np.uint64)
        if n.value:
            _ffi.check(_ffi.lib().pfq_debug_kmer_indices(self._h, buf.ctypes.data, len(seq), out.ctypes.data, C.byref(n)))
        return out

    def node_filter(self, node: int) -> np.ndarray:
        i = self.info()
        out = np.zeros((int(i.nbits) + 63) // 64, dtype=np.uint64)
        _ffi.check(_ffi.lib().pfq_debug_node_filter(self._h, node, out.ctypes.data, out.size))
        return out

    # ---- query
    def query_packed(self, seq: np.ndarray, off: np.ndarray, threshold: float, want_hits: bool = False,
                     want_scores: bool = False, paired: bool = False, pair_mode: str = "either",
                     lca: Optional[str] = None, abundance: bool = False, coverage: bool = False, taxa: bool = False,
                     best: bool = False, sweep: bool = False):
        """One block of reads from host memory.  Returns None, the (offsets, leaves) CSR, or with `want_scores`
        (offsets, leaves, scores): scores[j] = how many of the read's k-mers leaf leaves[j] contains (pfq_last_hit_scores).
        `paired`: reads 2i and 2i + 1 are mates (PFQ_PAIRED); rows, counts and scores are per fragment, whose set is the union
        (pair_mode "either") or the intersection ("both") of the mates' sets.
        `lca`: "all" also assigns every read / fragment to the lowest common ancestor of its hit leaves (last_lca(),
        clade_counts()), "best" to that of its best-scoring hits (needs want_hits and want_scores); the return value and
        every other result stay what they are without it.
        `abundance`: the call's rows are also logged on the device for abundance() (needs want_hits).
        `coverage`: every listed genome's matched k-mers are also sketched on the device for coverage() (needs want_hits).
        `taxa`: every read / fragment is also counted on the nodes of the taxonomy set_taxonomy() gave (needs want_hits):
        last_taxa(), taxon_counts().
        `best`: `abundance`, `coverage` and `taxa` take every read's / fragment's best-scoring genomes instead of its whole row
        (PFQ_ROWS_BEST; needs want_hits and want_scores); last_best_rows() gives those rows.  Everything else stays what it is.
        `sweep`: the rows and scores are also counted against the list set_sweep() gave (PFQ_WANT_SWEEP; needs want_hits and
        want_scores, reads only, `threshold` at most the list's lowest): sweep()."""
        lca_flags = (_lca_flags(lca, want_hits, want_scores) | _abundance_flags(abundance, want_hits) | _coverage_flags(coverage, want_hits) |
                     _taxa_flags(taxa, want_hits) | _best_flags(best, want_hits, want_scores) | _sweep_flags(sweep, want_hits, want_scores))
        n = len(off) - 1
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        hits = _ffi.Hits()
        flags = (_ffi.WANT_HITS if want_hits else 0) | (_ffi.WANT_SCORES if want_scores else 0) | _pair_flags(paired, pair_mode) | lca_flags
        _ffi.check(_ffi.lib().pfq_query_batch(self._h, seq.ctypes.data, off.ctypes.data, n, threshold, flags, C.byref(hits)))
        return self._hits_result(hits, want_hits, want_scores)

    def _hits_result(self, hits: "_ffi.Hits", want_hits: bool, want_scores: bool):
        if not want_hits:
            return None
        n = int(hits.n_reads)
        offs = np.ctypeslib.as_array(hits.offsets, shape=(n + 1,)).copy() if n else np.zeros(1, dtype=np.uint64)
        total = int(offs[-1])
        leaves = np.ctypeslib.as_array(hits.leaves, shape=(total,)).copy() if total else np.zeros(0, dtype=np.uint32)
        if not want_scores:
            return offs, leaves
        return offs, leaves, self.last_hit_scores().copy()

    # ---- text
    def parse_text(self, data: bytes, fmt: str, limit: Optional[int] = None, final: bool = True, want_records: bool = False) -> dict:
        """Plain FASTA / FASTQ text (`fmt` "fasta" or "fastq") parsed on the device into the block query_text() classifies
        (pfq_text_parse): data[0] must begin a record's header line.  Records that begin at or beyond `limit` bytes are left
        (None: no limit); `final`: the text ends where the file ends, so an unterminated last line counts.  Returns n_records,
        consumed (where the first record not taken begins), n_bases, stop ("end", "limit", "more": the next record is not
        complete, "slow": it is not an ordinary record, the sequential reader must take over at consumed) and, with
        `want_records`, rec_begin: uint64[n_records + 1], every taken record's byte offset, then consumed.  No counter changes."""
        if fmt not in ("fasta", "fastq"):
            raise ValueError(f"fmt must be 'fasta' or 'fastq', not {fmt!r}")
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        out = _ffi.Text()
        flags = (_ffi.TEXT_FINAL if final else 0) | (_ffi.TEXT_WANT_RECORDS if want_records else 0)
        _ffi.check(_ffi.lib().pfq_text_parse(self._h, buf.ctypes.data if buf.size else None, buf.size, (1 << 64) - 1 if limit is None else limit,
                                             _ffi.TEXT_FASTQ if fmt == "fastq" else _ffi.TEXT_FASTA, flags, C.byref(out)))
        self._text_shape = (int(out.n_records), int(out.n_bases))
        n = int(out.n_records)
        return {"n_records": n, "consumed": int(out.consumed), "n_bases": int(out.n_bases),
                "stop": ("end", "limit", "more", "slow")[out.stop],
                "rec_begin": np.ctypeslib.as_array(out.rec_begin, shape=(n + 1,)).copy() if want_records else None}

    def inflate_text(self, data: bytes, max_text: int = 0, final: bool = True) -> dict:
        """The members of blocked gzip (BGZF) bytes inflated on the device into the text parse_inflated() parses
        (pfq_text_inflate).  Returns what gz_scan() returns for the same arguments and status: uint8[n_members] (0 ok, 1
        malformed deflate, 2 length mismatch, 3 CRC mismatch), n_good: the leading members with status 0, good_text: their text
        bytes.  No counter changes, the block parsed last stays."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        out = _ffi.TextInflated()
        _ffi.check(_ffi.lib().pfq_text_inflate(self._h, buf.ctypes.data if buf.size else None, buf.size, max_text, _ffi.TEXT_FINAL if final else 0,
                                               C.byref(out)))
        res = _gz_members(out.members)
        n = res["n_members"]
        res.update(n_good=int(out.n_good), good_text=int(out.good_text),
                   status=np.ctypeslib.as_array(out.status, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint8))
        return res

    def parse_inflated(self, fmt: str, carry: bytes = b"", limit: Optional[int] = None, final: bool = True, want_records: bool = False) -> dict:
        """parse_text() of `carry` followed by the good text inflate_text() left on the device (pfq_text_parse_inflated): same
        result, and query_text(), format_text(), text_csr() and read_text() see that text."""
        if fmt not in ("fasta", "fastq"):
            raise ValueError(f"fmt must be 'fasta' or 'fastq', not {fmt!r}")
        buf = np.frombuffer(bytes(carry), dtype=np.uint8)
        out = _ffi.Text()
        flags = (_ffi.TEXT_FINAL if final else 0) | (_ffi.TEXT_WANT_RECORDS if want_records else 0)
        _ffi.check(_ffi.lib().pfq_text_parse_inflated(self._h, buf.ctypes.data if buf.size else None, buf.size, (1 << 64) - 1 if limit is None else limit,
                                                      _ffi.TEXT_FASTQ if fmt == "fastq" else _ffi.TEXT_FASTA, flags, C.byref(out)))
        self._text_shape = (int(out.n_records), int(out.n_bases))
        n = int(out.n_records)
        return {"n_records": n, "consumed": int(out.consumed), "n_bases": int(out.n_bases),
                "stop": ("end", "limit", "more", "slow")[out.stop],
                "rec_begin": np.ctypeslib.as_array(out.rec_begin, shape=(n + 1,)).copy() if want_records else None}

    def read_text(self, begin: int, n: int) -> bytes:
        """Bytes [begin, begin + n) of the text parsed last by parse_text() or parse_inflated() (pfq_text_read)."""
        dst = np.zeros(n, dtype=np.uint8)
        _ffi.check(_ffi.lib().pfq_text_read(self._h, begin, n, dst.ctypes.data if n else None))
        return dst.tobytes()

    def last_inflate_ms(self) -> Tuple[float, float]:
        """Device milliseconds of the last inflate_text() with members: (copies to the device, kernel) (pfq_debug_last_inflate)."""
        ms = (C.c_double * 2)()
        _ffi.check(_ffi.lib().pfq_debug_last_inflate(self._h, ms))
        return float(ms[0]), float(ms[1])

    def text_csr(self) -> Tuple[np.ndarray, np.ndarray]:
        """The block parsed last, copied to the host: (seq uint8[n_bases], off uint64[n_records + 1]) (pfq_debug_text_csr)."""
        n, nb = getattr(self, "_text_shape", (0, 0))
        seq, off = np.zeros(nb, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
        _ffi.check(_ffi.lib().pfq_debug_text_csr(self._h, seq.ctypes.data, off.ctypes.data))
        return seq, off

    def query_text(self, threshold: float, want_hits: bool = False, want_scores: bool = False, paired: bool = False,
                   pair_mode: str = "either", lca: Optional[str] = None, abundance: bool = False, coverage: bool = False, taxa: bool = False,
                   best: bool = False, sweep: bool = False):
        """Classifies the block parse_text() parsed last, exactly as query_packed() classifies the same reads from host memory
        (pfq_text_query); same keywords, same return value.  May be repeated: the counters grow each time."""
        lca_flags = (_lca_flags(lca, want_hits, want_scores) | _abundance_flags(abundance, want_hits) | _coverage_flags(coverage, want_hits) |
                     _taxa_flags(taxa, want_hits) | _best_flags(best, want_hits, want_scores) | _sweep_flags(sweep, want_hits, want_scores))
        hits = _ffi.Hits()
        flags = (_ffi.WANT_HITS if want_hits else 0) | (_ffi.WANT_SCORES if want_scores else 0) | _pair_flags(paired, pair_mode) | lca_flags
        _ffi.check(_ffi.lib().pfq_text_query(self._h, threshold, flags, C.byref(hits)))
        return self._hits_result(hits, want_hits, want_scores)

    LEFT_REASONS = {_ffi.LEFT_HEAD: "head", _ffi.LEFT_TAIL: "tail", _ffi.LEFT_REPEATED_ID: "repeated_id"}

    def format_text(self, first_index: int = 0, block: int = 100, pos: bool = True, neg: bool = True) -> dict:
        """The POS / NEG records of the block parse_text() parsed and query_text(want_hits=True) classified last, formatted on the
        device (pfq_text_format; the rules are pfq.h "text output").  Record r has the global index first_index + r and lies in
        result block (first_index + r) // block; only whole blocks whose ids are pairwise different are formatted.  Returns
        n_records, pos, neg (bytes), pos_records, neg_records and left: a list of (first, count, pos_at, neg_at, why) — the runs
        of records left to the caller, the offsets in the two streams where their bytes belong, and why ("head", "tail",
        "repeated_id").  No counter changes."""
        out = _ffi.TextRecords()
        flags = (_ffi.FMT_POS if pos else 0) | (_ffi.FMT_NEG if neg else 0)
        _ffi.check(_ffi.lib().pfq_text_format(self._h, first_index, block, flags, C.byref(out)))
        left = [(int(x.first), int(x.count), int(x.pos_at), int(x.neg_at), self.LEFT_REASONS[x.why]) for x in out.left[:int(out.n_left)]]
        return {"n_records": int(out.n_records), "pos": C.string_at(out.pos, int(out.pos_bytes)), "neg": C.string_at(out.neg, int(out.neg_bytes)),
                "pos_records": int(out.pos_records), "neg_records": int(out.neg_records), "left": left}

    def last_format_ms(self) -> Tuple[float, float, float]:
        """Device milliseconds of the last format_text() under PFQ_FMT_TIME=1: (ids and blocks, sizes and scans, emit)
        (pfq_debug_last_format)."""
        ms = (C.c_double * 3)()
        _ffi.check(_ffi.lib().pfq_debug_last_format(self._h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    # ---- blocked gzip written on the device
    @staticmethod
    def _bgzf(out) -> dict:
        n, k = int(out.n_members), int(out.n_pieces)
        return {"gz": C.string_at(out.gz, int(out.gz_bytes)), "n_members": n,
                "piece_begin": np.ctypeslib.as_array(out.piece_begin, shape=(k + 1,)).copy(),
                "member_begin": np.ctypeslib.as_array(out.member_begin, shape=(n + 1,)).copy()}

    def deflate_bytes(self, data: bytes, cuts: Sequence[int] = ()) -> dict:
        """`data`, cut at the ascending offsets `cuts` into len(cuts) + 1 pieces and every piece into members of 65280 text bytes,
        deflated on the device into blocked gzip (pfq_bgzf_deflate; the rules are pfq.h "blocked gzip written on the device").
        Returns gz (the members back to back, no end marker), n_members, piece_begin uint64[pieces + 1] and member_begin
        uint64[n_members + 1], offsets into gz.  No counter changes."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        c = np.asarray(list(cuts), dtype=np.uint64)
        out = _ffi.Bgzf()
        _ffi.check(_ffi.lib().pfq_bgzf_deflate(self._h, buf.ctypes.data if buf.size else None, buf.size, c.ctypes.data if c.size else None, c.size,
                                               C.byref(out)))
        return self._bgzf(out)

    def format_text_gz(self, first_index: int = 0, block: int = 100, pos: bool = True, neg: bool = True) -> dict:
        """format_text() for the same arguments with the two streams deflated on the device instead of copied
        (pfq_text_format_gz): pos_gz and neg_gz replace pos and neg, and pos_piece_begin / neg_piece_begin uint64[len(left) + 2]
        say where the pieces lie: piece j of a stream is what belongs between the caller's bytes for left run j - 1 and j."""
        out, pg, ng = _ffi.TextRecords(), _ffi.Bgzf(), _ffi.Bgzf()
        flags = (_ffi.FMT_POS if pos else 0) | (_ffi.FMT_NEG if neg else 0)
        _ffi.check(_ffi.lib().pfq_text_format_gz(self._h, first_index, block, flags, C.byref(out), C.byref(pg), C.byref(ng)))
        left = [(int(x.first), int(x.count), int(x.pos_at), int(x.neg_at), self.LEFT_REASONS[x.why]) for x in out.left[:int(out.n_left)]]
        p, q = self._bgzf(pg), self._bgzf(ng)
        return {"n_records": int(out.n_records), "pos_gz": p["gz"], "neg_gz": q["gz"], "pos_piece_begin": p["piece_begin"],
                "neg_piece_begin": q["piece_begin"], "pos_bytes": int(out.pos_bytes), "neg_bytes": int(out.neg_bytes),
                "pos_records": int(out.pos_records), "neg_records": int(out.neg_records), "left": left}

    def last_deflate_ms(self) -> Tuple[float, float, float]:
        """Device milliseconds of the last deflate_bytes() or format_text_gz() stream with members: (copy in, deflate kernel,
        scan + gather + copy out) (pfq_debug_last_deflate)."""
        ms = (C.c_double * 3)()
        _ffi.check(_ffi.lib().pfq_debug_last_deflate(self._h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    # ---- read preprocessing
    PREP_REASONS = ("kept", "short", "n", "complexity", "mate")

    def prep_reads(self, seq: np.ndarray, off: np.ndarray, qual: Optional[np.ndarray] = None, has_qual: Optional[np.ndarray] = None, *,
                   trim_quality: int = 0, trim_window: int = 4, poly_x: int = 0, min_length: int = 0, max_n: Optional[int] = None,
                   min_complexity: int = 0, paired: bool = False, want_reads: bool = False) -> dict:
        """One block of reads from host memory trimmed and filtered on the device into the block query_prep() classifies
        (pfq_prep_reads; the rules are pfq.h "read preprocessing").  `qual`: Phred+33 bytes that share `off` with `seq` (None: no
        read has qualities); `has_qual`: a byte per read (None: all have).  `max_n` None: off.  `paired`: reads 2i and 2i + 1
        are mates and are dropped together.  Returns the totals n_reads, n_kept, bases_in, bases_kept, n_trimmed and n_reason
        (a dict by PREP_REASONS) and, with `want_reads`, begin, len, reason uint32[n_reads] and kept uint32[n_kept] (else None).
        No counter changes."""
        n = len(off) - 1
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        qual = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8)
        has_qual = None if has_qual is None else np.ascontiguousarray(has_qual, dtype=np.uint8)
        total = int(off[-1]) if n >= 0 and off.size else 0
        if seq.size < total or (qual is not None and qual.size < total):
            raise ValueError("seq and qual must hold off[-1] bytes each: qual shares off with seq, one quality byte per base")
        if has_qual is not None and has_qual.size != n:
            raise ValueError("has_qual must hold one byte per read")
        par = _ffi.PrepParams(trim_quality, trim_window, poly_x, min_length, _ffi.PREP_MAX_N_OFF if max_n is None else max_n, min_complexity,
                              (_ffi.PREP_PAIRED if paired else 0) | (_ffi.PREP_WANT_READS if want_reads else 0))
        out = _ffi.Prep()
        _ffi.check(_ffi.lib().pfq_prep_reads(self._h, seq.ctypes.data if seq.size else None, None if qual is None or not qual.size else qual.ctypes.data,
                                             off.ctypes.data, None if has_qual is None or not n else has_qual.ctypes.data, n, C.byref(par),
                                             C.byref(out)))
        nk = int(out.n_kept)
        self._prep_shape = (nk, int(out.bases_kept))
        self._prep_reads = n

        def arr(p, m):
            if not want_reads:
                return None
            return np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0, dtype=np.uint32)
        return {"n_reads": int(out.n_reads), "n_kept": nk, "bases_in": int(out.bases_in), "bases_kept": int(out.bases_kept),
                "n_trimmed": int(out.n_trimmed), "n_reason": {k: int(out.n_reason[i]) for i, k in enumerate(self.PREP_REASONS)},
                "begin": arr(out.begin, n), "len": arr(out.len, n), "reason": arr(out.reason, n), "kept": arr(out.kept, nk)}

    def prep_csr(self) -> Tuple[np.ndarray, np.ndarray]:
        """The block prepared last, copied to the host: (seq uint8[bases_kept], off uint64[n_kept + 1]) (pfq_debug_prep_csr)."""
        n, nb = getattr(self, "_prep_shape", (0, 0))
        seq, off = np.zeros(nb, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
        _ffi.check(_ffi.lib().pfq_debug_prep_csr(self._h, seq.ctypes.data, off.ctypes.data))
        return seq, off

    def last_prep_ms(self) -> Tuple[float, float, float]:
        """Device milliseconds of the last prep_reads(): (trim and mark, the scans, offsets and gather) (pfq_debug_last_prep)."""
        ms = (C.c_double * 3)()
        _ffi.check(_ffi.lib().pfq_debug_last_prep(self._h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    def set_adapters(self, set1, set2=None, min_overlap: int = 5, max_error_percent: int = 10) -> None:
        """3' adapters that every later prep_reads() cuts before its other steps (pfq_tree_set_adapters; the rule is pfq.h
        "adapters"): each read ends at the leftmost position where an adapter of its set matches over at least `min_overlap`
        bases with at most `max_error_percent` percent mismatches.  `set1`: sequences (str or bytes, ACGT) for unpaired reads and
        first mates; `set2`: for second mates of a paired call (None or empty: they use `set1`).  An empty `set1`: no adapters."""
        def strings(seqs):
            seqs = list(seqs or ())
            arr = (C.c_char_p * max(len(seqs), 1))()
            for i, s in enumerate(seqs):
                arr[i] = s.encode() if isinstance(s, str) else (None if s is None else bytes(s))
            return arr, len(seqs)
        a1, n1 = strings(set1)
        a2, n2 = strings(set2)
        _ffi.check(_ffi.lib().pfq_tree_set_adapters(self._h, a1, n1, a2, n2, min_overlap, max_error_percent))

    def last_adapters(self) -> dict:
        """What the adapter step of the last prep_reads() found, before the mate rule (pfq_prep_last_adapters): n_reads, n_found
        (reads with cut < L), bases_cut, found (reads per adapter: set1 at [0, 8), set2 at [8, 16)) and, if that call had
        want_reads, cut uint32[n_reads] and which uint8[n_reads] (0xff: no adapter), else None for both."""
        out = _ffi.PrepAdapters()
        _ffi.check(_ffi.lib().pfq_prep_last_adapters(self._h, C.byref(out)))
        n = int(out.n_reads)

        def arr(p, dtype):
            if not p:
                return None
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype=dtype)
        return {"n_reads": n, "n_found": int(out.n_found), "bases_cut": int(out.bases_cut), "found": [int(v) for v in out.found],
                "cut": arr(out.cut, np.uint32), "which": arr(out.which, np.uint8)}

    def last_adapters_ms(self) -> float:
        """Device milliseconds of the adapter kernels of the last prep_reads() (pfq_debug_last_adapters)."""
        ms = C.c_double()
        _ffi.check(_ffi.lib().pfq_debug_last_adapters(self._h, C.byref(ms)))
        return float(ms.value)

    OVERLAP_TOTALS = ("n_fragments", "n_analysed", "n_skipped", "n_overlapped", "n_readthrough", "reads_cut", "bases_cut")

    def set_mate_overlap(self, min_overlap: int = 30, max_error_percent: int = 10) -> None:
        """Every later prep_reads(paired=True) finds each fragment's insert length from the overlap of its mates and cuts both
        mates there (pfq_tree_set_mate_overlap; the rule is pfq.h "mate overlap"): the largest insert at which the mates are
        reverse complements over at least `min_overlap` bases with at most `max_error_percent` percent mismatches.
        `min_overlap` 0 drops it."""
        _ffi.check(_ffi.lib().pfq_tree_set_mate_overlap(self._h, min_overlap, max_error_percent))

    def last_overlap(self) -> dict:
        """What the mate overlap step of the last prep_reads() found, before the mate rule (pfq_prep_last_overlap): the totals
        OVERLAP_TOTALS, hist uint64[1025] (fragments per insert length) and, if that call had want_reads, insert and mismatches
        uint32[n_fragments] (insert 0xffffffff: none), else None for both."""
        out = _ffi.PrepOverlap()
        _ffi.check(_ffi.lib().pfq_prep_last_overlap(self._h, C.byref(out)))
        n = int(out.n_fragments)

        def arr(p):
            if not p:
                return None
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint32)
        res = {k: int(getattr(out, k)) for k in self.OVERLAP_TOTALS}
        res.update(hist=np.ctypeslib.as_array(out.hist, shape=(_ffi.OVERLAP_INSERT_MAX + 1,)).copy(), insert=arr(out.insert), mismatches=arr(out.mismatches))
        return res

    def last_overlap_ms(self) -> float:
        """Device milliseconds of the overlap kernel of the last prep_reads() (pfq_debug_last_overlap)."""
        ms = C.c_double()
        _ffi.check(_ffi.lib().pfq_debug_last_overlap(self._h, C.byref(ms)))
        return float(ms.value)

    CORRECT_TOTALS = ("n_fragments_corrected", "n_bases", "n_unresolved", "n_no_quality")
    PATCH_DTYPE = np.dtype([("read", np.uint32), ("pos", np.uint32), ("base", np.uint8), ("qual", np.uint8), ("old_base", np.uint8), ("old_qual", np.uint8)])

    def set_mate_correct(self, high: int = _ffi.MATE_CORRECT_HIGH, low: int = _ffi.MATE_CORRECT_LOW) -> None:
        """Every later prep_reads(paired=True) with the mate overlap set corrects, where the mates of a fragment disagree inside
        their overlap, the base whose quality is at most `low` by the mate's if that one's is at least `high`, before trimming
        and the gather (pfq_tree_set_mate_correct; the rule is pfq.h "mate correction").  `high` 0 drops it."""
        _ffi.check(_ffi.lib().pfq_tree_set_mate_correct(self._h, high, low))

    def last_corrections(self) -> dict:
        """What the mate correction of the last prep_reads() did (pfq_prep_last_corrections): n_fragments_corrected, n_bases (a
        list: first mates, second mates), n_unresolved, n_no_quality and, if that call had want_reads, patches: a structured
        array PATCH_DTYPE (read, pos, base, qual, old_base, old_qual), ascending by (read, pos); else None."""
        out = _ffi.PrepCorrections()
        _ffi.check(_ffi.lib().pfq_prep_last_corrections(self._h, C.byref(out)))
        n = int(out.n_patches)
        patches = None
        if out.patches:
            patches = np.frombuffer(C.string_at(out.patches, n * self.PATCH_DTYPE.itemsize), dtype=self.PATCH_DTYPE).copy() if n else np.zeros(0, dtype=self.PATCH_DTYPE)
        return {"n_fragments_corrected": int(out.n_fragments_corrected), "n_bases": [int(out.n_bases[0]), int(out.n_bases[1])],
                "n_unresolved": int(out.n_unresolved), "n_no_quality": int(out.n_no_quality), "patches": patches}

    def last_corrections_ms(self) -> float:
        """Device milliseconds of the scan and the patch kernel of the last prep_reads(want_reads=True) with the mate correction
        (pfq_debug_last_corrections); last_overlap_ms() has the overlap kernel, the correction or its counting included."""
        ms = C.c_double()
        _ffi.check(_ffi.lib().pfq_debug_last_corrections(self._h, C.byref(ms)))
        return float(ms.value)

    DEPLETE_TOTALS = ("n_units", "units_removed", "reads_removed", "bases_removed", "n_kept", "bases_kept")

    def prep_deplete(self, screen: "BloomTree", threshold: float, paired: bool = False, pair_mode: str = "either") -> dict:
        """Removes from the block prep_reads() prepared last the units (kept reads; `paired`: kept fragments) that hit `screen`, a
        second tree on the same device, at `threshold` (pfq_prep_deplete; the rule is pfq.h "depletion").  prep_csr(),
        query_prep() and a further prep_deplete() then see the remaining units.  `screen`'s counters grow as by a query of the
        block; this tree's do not change.  Returns the totals DEPLETE_TOTALS and, if the block was prepared with want_reads,
        kept uint32[n_kept] (indices into the block given to prep_reads) and reason uint32[n_reads] (5 = depleted), else None."""
        out = _ffi.PrepDepleted()
        n_reads = getattr(self, "_prep_reads", 0)
        _ffi.check(_ffi.lib().pfq_prep_deplete(self._h, screen._h, threshold, _pair_flags(paired, pair_mode), C.byref(out)))
        nk = int(out.n_kept)
        self._prep_shape = (nk, int(out.bases_kept))

        def arr(p, m):
            if not p:
                return None
            return np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0, dtype=np.uint32)
        res = {k: int(getattr(out, k)) for k in self.DEPLETE_TOTALS}
        res.update(kept=arr(out.kept, nk), reason=arr(out.reason, n_reads))
        return res

    def last_deplete_ms(self) -> Tuple[float, float]:
        """Device milliseconds of the last prep_deplete(): (the screen's classification, mark + scans + compaction)
        (pfq_debug_last_deplete)."""
        ms = (C.c_double * 2)()
        _ffi.check(_ffi.lib().pfq_debug_last_deplete(self._h, ms))
        return float(ms[0]), float(ms[1])

    def query_prep(self, threshold: float, want_hits: bool = False, want_scores: bool = False, paired: bool = False,
                   pair_mode: str = "either", lca: Optional[str] = None, abundance: bool = False, coverage: bool = False, taxa: bool = False,
                   best: bool = False, sweep: bool = False):
        """Classifies the block prep_reads() prepared last, exactly as query_packed() classifies the kept, trimmed reads from host
        memory (pfq_prep_query); same keywords, same return value; `paired` needs a block prepared with paired=True.  May be
        repeated: the counters grow each time."""
        lca_flags = (_lca_flags(lca, want_hits, want_scores) | _abundance_flags(abundance, want_hits) | _coverage_flags(coverage, want_hits) |
                     _taxa_flags(taxa, want_hits) | _best_flags(best, want_hits, want_scores) | _sweep_flags(sweep, want_hits, want_scores))
        hits = _ffi.Hits()
        flags = (_ffi.WANT_HITS if want_hits else 0) | (_ffi.WANT_SCORES if want_scores else 0) | _pair_flags(paired, pair_mode) | lca_flags
        _ffi.check(_ffi.lib().pfq_prep_query(self._h, threshold, flags, C.byref(hits)))
        return self._hits_result(hits, want_hits, want_scores)

    def _segments(self, out: "_ffi.Segments"):
        n = int(out.n_seqs)
        offs = np.ctypeslib.as_array(out.offsets, shape=(n + 1,)).copy() if n else np.zeros(1, dtype=np.uint64)
        total = int(offs[-1])
        segs = np.zeros(total, dtype=SEGMENT_DTYPE)
        if total:
            C.memmove(segs.ctypes.data, out.seg, total * SEGMENT_DTYPE.itemsize)
        self.last_n_frames = int(out.n_frames)
        return offs, segs

    def query_frames(self, seq: np.ndarray, off: np.ndarray, frame: int, step: int, threshold: float):
        """Long sequences (contigs, long reads) from host memory, classified in overlapping frames of `frame` bases every
        `step` bases (pfq_query_frames).  Returns (offsets uint64[n + 1], segments): segments[offsets[i]:offsets[i + 1]] are
        those of sequence i, a structured array (SEGMENT_DTYPE) ordered by first_frame, then leaf; coordinates are 0-based and
        half-open.  The leaf counters grow by one per (sequence, distinct leaf among its segments); last_n_frames is the
        number of frames the call classified."""
        n = len(off) - 1
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        out = _ffi.Segments()
        _ffi.check(_ffi.lib().pfq_query_frames(self._h, seq.ctypes.data, off.ctypes.data, n, frame, step, threshold, 0, C.byref(out)))
        return self._segments(out)

    def query_frames_device(self, d_seq: int, d_off: int, n_seqs: int, total_bytes: int, frame: int, step: int, threshold: float,
                            stream: int = 0):
        """The same with the sequences already resident in HBM (raw device pointers), on `stream`; synchronous."""
        out = _ffi.Segments()
        _ffi.check(_ffi.lib().pfq_query_frames_device(self._h, d_seq, d_off, n_seqs, total_bytes, frame, step, threshold, 0, stream,
                                                      C.byref(out)))
        return self._segments(out)

    def last_hit_scores(self) -> np.ndarray:
        """Scores of the hits of the last query call, which must have asked for them (view of the library's buffer, valid
        until the next query call on this tree)."""
        p = C.POINTER(C.c_uint32)()
        n = C.c_uint64()
        _ffi.check(_ffi.lib().pfq_last_hit_scores(self._h, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(p, shape=(n.value,)) if n.value else np.zeros(0, dtype=np.uint32)

    def query_device(self, d_seq: int, d_off: int, n_reads: int, total_bytes: int, threshold: float,
                     stream: int = 0, paired: bool = False, pair_mode: str = "either", lca: Optional[str] = None) -> None:
        """One block already resident in HBM (raw device pointers), asynchronous on `stream`.  `lca`: None or "all"
        (as in query_packed; "best" needs the hits: query_device_hits)."""
        flags = _pair_flags(paired, pair_mode) | _lca_flags(lca, False, False)
        _ffi.check(_ffi.lib().pfq_query_batch_device(self._h, d_seq, d_off, n_reads, total_bytes, threshold, flags, stream, None))

    def query_device_hits(self, d_seq: int, d_off: int, n_reads: int, total_bytes: int, threshold: float, stream: int = 0,
                          want_scores: bool = False, paired: bool = False, pair_mode: str = "either",
                          lca: Optional[str] = None, abundance: bool = False, coverage: bool = False, taxa: bool = False,
                          best: bool = False, sweep: bool = False):
        """The same block with PFQ_WANT_HITS: synchronous, returns the CSR (offsets, leaves) — with `want_scores`
        (offsets, leaves, scores) — as views of the library's buffers (valid until the next call on this tree).
        `paired`: one row per fragment (reads 2i, 2i + 1), `lca`: None, "all" or "best", `abundance`, `coverage`, `taxa`, `best`, `sweep`, as in query_packed."""
        hits = _ffi.Hits()
        flags = (_ffi.WANT_HITS | (_ffi.WANT_SCORES if want_scores else 0) | _pair_flags(paired, pair_mode) |
                 _lca_flags(lca, True, want_scores) | _abundance_flags(abundance, True) | _coverage_flags(coverage, True) | _taxa_flags(taxa, True) |
                 _best_flags(best, True, want_scores) | _sweep_flags(sweep, True, want_scores))
        _ffi.check(_ffi.lib().pfq_query_batch_device(self._h, d_seq, d_off, n_reads, total_bytes, threshold, flags,
                                                     stream, C.byref(hits)))
        n_reads = int(hits.n_reads)
        offs = np.ctypeslib.as_array(hits.offsets, shape=(n_reads + 1,)) if n_reads else np.zeros(1, dtype=np.uint64)
        total = int(offs[-1])
        leaves = np.ctypeslib.as_array(hits.leaves, shape=(total,)) if total else np.zeros(0, dtype=np.uint32)
        if not want_scores:
            return offs, leaves
        return offs, leaves, self.last_hit_scores()

    def query_pairs(self, r1: Sequence[bytes], r2: Sequence[bytes], threshold: float,
                    mode: str = "either", lca: Optional[str] = None, abundance: bool = False,
                    coverage: bool = False, taxa: bool = False, best: bool = False) -> List[List[int]]:
        """Mates r1[i], r2[i] as fragment i: its leaves (ascending indices into get_leaf_counts' order), the union
        (mode "either") or the intersection ("both") of the mates' hit sets.  Leaf counters count fragments.
        `lca`: None, "all" or "best" (scores are then computed as well): the fragments' clades are in last_lca().
        `abundance`: the fragments' rows are also logged for abundance(); `coverage`: both mates' matched k-mers are also
        sketched for coverage(), per genome the fragment lists; `taxa`: the fragments are also counted on the taxonomy's nodes;
        `best`: those three take every fragment's best-scoring genomes (scores are then computed as well; last_best_rows())."""
        if lca not in (None, "all", "best"):
            raise ValueError(f"lca must be None, 'all' or 'best', not {lca!r}")
        if len(r1) != len(r2):
            raise ValueError(f"{len(r1)} first mates but {len(r2)} second mates")
        seq, off = pack_reads([m for pair in zip(r1, r2) for m in pair])
        offs, leaves = self.query_packed(seq, off, threshold, want_hits=True, want_scores=lca == "best" or best, paired=True,
                                         pair_mode=mode, lca=lca, abundance=abundance, coverage=coverage, taxa=taxa, best=best)[:2]
        return [leaves[int(offs[i]):int(offs[i + 1])].tolist() for i in range(len(r1))]

    # ---- clades (lowest common ancestors)
    def clades(self) -> List[Tuple[int, int, int, int, str]]:
        """The clades of the tree as it is: (parent, depth, first_leaf, n_leaves, name) per node reachable from the root, in
        pre-order (the root is clade 0, its parent -1); a clade's leaves are get_leaf_counts()[first_leaf : first_leaf +
        n_leaves]."""
        p = C.POINTER(_ffi.Clade)()
        n = C.c_uint64()
        _ffi.check(_ffi.lib().pfq_tree_clades(self._h, C.byref(p), C.byref(n)))
        return [(-1 if p[i].parent == _ffi.NO_CLADE else int(p[i].parent), int(p[i].depth), int(p[i].first_leaf),
                 int(p[i].n_leaves), p[i].name.decode()) for i in range(n.value)]

    def clade_counts(self) -> Tuple[np.ndarray, np.ndarray]:
        """(here, below): per clade the reads / fragments whose LCA it is, and the sum of that over its subtree."""
        here, below = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        n = C.c_uint64()
        _ffi.check(_ffi.lib().pfq_clade_counts(self._h, C.byref(here), C.byref(below), C.byref(n)))
        if not n.value:
            return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
        return (np.ctypeslib.as_array(here, shape=(n.value,)).copy(), np.ctypeslib.as_array(below, shape=(n.value,)).copy())

    def last_lca(self) -> np.ndarray:
        """Clade index per read / fragment of the last query call, which must have asked for it (_ffi.NO_CLADE: no hit)."""
        p = C.POINTER(C.c_uint32)()
        n = C.c_uint64()
        _ffi.check(_ffi.lib().pfq_last_lca(self._h, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.uint32)

    # ---- best rows (PFQ_ROWS_BEST)
    def last_best_rows(self) -> Tuple[np.ndarray, np.ndarray]:
        """(offsets, leaves): per read / fragment of the last query call, which must have set `best`, the genomes of its row
        whose score is the row's highest, ascending (pfq_last_best_rows); copied from the device by this call."""
        hits = _ffi.Hits()
        _ffi.check(_ffi.lib().pfq_last_best_rows(self._h, C.byref(hits)))
        n = int(hits.n_reads)
        offs = np.ctypeslib.as_array(hits.offsets, shape=(n + 1,)).copy()
        total = int(offs[-1])
        leaves = np.ctypeslib.as_array(hits.leaves, shape=(total,)).copy() if total else np.zeros(0, dtype=np.uint32)
        return offs, leaves

    # ---- taxonomy (PFQ_WANT_TAXA)
    def set_taxonomy(self, taxon_parent: Sequence[int], taxon_names: Sequence[str], leaf_taxon: Sequence[int]) -> None:
        """Lays a taxonomy over the current leaves (pfq_tree_set_taxonomy): taxon 0 is the root (parent _ffi.NO_CLADE or -1),
        taxon_parent[i] < i, leaf_taxon[l] is the taxon genome l of get_leaf_counts() sits directly under.  Replaces an earlier
        one and zeroes the taxon counters; prune_tree and insert drop it."""
        if len(taxon_parent) != len(taxon_names):
            raise ValueError(f"{len(taxon_parent)} taxon parents but {len(taxon_names)} taxon names")
        par = np.ascontiguousarray([_ffi.NO_CLADE if int(x) < 0 else int(x) for x in taxon_parent], dtype=np.uint32)
        leaf = np.ascontiguousarray(np.asarray(leaf_taxon, dtype=np.int64), dtype=np.uint32)
        names = (C.c_char_p * max(len(taxon_names), 1))(*[t.encode() for t in taxon_names])
        _ffi.check(_ffi.lib().pfq_tree_set_taxonomy(self._h, len(par), par.ctypes.data if par.size else None, names,
                                                    leaf.ctypes.data if leaf.size else None))

    def taxa(self) -> List[Tuple[int, int, int, int, int, str]]:
        """The nodes of the taxonomy: (parent, depth, first_rank, n_leaves, leaf, name) per node in pre-order; parent -1 for
        the root, leaf -1 for a taxon (a genome node: its index in get_leaf_counts()).  Empty when no taxonomy is set."""
        p = C.POINTER(_ffi.Taxon)()
        n = C.c_uint64()
        _ffi.check(_ffi.lib().pfq_tree_taxa(self._h, C.byref(p), C.byref(n)))
        return _taxon_rows(p, n.value)

    def taxon_counts(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(here, below, any) per node of the taxonomy: the reads / fragments assigned to it, the sum of that over its subtree,
        and those that hit at least one genome below it."""
        here, below, any_ = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        n = C.c_uint64()
        _ffi.check(_ffi.lib().pfq_taxon_counts(self._h, C.byref(here), C.byref(below), C.byref(any_), C.byref(n)))
        if not n.value:
            return tuple(np.zeros(0, dtype=np.uint64) for _ in range(3))
        return tuple(np.ctypeslib.as_array(x, shape=(n.value,)).copy() for x in (here, below, any_))

    def last_taxa(self) -> np.ndarray:
        """Node index per read / fragment of the last query call, which must have asked for it (_ffi.NO_CLADE: no hit)."""
        p = C.POINTER(C.c_uint32)()
        n = C.c_uint64()
        _ffi.check(_ffi.lib().pfq_last_taxa(self._h, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.uint32)

    # ---- abundance (PFQ_WANT_ABUNDANCE)
    def abundance(self, max_iters: int = 200, tol: int = 65) -> dict:
        """Per-genome abundance from the rows the `abundance=True` calls have logged (pfq_abundance_estimate): an integer
        EM from a uniform start that gives every genome its share of the ambiguous rows.  `mass` (numpy uint64, leaf order of
        get_leaf_counts) is in units of 2**-16 reads / fragments, `tol` likewise (65: below 0.001).  Also `unique`, the class
        counters n_units, n_unhit, n_unique, n_ambiguous, n_all_leaves, n_entries, and iterations, converged, last_delta.
        The log is not consumed: more queries and another estimate may follow."""
        a = _ffi.Abundance()
        _ffi.check(_ffi.lib().pfq_abundance_estimate(self._h, max_iters, tol, C.byref(a)))
        n = int(a.n_leaves)
        out = {"mass": np.ctypeslib.as_array(a.mass, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint64),
               "unique": np.ctypeslib.as_array(a.unique, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint64)}
        for k in ("n_units", "n_unhit", "n_unique", "n_ambiguous", "n_all_leaves", "n_entries", "iterations", "converged", "last_delta"):
            out[k] = int(getattr(a, k))
        return out

    def abundance_reset(self) -> None:
        """Empties the abundance log (reset_counts, prune_tree and insert do so as well)."""
        _ffi.check(_ffi.lib().pfq_abundance_reset(self._h))

    def abundance_absorb(self, other: "BloomTree") -> None:
        """Moves the abundance log of `other`, a replica of this database (on any device), into this tree's and empties it."""
        _ffi.check(_ffi.lib().pfq_abundance_absorb(self._h, other._h))

    # ---- coverage (PFQ_WANT_COVERAGE)
    def coverage(self) -> dict:
        """Per-genome distinct k-mers and what goes with them, from the `coverage=True` calls so far (pfq_coverage_get), as
        numpy arrays in the leaf order of get_leaf_counts: `registers` uint8 (n_leaves, 2**precision), the HyperLogLog
        sketches; `units`, `matched`, `filter_bits` uint64; `distinct`, `genome_kmers` float64; and the ints `n_leaves`,
        `n_units`, `precision`.  Breadth of coverage is distinct / genome_kmers, duplication matched / distinct.  Before
        any such call everything but filter_bits and genome_kmers is 0.  The sketch is not consumed."""
        c = _ffi.Coverage()
        _ffi.check(_ffi.lib().pfq_coverage_get(self._h, C.byref(c)))
        n, p = int(c.n_leaves), int(c.precision)

        def arr(ptr, shape, dtype):
            return np.ctypeslib.as_array(ptr, shape=shape).copy() if n else np.zeros(shape, dtype=dtype)
        out = {"n_leaves": n, "n_units": int(c.n_units), "precision": p, "registers": arr(c.registers, (n, 1 << p), np.uint8)}
        for k in ("units", "matched", "filter_bits"):
            out[k] = arr(getattr(c, k), (n,), np.uint64)
        for k in ("distinct", "genome_kmers"):
            out[k] = arr(getattr(c, k), (n,), np.float64)
        return out

    def coverage_reset(self) -> None:
        """Empties the coverage sketch and frees it (reset_counts, prune_tree and insert do so as well)."""
        _ffi.check(_ffi.lib().pfq_coverage_reset(self._h))

    def coverage_absorb(self, other: "BloomTree") -> None:
        """Merges the coverage sketch of `other`, a replica of this database (on any device) or the same shard of it, into
        this tree's (registers: element-wise max, counters: sums) and empties it."""
        _ffi.check(_ffi.lib().pfq_coverage_absorb(self._h, other._h))

    # ---- threshold sweep (PFQ_WANT_SWEEP)
    def set_sweep(self, thresholds: Sequence[float]) -> None:
        """Sets the list of thresholds (1 to _ffi.SWEEP_MAX floats, strictly ascending) the `sweep=True` calls count against
        (pfq_tree_set_sweep) and zeroes the counters; an empty list drops it.  Refused on a tree that is not superset-verified
        and on a subtree shard."""
        thr = np.ascontiguousarray(thresholds, dtype=np.float32)
        if thr.ndim != 1:
            raise ValueError("thresholds must be a flat sequence of floats")
        _ffi.check(_ffi.lib().pfq_tree_set_sweep(self._h, thr.ctypes.data_as(C.POINTER(C.c_float)), len(thr)))

    def sweep(self) -> dict:
        """Per threshold of the list what a query of its own at that threshold would have counted for the reads of the
        `sweep=True` calls so far (pfq_sweep_get), as numpy arrays: `thresholds` float32 (T,); `leaf_units` (the leaf counters'
        increase) and `leaf_unique` (reads that list that genome alone) uint64 (T, n_leaves) in the leaf order of
        get_leaf_counts; `units_hit` (reads with a hit), `units_unique` (reads with one genome), `entries` (listed (read,
        genome) pairs), `genomes_hit` uint64 (T,); and the ints `n_leaves`, `n_units`.  The counters are not consumed."""
        c = _ffi.Sweep()
        _ffi.check(_ffi.lib().pfq_sweep_get(self._h, C.byref(c)))
        t, n = int(c.n_thresholds), int(c.n_leaves)

        def arr(ptr, shape, dtype):
            return np.ctypeslib.as_array(ptr, shape=shape).copy() if all(shape) else np.zeros(shape, dtype=dtype)
        out = {"n_leaves": n, "n_units": int(c.n_units), "thresholds": arr(c.thresholds, (t,), np.float32)}
        for k in ("leaf_units", "leaf_unique"):
            out[k] = arr(getattr(c, k), (t, n), np.uint64)
        for k in ("units_hit", "units_unique", "entries", "genomes_hit"):
            out[k] = arr(getattr(c, k), (t,), np.uint64)
        return out

    def sweep_reset(self) -> None:
        """Zeroes the sweep's counters and keeps the list (reset_counts does so as well)."""
        _ffi.check(_ffi.lib().pfq_sweep_reset(self._h))

    def sweep_absorb(self, other: "BloomTree") -> None:
        """Adds the sweep counters of `other`, a replica of this database (on any device) with the same list, to this tree's
        and zeroes them there."""
        _ffi.check(_ffi.lib().pfq_sweep_absorb(self._h, other._h))

    # ---- genome similarity
    def similarity(self, other: Optional["BloomTree"] = None, leaves_a: Optional[Sequence[int]] = None,
                   leaves_b: Optional[Sequence[int]] = None) -> dict:
        """How related are the genomes of this database, or of this one and `other` (pfq_tree_similarity)?  leaves_a / leaves_b
        are leaf indices in the order of get_leaf_counts (None: all leaves; any order, repeats allowed; an empty list gives an
        empty result), into this tree and into `other` (None: this tree).  Returns numpy copies: `shared_bits` uint32
        (n_a, n_b), the set bits the two leaves' filters have in common; `bits_a`, `bits_b` uint64, each filter's set bits;
        `kmers_a`, `kmers_b`, and per pair `shared_kmers`, `jaccard` float64, the estimates derived from them.  The trees must
        share k, filter size, hashes and seeds.  Changes nothing a query left behind."""
        def as_list(v):
            if v is None:
                return None, 0, None
            a = np.ascontiguousarray(v, dtype=np.uint32).reshape(-1)
            n = len(a)
            if not n:
                a = np.zeros(1, dtype=np.uint32)  # (an empty list is still a list: the pointer must not be NULL)
            return a, n, a.ctypes.data
        la, na, pa = as_list(leaves_a)
        lb, nb, pb = as_list(leaves_b)
        s = _ffi.Similarity()
        _ffi.check(_ffi.lib().pfq_tree_similarity(self._h, pa, na, other._h if other is not None else None, pb, nb, C.byref(s)))
        n_a, n_b = int(s.n_a), int(s.n_b)

        def arr(ptr, shape, dtype):
            return np.ctypeslib.as_array(ptr, shape=shape).copy() if n_a and n_b else np.zeros(shape, dtype=dtype)
        out = {"shared_bits": arr(s.shared_bits, (n_a, n_b), np.uint32)}
        for k, n in (("bits_a", n_a), ("bits_b", n_b)):
            out[k] = arr(getattr(s, k), (n,), np.uint64)
        for k, n in (("kmers_a", n_a), ("kmers_b", n_b)):
            out[k] = arr(getattr(s, k), (n,), np.float64)
        for k in ("shared_kmers", "jaccard"):
            out[k] = arr(getattr(s, k), (n_a, n_b), np.float64)
        return out

    def last_similarity(self) -> Tuple[float, int]:
        """(device milliseconds of the intersection kernel, slices of the filter words) of the last similarity() call that had
        pairs to compute (pfq_debug_last_similarity); the time is measured only under set_option("PFQ_SIM_TIME", "1"), else 0."""
        ms, sl = C.c_double(), C.c_uint32()
        _ffi.check(_ffi.lib().pfq_debug_last_similarity(self._h, C.byref(ms), C.byref(sl)))
        return float(ms.value), int(sl.value)

    # ---- re-clustering
    def recluster(self) -> "BloomTree":
        """A new tree over this tree's leaves, on the same device, whose shape follows from the leaf filters alone
        (pfq_tree_recluster): average-linkage clustering of their chance-corrected similarities.  The leaves keep their names and
        filter words; this tree is left as it was.  merges() of the new tree is the dendrogram."""
        h = C.c_void_p()
        _ffi.check(_ffi.lib().pfq_tree_recluster(self._h, C.byref(h)))
        return BloomTree(h, self.device)

    def merges(self) -> np.ndarray:
        """The merge log of a tree made by recluster() (pfq_tree_merges), one MERGE_DTYPE record per internal node in creation
        order: `node`, `left`, `right` number the source tree's leaves 0 .. L - 1 in its get_leaf_counts order and the internal
        nodes from L on; `round`, `n_leaves`, `score_sum`, `pairs`: the merge happened at similarity score_sum / (pairs * 2**20).
        Empty for any other tree."""
        p = C.POINTER(_ffi.Merge)()
        n = C.c_uint64()
        r = C.c_uint32()
        _ffi.check(_ffi.lib().pfq_tree_merges(self._h, C.byref(p), C.byref(n), C.byref(r)))
        if not n.value:
            return np.zeros(0, dtype=MERGE_DTYPE)
        return np.frombuffer(C.string_at(p, n.value * C.sizeof(_ffi.Merge)), dtype=MERGE_DTYPE).copy()

    def merge_rounds(self) -> int:
        """Rounds the clustering behind this tree ran (0 for a tree not made by recluster(), and for one leaf)."""
        p = C.POINTER(_ffi.Merge)()
        n = C.c_uint64()
        r = C.c_uint32()
        _ffi.check(_ffi.lib().pfq_tree_merges(self._h, C.byref(p), C.byref(n), C.byref(r)))
        return int(r.value)

    def last_recluster(self) -> dict:
        """Of the last recluster() of this tree (pfq_debug_last_recluster): `scores_ms`, `rounds_ms`, `nearest_ms` — device
        milliseconds, measured only under set_option("PFQ_CLUSTER_TIME", "1") — `nearest_bytes` and `rounds`."""
        ms = (C.c_double * 3)()
        b = C.c_uint64()
        r = C.c_uint32()
        _ffi.check(_ffi.lib().pfq_debug_last_recluster(self._h, ms, C.byref(b), C.byref(r)))
        return {"scores_ms": ms[0], "rounds_ms": ms[1], "nearest_ms": ms[2], "nearest_bytes": int(b.value), "rounds": int(r.value)}

    def export_counts(self, d_dst: int, stream: int = 0) -> None:
        _ffi.check(_ffi.lib().pfq_leaf_counts_export(self._h, d_dst, stream))

    def import_counts(self, d_src: int, stream: int = 0) -> None:
        _ffi.check(_ffi.lib().pfq_leaf_counts_import(self._h, d_src, stream))

    def export_counts_delta(self, d_dst: int, stream: int = 0) -> None:
        """What this replica counted since it was opened / last reset, imported or reduced (counters - base)."""
        _ffi.check(_ffi.lib().pfq_leaf_counts_export_delta(self._h, d_dst, stream))

    def import_counts_delta(self, d_src: int, stream: int = 0) -> None:
        """counters = base + d_src (the sum of the ranks' deltas); that becomes the new base."""
        _ffi.check(_ffi.lib().pfq_leaf_counts_import_delta(self._h, d_src, stream))


def _lca_flags(lca: Optional[str], want_hits: bool, want_scores: bool) -> int:
    if lca is None:
        return 0
    if lca not in ("all", "best"):
        raise ValueError(f"lca must be None, 'all' or 'best', not {lca!r}")
    if lca == "all":
        return _ffi.WANT_LCA
    if not (want_hits and want_scores):
        raise ValueError("lca='best' needs the hits and their scores (want_hits=True, want_scores=True)")
    return _ffi.WANT_LCA | _ffi.LCA_BEST


def _best_flags(best: bool, want_hits: bool, want_scores: bool) -> int:
    if not best:
        return 0
    if not (want_hits and want_scores):
        raise ValueError("best=True needs the hits and their scores (want_hits=True, want_scores=True)")
    return _ffi.ROWS_BEST


def _sweep_flags(sweep: bool, want_hits: bool, want_scores: bool) -> int:
    if not sweep:
        return 0
    if not (want_hits and want_scores):
        raise ValueError("sweep=True needs the hits and their scores (want_hits=True, want_scores=True)")
    return _ffi.WANT_SWEEP


def _abundance_flags(abundance: bool, want_hits: bool) -> int:
    if not abundance:
        return 0
    if not want_hits:
        raise ValueError("abundance=True needs the hits (want_hits=True): the log holds the rows of the call's hit lists")
    return _ffi.WANT_ABUNDANCE


def _taxa_flags(taxa: bool, want_hits: bool) -> int:
    if not taxa:
        return 0
    if not want_hits:
        raise ValueError("taxa=True needs the hits (want_hits=True): a node is touched by whole rows of the call's hit lists")
    return _ffi.WANT_TAXA


def _taxon_rows(p, n: int) -> List[Tuple[int, int, int, int, int, str]]:
    def idx(x):
        return -1 if x == _ffi.NO_CLADE else int(x)
    return [(idx(p[i].parent), int(p[i].depth), int(p[i].first_rank), int(p[i].n_leaves), idx(p[i].leaf), p[i].name.decode()) for i in range(n)]


def db_leaf_ids(directory: str) -> List[str]:
    """The tax_ids of a database's leaves in get_leaf_counts order, from tree.bin alone (pfq_db_leaf_ids); needs no device."""
    ids = C.POINTER(C.c_char_p)()
    n = C.c_uint64()
    _ffi.check(_ffi.lib().pfq_db_leaf_ids(directory.encode(), C.byref(ids), C.byref(n)))
    return [ids[i].decode() for i in range(n.value)]


GZ_STOPS = ("end", "limit", "more", "foreign")


def _gz_members(m: "_ffi.GzMembers") -> dict:
    n = int(m.n_members)
    return {"n_members": n, "consumed": int(m.consumed), "text_bytes": int(m.text_bytes), "stop": GZ_STOPS[m.stop],
            "begin": np.ctypeslib.as_array(m.begin, shape=(n + 1,)).copy(), "text_begin": np.ctypeslib.as_array(m.text_begin, shape=(n + 1,)).copy()}


def gz_scan(data: bytes, max_text: int = 0, final: bool = True) -> dict:
    """The members of blocked gzip (BGZF) bytes found by walking their headers (pfq_gz_scan; the rules are pfq.h "blocked gzip");
    needs no device.  Members are taken from data[0] while they are BGZF members and their text stays within `max_text` (0: no
    limit).  Returns n_members, consumed, text_bytes, stop ("end", "limit", "more": the next member is not all there, "foreign":
    what follows is no BGZF member, or with `final` a truncated one), begin and text_begin: uint64[n_members + 1]."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = _ffi.GzMembers()
    _ffi.check(_ffi.lib().pfq_gz_scan(buf.ctypes.data if buf.size else None, buf.size, max_text, _ffi.TEXT_FINAL if final else 0, C.byref(out)))
    return _gz_members(out)


def read_taxonomy(path: str, leaf_ids: Sequence[str]) -> Tuple[List[int], List[str], List[int]]:
    """A taxonomy file (`genome<TAB>lineage` per line, the lineage a ';'-separated list of names from the top rank down; see
    pfq_taxonomy_read in include/pfq.h) for the leaves named `leaf_ids`: (taxon_parent, taxon_names, leaf_taxon) as
    BloomTree.set_taxonomy takes them (the root's parent is -1).  Needs no device.  A bad file raises PfqError."""
    ids = (C.c_char_p * max(len(leaf_ids), 1))(*[t.encode() for t in leaf_ids])
    out = _ffi.TaxonomyFile()
    _ffi.check(_ffi.lib().pfq_taxonomy_read(path.encode(), ids, len(leaf_ids), C.byref(out)))
    nt, nl = int(out.n_taxa), int(out.n_leaves)
    parent = [-1 if out.taxon_parent[i] == _ffi.NO_CLADE else int(out.taxon_parent[i]) for i in range(nt)]
    return parent, [out.taxon_names[i].decode() for i in range(nt)], [int(out.leaf_taxon[l]) for l in range(nl)]


def taxonomy_nodes(leaf_ids: Sequence[str], taxon_parent: Sequence[int], taxon_names: Sequence[str],
                   leaf_taxon: Sequence[int]) -> List[Tuple[int, int, int, int, int, str]]:
    """The node table BloomTree.set_taxonomy would derive for leaves named `leaf_ids` (pfq_taxonomy_nodes), as BloomTree.taxa()
    returns it.  Needs no device."""
    ids = (C.c_char_p * max(len(leaf_ids), 1))(*[t.encode() for t in leaf_ids])
    names = (C.c_char_p * max(len(taxon_names), 1))(*[t.encode() for t in taxon_names])
    par = np.ascontiguousarray([_ffi.NO_CLADE if int(x) < 0 else int(x) for x in taxon_parent], dtype=np.uint32)
    leaf = np.ascontiguousarray(np.asarray(leaf_taxon, dtype=np.int64), dtype=np.uint32)
    p = C.POINTER(_ffi.Taxon)()
    n = C.c_uint64()
    _ffi.check(_ffi.lib().pfq_taxonomy_nodes(len(leaf_ids), ids, len(par), par.ctypes.data if par.size else None, names,
                                             leaf.ctypes.data if leaf.size else None, C.byref(p), C.byref(n)))
    return _taxon_rows(p, n.value)


def _coverage_flags(coverage: bool, want_hits: bool) -> int:
    if not coverage:
        return 0
    if not want_hits:
        raise ValueError("coverage=True needs the hits (want_hits=True): the genomes a read lists are the ones it is sketched for")
    return _ffi.WANT_COVERAGE


def _pair_flags(paired: bool, pair_mode: str) -> int:
    if pair_mode not in ("either", "both"):
        raise ValueError(f"pair_mode must be 'either' or 'both', not {pair_mode!r}")
    if not paired:
        return 0
    return _ffi.PAIRED | (_ffi.PAIR_BOTH if pair_mode == "both" else 0)


def query_batch(bloom_tree: BloomTree, read_set: Sequence[bytes], threshold: float,
                result_map: Optional[ResultMap] = None, read_ids: Optional[Sequence[str]] = None, best: bool = False) -> BloomTree:
    """query::query_batch (query.rs:66-82).  Leaf counts accumulate in the tree; when `result_map` is given
    (the reference fills it when reads carry their sequence, query.rs:146-154) every (read id, tax id) hit is added.
    `best`: the call also asks for hits and scores and reduces every read's row to its best-scoring genomes
    (bloom_tree.last_best_rows()); the leaf counts and `result_map` stay those of the whole rows."""
    seq, off = pack_reads(read_set)
    res = bloom_tree.query_packed(seq, off, threshold, want_hits=result_map is not None or best, want_scores=best, best=best)
    if result_map is not None:
        offs, leaves = res[:2]
        names = [t for t, _ in bloom_tree.get_leaf_counts()]
        for r in range(len(read_set)):
            rid = read_ids[r] if read_ids is not None else str(r)
            for j in range(int(offs[r]), int(offs[r + 1])):
                result_map.add_read_map(rid, names[int(leaves[j])])
    return bloom_tree


def get_leaf_counts(bloom_tree: BloomTree) -> List[Tuple[str, int]]:
    return bloom_tree.get_leaf_counts()


def save_leaf_counts(bloom_tree: BloomTree, path: str) -> None:
    bloom_tree.save_leaf_counts(path)


def allreduce_counts(trees: Sequence[BloomTree]) -> int:
    """Sum the per-leaf counters of replicas of one database (one per GPU, or several on one GPU) so that every replica
    holds the totals; returns the number of RCCL ranks used.  The in-process counterpart of dist.all_reduce_counts."""
    hs = (C.c_void_p * len(trees))(*[t._h for t in trees])
    _ffi.check(_ffi.lib().pfq_trees_allreduce_counts(hs, len(trees)))
    return int(_ffi.lib().pfq_last_allreduce_ranks())
