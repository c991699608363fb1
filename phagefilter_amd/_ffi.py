"""ctypes binding of libpfq (include/pfq.h).  No fallback: importing the product without the built HIP
library raises, and every compute call needs a gfx950 device."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (PFQ_LIBPFQ: another build of the library, for A/B measurements of two builds on one box)
LIB_PATH = os.environ.get("PFQ_LIBPFQ") or os.path.join(_HERE, "libpfq.so")

# every symbol include/pfq.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "pfq_tree_open", "pfq_tree_open_subtree", "pfq_db_shard_count", "pfq_tree_create", "pfq_tree_insert", "pfq_tree_build_balanced", "pfq_tree_build_balanced_device",
    "pfq_tree_build_balanced_subtree_device", "pfq_trees_allreduce_counts", "pfq_last_allreduce_ranks", "pfq_device_count", "pfq_set_option", "pfq_tree_save", "pfq_tree_info",
    "pfq_tree_prune", "pfq_tree_close", "pfq_query_batch", "pfq_query_batch_device", "pfq_last_hit_scores", "pfq_leaf_counts",
    "pfq_tree_clades", "pfq_clade_counts", "pfq_last_lca",
    "pfq_tree_set_taxonomy", "pfq_tree_taxa", "pfq_taxon_counts", "pfq_last_taxa", "pfq_last_best_rows", "pfq_db_leaf_ids", "pfq_taxonomy_read", "pfq_taxonomy_nodes",
    "pfq_abundance_estimate", "pfq_abundance_reset", "pfq_abundance_absorb",
    "pfq_coverage_get", "pfq_coverage_reset", "pfq_coverage_absorb",
    "pfq_tree_set_sweep", "pfq_sweep_get", "pfq_sweep_reset", "pfq_sweep_absorb",
    "pfq_query_frames", "pfq_query_frames_device",
    "pfq_text_parse", "pfq_text_query", "pfq_debug_text_csr", "pfq_text_format", "pfq_debug_last_format",
    "pfq_gz_scan", "pfq_text_inflate", "pfq_text_parse_inflated", "pfq_text_read", "pfq_debug_last_inflate",
    "pfq_bgzf_deflate", "pfq_text_format_gz", "pfq_debug_last_deflate",
    "pfq_prep_reads", "pfq_prep_query", "pfq_debug_prep_csr", "pfq_debug_last_prep",
    "pfq_tree_set_adapters", "pfq_prep_last_adapters", "pfq_debug_last_adapters",
    "pfq_tree_set_mate_overlap", "pfq_prep_last_overlap", "pfq_debug_last_overlap",
    "pfq_tree_set_mate_correct", "pfq_prep_last_corrections", "pfq_debug_last_corrections",
    "pfq_prep_deplete", "pfq_debug_last_deplete",
    "pfq_tree_similarity", "pfq_tree_recluster", "pfq_tree_merges",
    "pfq_save_leaf_counts", "pfq_leaf_counts_export", "pfq_leaf_counts_import", "pfq_leaf_counts_reset",
    "pfq_leaf_counts_export_delta", "pfq_leaf_counts_import_delta",
    "pfq_last_stats", "pfq_set_path", "pfq_profile_begin", "pfq_profile_end", "pfq_debug_kmer_indices", "pfq_debug_node_filter", "pfq_debug_last_capacity", "pfq_debug_last_similarity", "pfq_debug_last_recluster",
    "pfq_tile_lists_info", "pfq_debug_tile_list", "pfq_debug_tile_bucket", "pfq_screen_info", "pfq_pair_info",
    "pfq_synth_genomes_device",
    "pfq_synth_reads_device", "pfq_host_alloc", "pfq_host_free", "pfq_last_error", "pfq_version",
]


class PfqError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libpfq error {code}: {msg}")
        self.code = code


class Info(C.Structure):
    _fields_ = [("kmer_size", C.c_uint64), ("nbits", C.c_uint64), ("num_hashes", C.c_uint32),
                ("largest_expected_genome", C.c_uint32), ("false_pos_rate", C.c_float),
                ("superset_verified", C.c_uint32), ("seed1", C.c_uint64), ("seed2", C.c_uint64),
                ("n_nodes", C.c_uint64), ("n_leaves", C.c_uint64), ("n_filters", C.c_uint64),
                ("device_bytes", C.c_uint64), ("shard_first_leaf", C.c_uint64), ("tree_leaves", C.c_uint64)]


class Hits(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("offsets", C.POINTER(C.c_uint64)), ("leaves", C.POINTER(C.c_uint32))]


class Stats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_candidates", C.c_uint64), ("n_hits", C.c_uint64),
                ("n_allhit_reads", C.c_uint64), ("algorithmic_bytes", C.c_uint64), ("path", C.c_uint32),
                ("n_slices", C.c_uint32), ("tile_mode", C.c_uint32), ("n_fallback_pairs", C.c_uint32),
                ("n_chunks", C.c_uint64), ("tile_entries", C.c_uint64), ("tile_passes_launched", C.c_uint32),
                ("tile_passes_needed", C.c_uint32), ("leaf_groups", C.c_uint32), ("coarse_cols", C.c_uint32),
                ("coarse_probes", C.c_uint32), ("tile_bin_build", C.c_uint32), ("group_reads", C.c_uint64),
                ("pair_stage", C.c_uint32), ("entry_pack", C.c_uint32)]


class Profile(C.Structure):
    _fields_ = [("calls", C.c_uint64), ("classify_ms", C.c_double), ("bucket_ms", C.c_double), ("bin_ms", C.c_double),
                ("test_ms", C.c_double), ("verify_ms", C.c_double), ("finalize_ms", C.c_double)]


class Clade(C.Structure):
    _fields_ = [("parent", C.c_uint32), ("depth", C.c_uint32), ("first_leaf", C.c_uint32), ("n_leaves", C.c_uint32),
                ("name", C.c_char_p)]


class Taxon(C.Structure):
    _fields_ = [("parent", C.c_uint32), ("depth", C.c_uint32), ("first_rank", C.c_uint32), ("n_leaves", C.c_uint32),
                ("leaf", C.c_uint32), ("name", C.c_char_p)]


class TaxonomyFile(C.Structure):
    _fields_ = [("n_taxa", C.c_uint64), ("taxon_parent", C.POINTER(C.c_uint32)), ("taxon_names", C.POINTER(C.c_char_p)),
                ("n_leaves", C.c_uint64), ("leaf_taxon", C.POINTER(C.c_uint32)), ("lines_considered", C.c_uint64),
                ("lines_other", C.c_uint64), ("leaves_without_line", C.c_uint64)]


class Abundance(C.Structure):
    _fields_ = [("n_leaves", C.c_uint64), ("mass", C.POINTER(C.c_uint64)), ("unique", C.POINTER(C.c_uint64)),
                ("n_units", C.c_uint64), ("n_unhit", C.c_uint64), ("n_unique", C.c_uint64), ("n_ambiguous", C.c_uint64),
                ("n_all_leaves", C.c_uint64), ("n_entries", C.c_uint64), ("last_delta", C.c_uint64),
                ("iterations", C.c_uint32), ("converged", C.c_uint32)]


class Coverage(C.Structure):
    _fields_ = [("n_leaves", C.c_uint64), ("n_units", C.c_uint64), ("precision", C.c_uint32),
                ("registers", C.POINTER(C.c_uint8)),
                ("units", C.POINTER(C.c_uint64)), ("matched", C.POINTER(C.c_uint64)), ("filter_bits", C.POINTER(C.c_uint64)),
                ("distinct", C.POINTER(C.c_double)), ("genome_kmers", C.POINTER(C.c_double))]


class Sweep(C.Structure):
    _fields_ = [("n_thresholds", C.c_uint32), ("thresholds", C.POINTER(C.c_float)), ("n_leaves", C.c_uint64), ("n_units", C.c_uint64),
                ("leaf_units", C.POINTER(C.c_uint64)), ("leaf_unique", C.POINTER(C.c_uint64)),
                ("units_hit", C.POINTER(C.c_uint64)), ("units_unique", C.POINTER(C.c_uint64)), ("entries", C.POINTER(C.c_uint64)),
                ("genomes_hit", C.POINTER(C.c_uint64))]


class Segment(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("leaf", "first_frame", "n_frames", "begin", "end", "match_begin", "match_end", "kmers",
                                          "matched", "longest_run")]


class Segments(C.Structure):
    _fields_ = [("n_seqs", C.c_uint64), ("n_frames", C.c_uint64), ("offsets", C.POINTER(C.c_uint64)), ("seg", C.POINTER(Segment))]


class Text(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("consumed", C.c_uint64), ("n_bases", C.c_uint64), ("stop", C.c_uint32),
                ("rec_begin", C.POINTER(C.c_uint64))]


class GzMembers(C.Structure):
    _fields_ = [("n_members", C.c_uint64), ("consumed", C.c_uint64), ("text_bytes", C.c_uint64), ("stop", C.c_uint32),
                ("begin", C.POINTER(C.c_uint64)), ("text_begin", C.POINTER(C.c_uint64))]


class TextInflated(C.Structure):
    _fields_ = [("members", GzMembers), ("n_good", C.c_uint64), ("good_text", C.c_uint64), ("status", C.POINTER(C.c_uint8))]


class TextLeft(C.Structure):
    _fields_ = [("first", C.c_uint64), ("count", C.c_uint64), ("pos_at", C.c_uint64), ("neg_at", C.c_uint64),
                ("why", C.c_uint32), ("pad_", C.c_uint32)]


class TextRecords(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("pos_records", C.c_uint64), ("neg_records", C.c_uint64),
                ("pos_bytes", C.c_uint64), ("neg_bytes", C.c_uint64), ("pos", C.POINTER(C.c_uint8)), ("neg", C.POINTER(C.c_uint8)),
                ("n_left", C.c_uint64), ("left", C.POINTER(TextLeft))]


class Bgzf(C.Structure):
    _fields_ = [("gz", C.POINTER(C.c_uint8)), ("gz_bytes", C.c_uint64), ("n_members", C.c_uint64), ("n_pieces", C.c_uint64),
                ("piece_begin", C.POINTER(C.c_uint64)), ("member_begin", C.POINTER(C.c_uint64))]


class PrepParams(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("trim_quality", "trim_window", "poly_x", "min_length", "max_n", "min_complexity", "flags")]


class Prep(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_kept", C.c_uint64), ("bases_in", C.c_uint64), ("bases_kept", C.c_uint64),
                ("n_trimmed", C.c_uint64), ("n_reason", C.c_uint64 * 5),
                ("begin", C.POINTER(C.c_uint32)), ("len", C.POINTER(C.c_uint32)), ("reason", C.POINTER(C.c_uint32)),
                ("kept", C.POINTER(C.c_uint32))]


ADAPTER_MAX, ADAPTER_LEN_MAX, ADAPTER_NONE = 8, 64, 0xFF


class PrepAdapters(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_found", C.c_uint64), ("bases_cut", C.c_uint64), ("found", C.c_uint64 * (2 * ADAPTER_MAX)),
                ("cut", C.POINTER(C.c_uint32)), ("which", C.POINTER(C.c_uint8))]


OVERLAP_LEN_MAX, OVERLAP_INSERT_MAX, NO_INSERT = 512, 1024, 0xFFFFFFFF


class PrepOverlap(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_fragments", "n_analysed", "n_skipped", "n_overlapped", "n_readthrough", "reads_cut", "bases_cut")] + [
                ("hist", C.POINTER(C.c_uint64)), ("insert", C.POINTER(C.c_uint32)), ("mismatches", C.POINTER(C.c_uint32))]


MATE_CORRECT_HIGH, MATE_CORRECT_LOW = 30, 14


class PrepPatch(C.Structure):
    _fields_ = [("read", C.c_uint32), ("pos", C.c_uint32), ("base", C.c_uint8), ("qual", C.c_uint8), ("old_base", C.c_uint8), ("old_qual", C.c_uint8)]


class PrepCorrections(C.Structure):
    _fields_ = [("n_fragments_corrected", C.c_uint64), ("n_bases", C.c_uint64 * 2), ("n_unresolved", C.c_uint64), ("n_no_quality", C.c_uint64),
                ("n_patches", C.c_uint64), ("patches", C.POINTER(PrepPatch))]


PREP_DEPLETED = 5


class PrepDepleted(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_units", "units_removed", "reads_removed", "bases_removed", "n_kept", "bases_kept")] + [
                ("kept", C.POINTER(C.c_uint32)), ("reason", C.POINTER(C.c_uint32))]


class Similarity(C.Structure):
    _fields_ = [("n_a", C.c_uint64), ("n_b", C.c_uint64), ("shared_bits", C.POINTER(C.c_uint32)),
                ("bits_a", C.POINTER(C.c_uint64)), ("bits_b", C.POINTER(C.c_uint64)),
                ("kmers_a", C.POINTER(C.c_double)), ("kmers_b", C.POINTER(C.c_double)),
                ("shared_kmers", C.POINTER(C.c_double)), ("jaccard", C.POINTER(C.c_double))]


class Merge(C.Structure):
    _fields_ = [("node", C.c_uint32), ("left", C.c_uint32), ("right", C.c_uint32), ("round", C.c_uint32), ("n_leaves", C.c_uint32),
                ("pad_", C.c_uint32), ("score_sum", C.c_uint64), ("pairs", C.c_uint64)]


WANT_HITS = 1
WANT_SCORES = 2
PAIRED = 4
PAIR_BOTH = 8
WANT_LCA = 16
LCA_BEST = 32
WANT_ABUNDANCE = 64
ABUND_Q = 16
WANT_COVERAGE = 128
WANT_TAXA = 256
ROWS_BEST = 512
WANT_SWEEP = 1024
SWEEP_MAX = 16
NO_CLADE = 0xFFFFFFFF
TEXT_FASTA, TEXT_FASTQ = 0, 1
TEXT_FINAL, TEXT_WANT_RECORDS = 1, 2
TEXT_END, TEXT_LIMIT, TEXT_MORE, TEXT_SLOW = 0, 1, 2, 3
GZ_MEMBER_TEXT_MAX = 65536
GZ_END, GZ_LIMIT, GZ_MORE, GZ_FOREIGN = 0, 1, 2, 3
GZ_OK, GZ_MALFORMED, GZ_LENGTH, GZ_CRC = 0, 1, 2, 3
FMT_POS, FMT_NEG, FMT_BLOCK_MAX = 1, 2, 8192
LEFT_HEAD, LEFT_TAIL, LEFT_REPEATED_ID = 1, 2, 3
PREP_PAIRED, PREP_WANT_READS = 1, 2
PREP_KEPT, PREP_SHORT, PREP_N, PREP_COMPLEXITY, PREP_MATE = 0, 1, 2, 3, 4
PREP_MAX_N_OFF = 0xFFFFFFFF
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C phagefilter_amd/csrc` "
                          "(or __graft_entry__.build()); phagefilter_amd has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u8p, u64p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    L.pfq_last_error.restype = C.c_char_p
    L.pfq_version.restype = C.c_char_p
    L.pfq_tree_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.pfq_tree_open_subtree.argtypes = [C.c_char_p, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.pfq_db_shard_count.argtypes = [C.c_char_p, C.c_uint64, u64p]
    L.pfq_tree_build_balanced.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64, C.c_uint64,
                                          C.c_uint32, C.c_uint64, C.c_uint64, C.c_float, C.c_uint32, C.c_int,
                                          C.POINTER(vp)]
    L.pfq_tree_build_balanced_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64,
                                                 C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_float, C.c_uint32,
                                                 C.c_int, C.POINTER(vp)]
    L.pfq_tree_build_balanced_subtree_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64,
                                                         C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_float, C.c_uint32,
                                                         C.c_uint64, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.pfq_trees_allreduce_counts.argtypes = [C.POINTER(vp), C.c_uint32]
    L.pfq_last_allreduce_ranks.restype = C.c_uint32
    L.pfq_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.pfq_tree_create.argtypes = [C.c_uint64, C.c_float, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.pfq_tree_insert.argtypes = [vp, vp, C.c_uint64, C.c_char_p, C.c_char_p]
    L.pfq_host_alloc.argtypes = [C.c_uint64, C.POINTER(vp)]
    L.pfq_host_free.argtypes = [vp]
    L.pfq_tree_save.argtypes = [vp, C.c_char_p]
    L.pfq_tree_info.argtypes = [vp, C.POINTER(Info)]
    L.pfq_tree_prune.argtypes = [vp, C.c_uint64]
    L.pfq_tree_close.argtypes = [vp]
    L.pfq_tree_close.restype = None
    L.pfq_query_batch.argtypes = [vp, vp, vp, C.c_uint64, C.c_float, C.c_uint32, C.POINTER(Hits)]
    L.pfq_query_batch_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_float, C.c_uint32, vp, C.POINTER(Hits)]
    L.pfq_last_hit_scores.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint32)), u64p]
    L.pfq_tree_clades.argtypes = [vp, C.POINTER(C.POINTER(Clade)), u64p]
    L.pfq_clade_counts.argtypes = [vp, C.POINTER(u64p), C.POINTER(u64p), u64p]
    L.pfq_last_lca.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint32)), u64p]
    u32p = C.POINTER(C.c_uint32)
    L.pfq_tree_set_taxonomy.argtypes = [vp, C.c_uint64, vp, C.POINTER(C.c_char_p), vp]
    L.pfq_tree_taxa.argtypes = [vp, C.POINTER(C.POINTER(Taxon)), u64p]
    L.pfq_taxon_counts.argtypes = [vp, C.POINTER(u64p), C.POINTER(u64p), C.POINTER(u64p), u64p]
    L.pfq_last_taxa.argtypes = [vp, C.POINTER(u32p), u64p]
    L.pfq_last_best_rows.argtypes = [vp, C.POINTER(Hits)]
    L.pfq_db_leaf_ids.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_char_p)), u64p]
    L.pfq_taxonomy_read.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(TaxonomyFile)]
    L.pfq_taxonomy_nodes.argtypes = [C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64, vp, C.POINTER(C.c_char_p), vp,
                                     C.POINTER(C.POINTER(Taxon)), u64p]
    L.pfq_abundance_estimate.argtypes = [vp, C.c_uint32, C.c_uint64, C.POINTER(Abundance)]
    L.pfq_abundance_reset.argtypes = [vp]
    L.pfq_abundance_absorb.argtypes = [vp, vp]
    L.pfq_coverage_get.argtypes = [vp, C.POINTER(Coverage)]
    L.pfq_coverage_reset.argtypes = [vp]
    L.pfq_coverage_absorb.argtypes = [vp, vp]
    L.pfq_tree_set_sweep.argtypes = [vp, C.POINTER(C.c_float), C.c_uint32]
    L.pfq_sweep_get.argtypes = [vp, C.POINTER(Sweep)]
    L.pfq_sweep_reset.argtypes = [vp]
    L.pfq_sweep_absorb.argtypes = [vp, vp]
    L.pfq_query_frames.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.POINTER(Segments)]
    L.pfq_query_frames_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, vp,
                                          C.POINTER(Segments)]
    L.pfq_text_parse.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(Text)]
    L.pfq_text_query.argtypes = [vp, C.c_float, C.c_uint32, C.POINTER(Hits)]
    L.pfq_debug_text_csr.argtypes = [vp, vp, vp]
    L.pfq_text_format.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(TextRecords)]
    L.pfq_debug_last_format.argtypes = [vp, C.POINTER(C.c_double)]
    L.pfq_gz_scan.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(GzMembers)]
    L.pfq_text_inflate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(TextInflated)]
    L.pfq_text_parse_inflated.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(Text)]
    L.pfq_text_read.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    L.pfq_debug_last_inflate.argtypes = [vp, C.POINTER(C.c_double)]
    L.pfq_bgzf_deflate.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(Bgzf)]
    L.pfq_text_format_gz.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(TextRecords), C.POINTER(Bgzf), C.POINTER(Bgzf)]
    L.pfq_debug_last_deflate.argtypes = [vp, C.POINTER(C.c_double)]
    L.pfq_prep_reads.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(PrepParams), C.POINTER(Prep)]
    L.pfq_prep_query.argtypes = [vp, C.c_float, C.c_uint32, C.POINTER(Hits)]
    L.pfq_debug_prep_csr.argtypes = [vp, vp, vp]
    L.pfq_debug_last_prep.argtypes = [vp, C.POINTER(C.c_double)]
    L.pfq_tree_set_adapters.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_uint32]
    L.pfq_prep_last_adapters.argtypes = [vp, C.POINTER(PrepAdapters)]
    L.pfq_debug_last_adapters.argtypes = [vp, C.POINTER(C.c_double)]
    L.pfq_tree_set_mate_overlap.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.pfq_prep_last_overlap.argtypes = [vp, C.POINTER(PrepOverlap)]
    L.pfq_debug_last_overlap.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "pfq_tree_set_mate_correct"):  # (an older build chosen through PFQ_LIBPFQ for an A/B has no mate correction)
        L.pfq_tree_set_mate_correct.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.pfq_prep_last_corrections.argtypes = [vp, C.POINTER(PrepCorrections)]
        L.pfq_debug_last_corrections.argtypes = [vp, C.POINTER(C.c_double)]
    L.pfq_prep_deplete.argtypes = [vp, vp, C.c_float, C.c_uint32, C.POINTER(PrepDepleted)]
    L.pfq_debug_last_deplete.argtypes = [vp, C.POINTER(C.c_double)]
    L.pfq_tree_similarity.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(Similarity)]
    L.pfq_debug_last_similarity.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.pfq_tree_recluster.argtypes = [vp, C.POINTER(vp)]
    L.pfq_tree_merges.argtypes = [vp, C.POINTER(C.POINTER(Merge)), u64p, C.POINTER(C.c_uint32)]
    L.pfq_debug_last_recluster.argtypes = [vp, C.POINTER(C.c_double), u64p, C.POINTER(C.c_uint32)]
    L.pfq_leaf_counts.argtypes = [vp, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(u64p), u64p]
    L.pfq_save_leaf_counts.argtypes = [vp, C.c_char_p]
    L.pfq_leaf_counts_export.argtypes = [vp, vp, vp]
    L.pfq_leaf_counts_import.argtypes = [vp, vp, vp]
    L.pfq_leaf_counts_export_delta.argtypes = [vp, vp, vp]
    L.pfq_leaf_counts_import_delta.argtypes = [vp, vp, vp]
    L.pfq_leaf_counts_reset.argtypes = [vp]
    L.pfq_last_stats.argtypes = [vp, C.POINTER(Stats)]
    L.pfq_set_path.argtypes = [vp, C.c_int]
    L.pfq_profile_begin.argtypes = [vp, C.c_uint32]
    L.pfq_profile_end.argtypes = [vp, C.POINTER(Profile)]
    L.pfq_debug_kmer_indices.argtypes = [vp, vp, C.c_uint64, vp, u64p]
    L.pfq_debug_node_filter.argtypes = [vp, C.c_uint64, vp, C.c_uint64]
    L.pfq_debug_last_capacity.argtypes = [vp, vp, C.c_uint64]
    if hasattr(L, "pfq_tile_lists_info"):  # (an older build chosen through PFQ_LIBPFQ for an A/B has no position slots)
        L.pfq_tile_lists_info.argtypes = [vp, vp]
        L.pfq_debug_tile_list.argtypes = [vp, C.c_uint64, C.c_uint64, vp, C.c_uint64]
    if hasattr(L, "pfq_debug_tile_bucket"):  # (likewise: an older build has no bucket read-back)
        L.pfq_debug_tile_bucket.argtypes = [vp, C.c_uint64, C.c_uint64, vp, C.c_uint64]
    if hasattr(L, "pfq_screen_info"):  # (likewise: an older build has one dense screen)
        L.pfq_screen_info.argtypes = [vp, vp]
    if hasattr(L, "pfq_pair_info"):  # (likewise: an older build reserves pair slots one pass at a time)
        L.pfq_pair_info.argtypes = [vp, vp]
    L.pfq_synth_genomes_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    L.pfq_synth_reads_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint64,
                                         C.c_uint64, vp]
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        raise PfqError(rc, lib().pfq_last_error().decode(errors="replace"))


def source_stamp() -> str:
    """sha256 over the sources of libpfq (csrc/*.hip, *.cpp, *.h + include/pfq.h): stamps measurements that are taken in a
    separate pass (profiles/pmc_traffic.json) so that bench.py can tell whether they still describe the code it runs."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")) +
                   glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(os.path.dirname(_HERE), "include", "pfq.h")])
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]
