/*
 * pfq.h — C ABI of libpfq: MI355X-native read classification against a PhageFilter Sequence Bloom Tree.
 *
 * This is the drop-in boundary for ONE path of Dreycey/PhageFilter: `phage_filter query`
 * (src/main.rs:249-376 -> src/query.rs:66-158).  The reference has no FFI of its own; each entry point
 * below replaces the in-process call a Rust `main.rs` makes at that seam and is what its FFI (`extern "C"`
 * block) would bind.  Paths are relative to the reference repository root.
 *
 * Conventions: every function returns PFQ_OK (0) or a negative pfq_status; nothing unwinds across the
 * boundary; `pfq_last_error()` gives the message of the last failure on the calling thread.  The caller owns
 * every input buffer; outputs marked "library-owned" stay valid until the next call on the same tree.
 * One calling thread per pfq_tree (the reference's block loop is serial, main.rs:334-368).
 * There is NO CPU fallback: every entry point that computes needs a gfx950 device and fails with
 * PFQ_ERR_DEVICE otherwise.
 */
#ifndef PFQ_H
#define PFQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pfq_status {
    PFQ_OK = 0,
    PFQ_ERR_ARG = -1,         /* bad argument */
    PFQ_ERR_IO = -2,          /* file missing / unreadable (reference: panic in bloom_tree.rs:375-379, bloom_filter.rs:155-168) */
    PFQ_ERR_FORMAT = -3,      /* tree.bin / .bf does not parse or is inconsistent */
    PFQ_ERR_UNSUPPORTED = -4, /* valid database outside the device path's limits */
    PFQ_ERR_DEVICE = -5,      /* HIP error / no gfx950 device */
    PFQ_ERR_STATE = -6        /* call order (e.g. query on an empty tree) */
} pfq_status;

typedef struct pfq_tree pfq_tree; /* BloomTree (bloom_tree.rs:29-48) + its filters, resident in HBM */

/* Tree-wide parameters: BloomTree fields (bloom_tree.rs:39-47) + the per-filter constants every node shares
 * (bloom_filter.rs:86-89; identical for all nodes because bloom_tree.rs:279-290 builds every filter alike). */
typedef struct pfq_info {
    uint64_t kmer_size;
    uint64_t nbits;
    uint32_t num_hashes;
    uint32_t largest_expected_genome;
    float false_pos_rate;
    uint32_t superset_verified; /* 1: parent ⊇ child holds on every edge (checked on the device at load) */
    uint64_t seed1, seed2;
    uint64_t n_nodes, n_leaves, n_filters;
    uint64_t device_bytes; /* HBM held by this tree */
    uint64_t shard_first_leaf; /* subtree shards: position of this shard's first leaf in the whole tree's leaf order */
    uint64_t tree_leaves;      /* leaves of the whole tree (== n_leaves unless this is a subtree shard) */
} pfq_info;

/* Per-read results of one pfq_query_batch call: CSR read -> leaf indices (indices into pfq_leaf_counts'
 * left-to-right leaf order).  Replaces ResultMap (result_map.rs:9-46) at the seam of query.rs:146-154. */
typedef struct pfq_hits {
    uint64_t n_reads;
    const uint64_t *offsets; /* [n_reads + 1], library-owned */
    const uint32_t *leaves;  /* [offsets[n_reads]], ascending within a read, library-owned */
} pfq_hits;

#define PFQ_WANT_HITS 1u /* fill pfq_hits (needed for POS/NEG filtering, main.rs:345-361) */
#define PFQ_WANT_SCORES 2u /* also score every hit (pfq_last_hit_scores); only together with PFQ_WANT_HITS, alone: PFQ_ERR_ARG */
/* Paired-end reads: reads 2i and 2i + 1 are the two mates of fragment i (an odd n_reads is PFQ_ERR_ARG).  Each mate is
 * classified on its own, exactly like an unpaired read (its own n_kmers and need); the fragment's hit set is the union of the
 * mates' sets, or with PFQ_PAIR_BOTH their intersection (a mate shorter than k passes every leaf: `either` gives every leaf,
 * `both` the other mate's set).  The leaf counters count fragments, one per leaf of the fragment's set; pfq_hits has one row
 * per fragment (n_reads / 2); pfq_last_hit_scores gives per (fragment, listed leaf) the matched k-mers of both mates summed,
 * each counted on that leaf's own filter.  Without PFQ_WANT_HITS the call returns once the mates' hit lists are checked and
 * the fragment kernels are queued. */
#define PFQ_PAIRED 4u
#define PFQ_PAIR_BOTH 8u /* only together with PFQ_PAIRED, alone: PFQ_ERR_ARG */
/* Lowest common ancestor: every unit of the call (a read; with PFQ_PAIRED a fragment) is also assigned to the deepest clade
 * that is an ancestor-or-self of every leaf of its hit set — exactly the row pfq_hits gives for it (pfq_last_lca), and that
 * clade's counter grows by one (pfq_clade_counts).  Combines with every other flag and changes none of their results.  Without
 * PFQ_WANT_HITS the call returns once the hit list is checked and the LCA kernels are queued.  Subtree shards:
 * PFQ_ERR_UNSUPPORTED (a shard does not hold the other shards' topology). */
#define PFQ_WANT_LCA 16u
/* The LCA is taken over the hits whose score (pfq_last_hit_scores) is the unit's highest; ties stay ambiguous.  Only together
 * with PFQ_WANT_LCA | PFQ_WANT_HITS | PFQ_WANT_SCORES, else PFQ_ERR_ARG. */
#define PFQ_LCA_BEST 32u
#define PFQ_NO_CLADE 0xffffffffu /* pfq_last_lca: the unit hit nothing */
/* Abundance: every unit of the call (a read; with PFQ_PAIRED a fragment) is also logged on the device for pfq_abundance_estimate
 * — exactly the row pfq_hits gives for it.  Only together with PFQ_WANT_HITS (alone: PFQ_ERR_ARG); combines with every other
 * flag and changes none of their results.  A block whose hit buffer overflowed and ran again is logged once.  Subtree shards:
 * PFQ_ERR_UNSUPPORTED (a shard sees only its own leaves, so its rows would be partial).  A call whose rows do not fit the log
 * (PFQ_ABUND_SLOTS, device memory, more than 2^32 - 1 units in all) returns PFQ_ERR_UNSUPPORTED with a message that names the
 * log: its other results (counts, hits, scores, LCAs) stand, the log keeps what it held and is incomplete until it is reset. */
#define PFQ_WANT_ABUNDANCE 64u
#define PFQ_ABUND_Q 16 /* pfq_abundance.mass counts units in steps of 2^-16 */
/* Coverage: every unit of the call (a read; with PFQ_PAIRED a fragment) is also sketched on the device for pfq_coverage_get: per
 * leaf of the row pfq_hits gives for it, the unit, its matched k-mers and a HyperLogLog sketch of them (see "coverage" below).
 * Only together with PFQ_WANT_HITS (alone: PFQ_ERR_ARG); combines with every other flag and changes none of their results.  A
 * block whose hit buffer overflowed and ran again is sketched once.  Subtree shards are accepted: a leaf's sketch depends only
 * on the units that list that leaf, so a shard's sketch of its leaves is the whole tree's sketch of those leaves.  The sketch is
 * allocated and zeroed by the first such call; if that fails the call returns PFQ_ERR_DEVICE and nothing of it is sketched. */
#define PFQ_WANT_COVERAGE 128u

/* ---- database ---- */

/* BloomTree::load (bloom_tree.rs:364-386) + every BloomFilter::load_from_file the LRU cache would do lazily
 * (cache.rs:56-77, bloom_filter.rs:153-174): parses <db_dir>/tree.bin and each node's .bf (filters are keyed
 * by their relative path exactly like the cache), uploads them, verifies parent ⊇ child per edge and builds
 * the device layout.  `device` = HIP device ordinal. */
int pfq_tree_open(const char *db_dir, int device, pfq_tree **out);

/* Subtree shard of a database, for trees larger than one GPU's HBM (BASELINE config 5): the shards
 * are the nodes of the depth-`depth` frontier in left-to-right order (nodes at that depth, plus leaves above it).
 * Shard `index` keeps that node, everything below it and the chain of its ancestors, each reduced to the child on
 * the path; only those .bf files are read.  Every rank classifies ALL reads against its shard; the shards' leaf
 * ranges are disjoint and contiguous in the whole tree's leaf order (pfq_info.shard_first_leaf), so the whole
 * job's counts are the concatenation of the shards' counts.  Ancestors that are not verified supersets become
 * guard columns, so results equal the reference's whole-tree traversal. */
int pfq_tree_open_subtree(const char *db_dir, int device, uint64_t depth, uint64_t index, pfq_tree **out);

/* Number of subtree shards of <db_dir> at depth `depth`: the size of the depth-`depth` frontier that
 * pfq_tree_open_subtree indexes (nodes at that depth, plus leaves above it).  Reads tree.bin only; no .bf file is
 * read and no device is used.  PFQ_ERR_IO: tree.bin missing or unreadable; PFQ_ERR_FORMAT: it does not parse;
 * PFQ_ERR_STATE: the tree is empty. */
int pfq_db_shard_count(const char *db_dir, uint64_t depth, uint64_t *n_shards);

/* The reference's `build` / `add` (main.rs:148-247) on the device.
 * pfq_tree_create = BloomTree::new (bloom_tree.rs:100-118): an empty tree; filter geometry from
 *   (false_pos_rate, largest_expected_genome) exactly like with_rate (bloom_filter.rs:229-240,:342-357, f32 arithmetic);
 *   the two hash seeds are explicit (the reference draws them at random, hasher.rs:24-30).  expected_genomes sizes the
 *   filter storage up front (2n-1 rows); 0 = grow on demand.
 * pfq_tree_insert = BloomTree::insert (bloom_tree.rs:128-143): a leaf filter holding every canonical k-mer of `seq`
 *   (:154-168), then the greedy descent (:187-214): every two-child node on the way absorbs the new filter and the walk
 *   continues into the child at smaller Hamming distance (right only if strictly smaller, :201); the leaf reached is
 *   replaced by a new internal node (left = old leaf, right = new leaf, filter = union, :226-245).  internal_name
 *   names that node (tax_id, "<name>.bf"); NULL = "Internal_Node_<n>" with a running n unique in the tree (the
 *   reference draws a random u16, :231-233).  Works on trees from pfq_tree_open as well (`add`).
 *   An insertion that fails (a node with one child on the walk: PFQ_ERR_FORMAT, the reference panics at :209; the
 *   device walk's barrier timing out: PFQ_ERR_DEVICE) may be reported by this call or, since the walk runs
 *   asynchronously, by the next call that needs the topology.  From then on the error persists until pfq_tree_close:
 *   pfq_tree_insert, pfq_tree_save, pfq_tree_prune, both query calls and every leaf-count call return the same code
 *   and message, and nothing is written.  pfq_tree_info and pfq_tree_close keep working. */
int pfq_tree_create(uint64_t kmer_size, float false_pos_rate, uint32_t largest_expected_genome, uint64_t seed1,
                    uint64_t seed2, uint64_t expected_genomes, int device, pfq_tree **out);
int pfq_tree_insert(pfq_tree *tree, const uint8_t *seq, uint64_t len, const char *tax_id, const char *internal_name);

/* Synthetic balanced SBT built on the device: leaf i = all canonical k-mers of genome i
 * (what bloom_tree.rs:154-168 inserts), internal = OR of children (bloom_tree.rs:238-239), complete-as-possible
 * balanced shape, leaf tax_id = tax_ids[i], internal tax_id = "Internal_Node_<n>".  genomes/offsets are HOST
 * buffers: genome i = genomes[offsets[i] .. offsets[i+1]).  NOT the reference's greedy `build`. */
int pfq_tree_build_balanced(const uint8_t *genomes, const uint64_t *offsets, uint64_t n_genomes,
                            const char *const *tax_ids, uint64_t kmer_size, uint64_t nbits, uint32_t num_hashes,
                            uint64_t seed1, uint64_t seed2, float false_pos_rate, uint32_t largest_expected_genome,
                            int device, pfq_tree **out);
/* Same, with genomes already in device memory (n_genomes x genome_len bytes, contiguous). */
int pfq_tree_build_balanced_device(const uint8_t *d_genomes, uint64_t genome_len, uint64_t n_genomes,
                                   const char *const *tax_ids, uint64_t kmer_size, uint64_t nbits,
                                   uint32_t num_hashes, uint64_t seed1, uint64_t seed2, float false_pos_rate,
                                   uint32_t largest_expected_genome, int device, pfq_tree **out);

/* One subtree shard of that synthetic tree without ever holding the whole tree (BASELINE config 5: 16 384 leaves =
 * 294 GB of filters, one 2048-leaf shard per GPU): the same topology and names as pfq_tree_build_balanced_device over all
 * n_genomes, reduced like pfq_tree_open_subtree(depth, index); the shard's subtree is built from its own genomes and every
 * ancestor on the chain holds the union of ALL genomes below it in the whole tree.  d_genomes: all n_genomes genomes. */
int pfq_tree_build_balanced_subtree_device(const uint8_t *d_genomes, uint64_t genome_len, uint64_t n_genomes,
                                           const char *const *tax_ids, uint64_t kmer_size, uint64_t nbits,
                                           uint32_t num_hashes, uint64_t seed1, uint64_t seed2, float false_pos_rate,
                                           uint32_t largest_expected_genome, uint64_t depth, uint64_t index, int device,
                                           pfq_tree **out);

/* BloomTree::save (bloom_tree.rs:339-355) + the .bf files BloomFilter::save_to_file writes
 * (bloom_filter.rs:176-205), so the reference binary can open a tree built here. */
int pfq_tree_save(const pfq_tree *tree, const char *db_dir);

int pfq_tree_info(const pfq_tree *tree, pfq_info *out);

/* BloomTree::prune_tree (bloom_tree.rs:302-330): nodes at depth >= search_depth become leaves. */
int pfq_tree_prune(pfq_tree *tree, uint64_t search_depth);

void pfq_tree_close(pfq_tree *tree);

/* ---- query ---- */

/* query::query_batch (query.rs:66-82) for one block of reads given as raw bytes: read i =
 * seq[offsets[i] .. offsets[i+1]) (HOST buffers).  k-mer extraction (file_parser.rs:135-148) happens on the
 * device.  Leaf counts accumulate across calls like BloomNode::mapped_reads (query.rs:143).  `hits` may be NULL
 * unless PFQ_WANT_HITS is set.  The input buffers may be reused as soon as the call returns.  Without
 * PFQ_WANT_HITS the call returns when the block has been copied and its kernels are queued (the copy of the next
 * block overlaps them); the calls that read results (pfq_leaf_counts, pfq_save_leaf_counts, pfq_last_stats,
 * pfq_tree_close) wait for the device. */
int pfq_query_batch(pfq_tree *tree, const uint8_t *seq, const uint64_t *offsets, uint64_t n_reads, float threshold,
                    uint32_t flags, pfq_hits *hits);

/* Same with the block already resident in HBM (device pointers) on HIP stream `stream` (hipStream_t, may be
 * NULL for the default stream).  total_bytes = offsets[n_reads], the size of the sequence buffer (0 if unknown:
 * the library then skips optimisations that need it).  Asynchronous unless PFQ_WANT_HITS is set; counts are final
 * after the stream is synchronised.  The tree's scratch buffers are reused call after call: calls on one stream are
 * ordered by it; a call on another stream than the previous one (pfq_query_batch uses the default stream) first waits
 * for that one.  This is the entry the benchmark times. */
int pfq_query_batch_device(pfq_tree *tree, const uint8_t *d_seq, const uint64_t *d_offsets, uint64_t n_reads,
                           uint64_t total_bytes, float threshold, uint32_t flags, void *stream, pfq_hits *hits);

/* Scores of the hits of the last pfq_query_batch[_device] call on `tree`, which must have set PFQ_WANT_SCORES (else
 * PFQ_ERR_ARG): scores[j] belongs to hits.leaves[j] of that call, n_hits = hits.offsets[n_reads].  The score of (read r,
 * hit leaf l) is num_matches of query_passes (query.rs:38-49) on l's filter: how many of get_kmers(r) (canonical k-mers,
 * duplicates counted, file_parser.rs:114-148) have all num_hashes probed bits set (bloom_filter.rs:312-332), between
 * ceil(threshold * n_kmers) and n_kmers = max(len - k + 1, 0).  The hits themselves are those of the same call without
 * PFQ_WANT_SCORES.  Library-owned; valid until the next query call on the tree.
 * "A query call", here and for pfq_last_lca, pfq_last_taxa, pfq_last_best_rows and pfq_text_format: every call of pfq_query_batch,
 * pfq_query_batch_device, pfq_text_query, pfq_prep_query, pfq_query_frames and pfq_query_frames_device whose tree (for the frames
 * calls also out, and for a non-empty block its buffers) is not NULL, and for the screen of a pfq_prep_deplete that is not refused.  Such a call ends the validity of what the one before it
 * left even when it is then refused: PFQ_ERR_ARG for a combination of flags, an odd PFQ_PAIRED block, PFQ_WANT_SWEEP above the
 * list's lowest threshold or with PFQ_PAIRED, PFQ_PAIRED on a block prepared unpaired, frames flags other than 0; PFQ_ERR_STATE for
 * PFQ_WANT_TAXA without a taxonomy, PFQ_WANT_SWEEP without a list, pfq_text_query before a parse, pfq_prep_query before a prep;
 * PFQ_ERR_UNSUPPORTED for a flag a subtree shard refuses or an abundance log that is full.  No refused call changes a counter, log
 * or sketch, except the one whose rows do not fit the abundance log: its other results stand (PFQ_WANT_ABUNDANCE).  Not query calls: pfq_text_parse, pfq_prep_reads,
 * pfq_text_format, the resets, the settings, pfq_tree_insert and pfq_tree_prune; they leave these results readable as the call
 * left them (clade and node indices then still number the tree and the taxonomy of that call). */
int pfq_last_hit_scores(pfq_tree *tree, const uint32_t **scores, uint64_t *n_hits);

/* ---- clades (PFQ_WANT_LCA) ----
 * The clades of a tree are the nodes reachable from its root as the tree currently is (after pfq_tree_prune, after
 * pfq_tree_insert), numbered in pre-order: node, left subtree, right subtree; the root is clade 0.  The index is the identity
 * of a clade; names may collide (the reference names internal nodes "Internal_Node_<random u16>"). */
typedef struct pfq_clade {
    uint32_t parent;     /* clade index; PFQ_NO_CLADE for the root */
    uint32_t depth;      /* edges from the root */
    uint32_t first_leaf; /* the clade's leaves are columns [first_leaf, first_leaf + n_leaves) of pfq_leaf_counts */
    uint32_t n_leaves;
    const char *name;    /* the node's tax_id; without one, its .bf file name without the suffix */
} pfq_clade;
/* The clade table: library-owned, valid until the topology next changes (pfq_tree_insert, pfq_tree_prune). */
int pfq_tree_clades(pfq_tree *tree, const pfq_clade **clades, uint64_t *n);
/* Per clade, here[c] = units whose LCA is c, accumulated over the PFQ_WANT_LCA calls like the leaf counters, and below[c] =
 * the sum of here over c's subtree (below[0] = units that hit anything).  They start at zero when a tree is opened or
 * created, are not stored by pfq_tree_save, and are zeroed by pfq_leaf_counts_reset, pfq_tree_prune and pfq_tree_insert.  A
 * block whose hit buffer overflowed and ran again counts once.  Waits for the device like pfq_leaf_counts.  Library-owned. */
int pfq_clade_counts(pfq_tree *tree, const uint64_t **here, const uint64_t **below, uint64_t *n);
/* One clade index (or PFQ_NO_CLADE) per unit of the last query call on `tree`, which must have set PFQ_WANT_LCA (else
 * PFQ_ERR_ARG); n_units = n_reads, with PFQ_PAIRED n_reads / 2.  Waits for that call.  A unit that hits every leaf (no k-mers,
 * threshold <= 0, all-leaf fragments) gets the LCA of all leaves: the root, or below a root with one child the deepest node
 * of that chain.  Library-owned; valid until the next query call on the tree. */
int pfq_last_lca(pfq_tree *tree, const uint32_t **lca, uint64_t *n_units);

/* ---- taxonomy (PFQ_WANT_TAXA) ----
 * The tree's topology is an index, not a classification: a taxonomy is a second tree over the same leaves, supplied by the user,
 * and every node of it gets two exact counts — the units assigned to it, and the units that touch it at all.
 * A taxonomy of a tree with L current leaves is given as n_taxa >= 1 taxa.
 *   - Taxon 0 is the root, with parent PFQ_NO_CLADE.
 *   - taxon_parent[i] < i for i > 0.
 *   - Every taxon has a name.
 *   - leaf_taxon[l] < n_taxa is the taxon that genome l sits directly under.
 *   - l is a leaf index in pfq_leaf_counts order.
 * The library derives the nodes:
 *   - Every genome is a node of its own, under its taxon.
 *   - A taxon with no genome anywhere below it is dropped.  The root is kept.
 *   - Nodes are numbered in pre-order: first a taxon, then the genomes directly under it in ascending leaf index, then its
 *     remaining child taxa in ascending input index, each with its subtree.
 *   - rank[l] is the position of genome l among the genomes in that order (0 .. L - 1).  So every node covers a contiguous
 *     range of ranks.
 * pfq_tree_taxa returns, per node, a pfq_taxon: parent, depth, first_rank, n_leaves, leaf (the leaf index of a genome node,
 * PFQ_NO_CLADE for a taxon), name (a genome node: the leaf's tax_id, as pfq_tree_clades names leaves).
 * A unit is a read, or with PFQ_PAIRED a fragment.  Its hit set H is exactly the row pfq_hits gives for it in that call; nothing
 * is decided again.  With PFQ_WANT_HITS an all-leaf unit's row lists all L leaves.  Per unit with H non-empty:
 *   - taxon(unit) is the deepest node that is an ancestor-or-self of every genome of H.  With H empty it is PFQ_NO_CLADE.
 *   - here[taxon(unit)] += 1.
 *   - any[t] += 1 for every node t that is an ancestor-or-self of at least one genome of H, once per unit however many genomes
 *     of H lie below t.
 *   - below[t] is the sum of here over t's subtree, derived on the host at read-out as pfq_clade_counts does.
 * Consequences: a call's increase of any[genome node of l] equals the increase of leaf counter l; any[root] = below[root] is the
 * number of units that hit anything; any[t] >= below[t] for every t.
 * All state is integer and is a pure function of the multiset of rows.  It does not depend on call split, replica split, path,
 * or any knob.
 *
 * pfq_tree_set_taxonomy copies everything it needs, builds the node table and uploads the device tables (their bytes count in
 * pfq_info.device_bytes); it replaces an earlier taxonomy and zeroes the taxon counters.  A violation of the rules above:
 * PFQ_ERR_ARG; an empty tree: PFQ_ERR_STATE; a subtree shard: PFQ_ERR_UNSUPPORTED (its rows are partial, as for PFQ_WANT_LCA and
 * PFQ_WANT_ABUNDANCE); a sticky insertion error is returned as by every other call.
 * pfq_tree_taxa: the node table, library-owned until the taxonomy is set again or dropped; *n = 0 when no taxonomy is set.
 * PFQ_WANT_TAXA: only together with PFQ_WANT_HITS (alone: PFQ_ERR_ARG — `any` needs whole rows, and the unordered hit pairs of a
 * counts-only call do not give them); without a taxonomy set: PFQ_ERR_STATE; on a subtree shard: PFQ_ERR_UNSUPPORTED.  It
 * combines with every other flag and changes none of their results (leaf counters, CSR, scores, LCAs, abundance log, coverage
 * sketch, pfq_last_stats), and works through pfq_query_batch, pfq_query_batch_device and pfq_text_query; pfq_query_frames keeps
 * flags == 0.  A block whose hit buffer overflowed and ran again is counted once.
 * pfq_taxon_counts waits for the device; here, below, any are library-owned [n] and any of the three pointers may be NULL.
 * pfq_last_taxa: one node index (or PFQ_NO_CLADE) per unit of the last query call on `tree`, which must have set PFQ_WANT_TAXA
 * (else PFQ_ERR_ARG, as pfq_last_lca); library-owned, valid until the next query call on the tree.
 * Lifetime: the counters are zeroed by pfq_leaf_counts_reset; pfq_tree_prune and pfq_tree_insert drop the taxonomy itself (the
 * leaves are no longer the ones it described): afterwards pfq_tree_taxa gives n = 0 and a flagged call PFQ_ERR_STATE until it is
 * set again.  Nothing of it is stored by pfq_tree_save. */
#define PFQ_WANT_TAXA 256u
typedef struct pfq_taxon {
    uint32_t parent;     /* node index; PFQ_NO_CLADE for the root */
    uint32_t depth;      /* edges from the root */
    uint32_t first_rank; /* the node's genomes are ranks [first_rank, first_rank + n_leaves) */
    uint32_t n_leaves;
    uint32_t leaf;       /* a genome node: its leaf index in pfq_leaf_counts order; a taxon: PFQ_NO_CLADE */
    const char *name;
} pfq_taxon;
int pfq_tree_set_taxonomy(pfq_tree *tree, uint64_t n_taxa, const uint32_t *taxon_parent, const char *const *taxon_names,
                          const uint32_t *leaf_taxon);
int pfq_tree_taxa(pfq_tree *tree, const pfq_taxon **nodes, uint64_t *n);
int pfq_taxon_counts(pfq_tree *tree, const uint64_t **here, const uint64_t **below, const uint64_t **any, uint64_t *n);
int pfq_last_taxa(pfq_tree *tree, const uint32_t **node, uint64_t *n_units);
/* The host side of the same, for tools that check a taxonomy before a device is used.  None of the three touches a device; what
 * they return is owned by the library per calling thread and valid until that thread calls the same function again.
 * pfq_db_leaf_ids: the tax_ids of <db_dir>'s leaves in pfq_leaf_counts order, from tree.bin alone (as pfq_db_shard_count reads
 *   it; PFQ_ERR_IO, PFQ_ERR_FORMAT likewise; an empty tree: n = 0).
 * pfq_taxonomy_read: a taxonomy file for the leaves named leaf_ids.  Lines end with '\n', a trailing '\r' is dropped; empty
 *   lines and lines beginning with '#' are skipped.  A line is genome<TAB>lineage[<TAB>ignored...]; fewer than two fields is an
 *   error.  lineage is a ';'-separated list of names from the top rank down, each trimmed of spaces; an empty lineage means
 *   directly under the root, an empty name inside a non-empty lineage is an error.  A taxon is identified by its whole path: the
 *   same name under two parents is two taxa.  Only lines whose genome equals a leaf id are considered (lines_considered; the
 *   others: lines_other) and every leaf with that id gets the lineage; two considered lines for one genome with different
 *   lineages is an error.  Taxon indices are assigned in order of first appearance over the considered lines, prefixes left to
 *   right; the root is taxon 0, named "root".  Leaves without a line sit under the root (leaves_without_line).  An unreadable
 *   file: PFQ_ERR_IO; an error in it: PFQ_ERR_FORMAT with a message that names the line.
 * pfq_taxonomy_nodes: the node table pfq_tree_set_taxonomy would derive for leaves named leaf_ids (PFQ_ERR_ARG as there). */
typedef struct pfq_taxonomy_file {
    uint64_t n_taxa;
    const uint32_t *taxon_parent;    /* [n_taxa] */
    const char *const *taxon_names;  /* [n_taxa] */
    uint64_t n_leaves;
    const uint32_t *leaf_taxon;      /* [n_leaves] */
    uint64_t lines_considered, lines_other, leaves_without_line;
} pfq_taxonomy_file;
int pfq_db_leaf_ids(const char *db_dir, const char *const **tax_ids, uint64_t *n_leaves);
int pfq_taxonomy_read(const char *path, const char *const *leaf_ids, uint64_t n_leaves, pfq_taxonomy_file *out);
int pfq_taxonomy_nodes(uint64_t n_leaves, const char *const *leaf_ids, uint64_t n_taxa, const uint32_t *taxon_parent,
                       const char *const *taxon_names, const uint32_t *leaf_taxon, const pfq_taxon **nodes, uint64_t *n);

/* ---- abundance (PFQ_WANT_ABUNDANCE) ----
 * The log holds, per unit of every PFQ_WANT_ABUNDANCE call since it was last cleared, the unit's row, by class (L = n_leaves):
 * empty: n_unhit; one leaf l: unique[l]; L > 1 and all L leaves (units without k-mers, threshold <= 0, all-leaf fragments — the
 * row says nothing about proportions): n_all_leaves; anything else: ambiguous, the row itself is kept in device memory.
 * pfq_abundance_estimate waits for the queued work and runs an integer EM from a uniform start, every time (the log is not
 * consumed; more queries may follow): a[l] = 1 << 16; one iteration: new[l] = unique[l] << 16, and every ambiguous row R with
 * D = sum of a over R > 0 adds (a[l] << 16) / D (unsigned, floor) to new[l] for each l in R (D = 0, possible only for rows of
 * 65 536 leaves or more, adds nothing); last_delta = max |new[l] - a[l]|; a = new.  It stops after an iteration with
 * last_delta <= tol (converged = 1), else after max_iters iterations (converged = 0).  The result is a pure function of the
 * multiset of logged rows: it does not depend on the order of the calls, how the units were split over them, or any knob.
 * The floor drops less than |R| * 2^-16 units per row and iteration, so the masses sum to slightly less than
 * (n_unique + n_ambiguous) << 16.  With no unit logged there is nothing to iterate: all masses are 0, iterations = 1,
 * converged = 1, last_delta = 0.  max_iters == 0: PFQ_ERR_ARG; an incomplete log (see PFQ_WANT_ABUNDANCE): PFQ_ERR_STATE.
 * mass and unique are library-owned and valid until the next estimate, reset or topology change on the tree.
 * The log and its counters are cleared by pfq_abundance_reset, pfq_leaf_counts_reset, pfq_tree_prune and pfq_tree_insert (the
 * leaf columns change meaning); they are not stored by pfq_tree_save.  The leaf counters are untouched by all of this. */
typedef struct pfq_abundance {
    uint64_t n_leaves;
    const uint64_t *mass;    /* [n_leaves] estimated units << 16, leaf order of pfq_leaf_counts; library-owned */
    const uint64_t *unique;  /* [n_leaves] units whose row is this leaf alone; library-owned */
    uint64_t n_units, n_unhit, n_unique, n_ambiguous, n_all_leaves;
    uint64_t n_entries;      /* leaf entries of the ambiguous rows held */
    uint64_t last_delta;
    uint32_t iterations, converged;
} pfq_abundance;
int pfq_abundance_estimate(pfq_tree *tree, uint32_t max_iters, uint64_t tol, pfq_abundance *out);
int pfq_abundance_reset(pfq_tree *tree);
/* Moves src's log (counters, unique, ambiguous rows) into dst's and clears src.  The trees must be replicas: the same
 * n_leaves, neither a subtree shard, dst != src (else PFQ_ERR_ARG); they may sit on different devices (the rows are staged
 * through host memory: this runs once per job).  An incomplete log on either side: PFQ_ERR_STATE.  If dst's log cannot take
 * the rows (as for a query call): PFQ_ERR_UNSUPPORTED, and both logs stay as they were. */
int pfq_abundance_absorb(pfq_tree *dst, pfq_tree *src);

/* ---- coverage (PFQ_WANT_COVERAGE) ----
 * Is a genome really in the sample, or do its reads pile onto one shared stretch?  Per leaf l the library keeps units[l],
 * matched[l] and a HyperLogLog sketch R[l] of 2^p one-byte registers (p: the option PFQ_COVER_P, 4..16, default 12) of the
 * distinct k-mers matched.  For every unit of a PFQ_WANT_COVERAGE call and every leaf l of its row: units[l] += 1, and every read x
 * of the unit (a fragment: both mates, whichever mate caused the listing) gives every canonical k-mer c of get_kmers(x),
 * duplicates included, whose num_hashes probed bits are all set in l's filter (the test PFQ_WANT_SCORES counts):
 *   matched[l] += 1;  h = seeded_hash(seed1, c), the first of the two hashes the probe indices are made of;
 *   u = mix(h), the splitmix64 finaliser: x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31;
 *   j = u >> (64 - p);  w = u << p (mod 2^64);  rho = min(clz64(w), 64 - p) + 1 (w = 0: 64 - p + 1);  R[l][j] = max(R[l][j], rho).
 * So a call's increase of matched[l] is the sum of its pfq_last_hit_scores over the rows that list l, and that of units[l] is the
 * leaf counter's.  The state is a pure function of the multiset of (k-mer, leaf) pairs logged: it does not depend on the order
 * of the calls, how the units were split over them, or any knob.
 * pfq_coverage_get waits for the queued work and copies the state out; the derived values are computed on the host in double:
 *   distinct[l]: classic HyperLogLog, m = 2^p, alpha = 0.7213 / (1 + 1.079 / m) (p = 4, 5, 6: 0.673, 0.697, 0.709),
 *     E = alpha m^2 / sum_j 2^-R[l][j], V = registers that are 0; m ln(m / V) if E <= 2.5 m and V > 0, else E; an all-zero sketch
 *     gives 0.  No large-range correction (the hash has 64 bits).  Standard error about 1.04 / sqrt(m): 1.6 % at p = 12.
 *   filter_bits[l]: set bits of l's filter (computed once per tree, lazily);
 *   genome_kmers[l] = -(nbits / num_hashes) log1p(-filter_bits / nbits), the distinct k-mers the genome put into the filter
 *     (Swamidass-Baldi); a full filter gives 0.0, "not estimable".
 * Breadth of coverage is distinct / genome_kmers (not clamped; 0 where genome_kmers is 0), duplication matched / distinct.
 * Before any PFQ_WANT_COVERAGE call everything is 0 except filter_bits and genome_kmers.  Leaves are in pfq_leaf_counts order;
 * the arrays are library-owned and valid until the next coverage call on the tree.
 * The sketch takes (n_leaves << p) + 16 n_leaves bytes of device memory (pfq_info.device_bytes counts them) from the first
 * flagged call until it is freed: by pfq_coverage_reset, pfq_leaf_counts_reset, pfq_tree_prune and pfq_tree_insert (the leaf
 * columns change meaning).  It is not stored by pfq_tree_save.  pfq_set_option("PFQ_COVER_P") outside 4..16 is PFQ_ERR_ARG, and
 * a change of p while the sketch holds units is PFQ_ERR_STATE.  The leaf counters are untouched by all of this. */
typedef struct pfq_coverage {
    uint64_t n_leaves, n_units; uint32_t precision;
    const uint8_t *registers;      /* [n_leaves << precision] */
    const uint64_t *units, *matched, *filter_bits;   /* [n_leaves] */
    const double *distinct, *genome_kmers;           /* [n_leaves] */
} pfq_coverage;                    /* library-owned, valid until the next coverage call on the tree */
int pfq_coverage_get(pfq_tree *tree, pfq_coverage *out);    /* before any flagged call: zeros, filter_bits filled */
int pfq_coverage_reset(pfq_tree *tree);
/* registers: element-wise max; units / matched / n_units: sums; src is emptied.  The trees must hold the same leaves with the
 * same hash parameters and precision (replicas, on any devices, or the same shard of one database), dst != src: else
 * PFQ_ERR_ARG.  Staged through host memory: this runs once per job. */
int pfq_coverage_absorb(pfq_tree *dst, pfq_tree *src);

/* ---- best rows (PFQ_ROWS_BEST) ----
 * Below threshold 1 a read from one strain also passes that strain's relatives, and its row lists the whole family although the
 * scores say which genome fits best.  With PFQ_ROWS_BEST the per-unit consumers take every unit's best-scoring genomes instead.
 * A unit is a read, or with PFQ_PAIRED a fragment.  Its row H(u) and the scores s are exactly what pfq_hits and
 * pfq_last_hit_scores give for the call.  The unit's best row is
 *     B(u) = { H(u)[j] : s[j] == max over the row }
 * in ascending leaf order; it is empty when H(u) is empty.  Ties stay.  Nothing is decided again: B is a pure function of (H, s).
 * With the flag set, PFQ_WANT_TAXA, PFQ_WANT_ABUNDANCE and PFQ_WANT_COVERAGE consume B(u) wherever their text above says "the row
 * pfq_hits gives for it".  Everything else of the call is bit for bit what it is without the flag: the leaf counters, the
 * pfq_hits CSR and pfq_last_hit_scores, pfq_last_stats and pfq_debug_last_capacity, PFQ_WANT_LCA with or without PFQ_LCA_BEST
 * (clade counters and pfq_last_lca), and the overflow retry: a block that ran again is reduced and consumed once.
 * Consequences:
 *   - Threshold 1: every listed leaf scores n_kmers, so B = H and the flag changes nothing.
 *   - Units without k-mers: all scores are 0, so B = H = all leaves.
 *   - Threshold <= 0 with k-mers: the row lists every leaf, and B is the top scorers only.
 *   - Abundance: the classes follow from |B(u)|: 0 unhit, 1 unique, L all-leaves, else ambiguous.
 *   - Coverage: units[l] counts the units whose best row lists l; a call's increase of matched[l] is the sum of its scores over the
 *     best rows that list l.
 *   - Taxonomy: any[genome node of l] grows by the units whose best row lists l, so it no longer equals the leaf counter's
 *     increase; any[root] = below[root] is still the number of units that hit anything.
 *   - All three states stay pure functions of the multiset of best rows: they do not depend on call split, replica split, query
 *     path or any knob.
 * Only together with PFQ_WANT_HITS | PFQ_WANT_SCORES, else PFQ_ERR_ARG.  Valid without any of the three consumers: then only
 * pfq_last_best_rows shows it.  On a subtree shard: PFQ_ERR_UNSUPPORTED — the best of a partial row is not the row's best; this
 * holds for PFQ_WANT_COVERAGE too, which otherwise accepts shards.  Works through pfq_query_batch, pfq_query_batch_device and
 * pfq_text_query; pfq_query_frames keeps flags == 0.
 * pfq_last_best_rows: the CSR of B for the last query call on `tree`, which must have set PFQ_ROWS_BEST (else PFQ_ERR_ARG, as
 * pfq_last_lca); out->n_reads is the number of units.  The rows live in device memory and are copied to the host by this call,
 * so a query call that is never asked pays nothing for the copy.  Library-owned; valid until the next query call on the tree.
 * It is also right after a call that returned PFQ_ERR_UNSUPPORTED from the abundance log with its other results standing. */
#define PFQ_ROWS_BEST 512u
int pfq_last_best_rows(pfq_tree *tree, pfq_hits *out);

/* ---- threshold sweep (PFQ_WANT_SWEEP) ----
 * The filter threshold decides everything a query reports, and finding it costs one whole run per candidate.  With a sweep list
 * set, one flagged call at a threshold no higher than the list's lowest also counts, per threshold of the list, what a call of
 * its own at that threshold would count.
 * A sweep list is T thresholds, 1 <= T <= PFQ_SWEEP_MAX, float, none NaN, strictly ascending.  Any finite values are allowed,
 * values <= 0 and > 1 included.  A unit is a read (fragments are refused); its n = max(len - k + 1, 0) k-mers.
 *     need_t = need_kmers(thr[t], n): the f32 product, ceilf, clamped, exactly what a call at thr[t] asks of the read.
 * thr[s] <= thr[t] implies need_s <= need_t, so the thresholds an entry passes are a prefix of the list.  For an entry e = (u, l)
 * of the call's final CSR with score s(e), exactly what pfq_hits and pfq_last_hit_scores give:
 *     p(e) = #{t : s(e) >= need_t(u)}, from 0 to T.
 * Per unit: top(u) = the maximum of p over its row (0 for an empty row); arg(u) = the leaf of the first entry that reaches it;
 * second(u) = the second-largest p counted with multiplicity (two entries at the maximum: second = top; a one-entry row: 0).
 * The unit's row at thr[t] is the entries with p > t.  That row is a single genome exactly for second <= t < top, and the genome
 * is arg.  State, all u64, accumulated over the flagged calls like the leaf counters, L = n_leaves:
 *     pass[(T + 1) x L]   pass[p][l] += 1 per entry
 *     uniq[T x L]         uniq[t][arg(u)] += 1 for every t in [second(u), top(u))
 *     tops[T + 1]         tops[top(u)] += 1 per unit
 *     n_units
 * Read-out (pfq_sweep_get), derived on the host in integers:
 *     leaf_units[t][l]  = sum over p > t of pass[p][l]        leaf_unique[t][l] = uniq[t][l]
 *     units_hit[t]      = sum over p > t of tops[p]           units_unique[t]   = sum over l of uniq[t][l]
 *     entries[t]        = sum over l of leaf_units[t][l]      genomes_hit[t]    = #{l : leaf_units[t][l] > 0}
 * Consequences:
 *   - On a tree where every parent filter is a superset of its children's (pfq_info.superset_verified == 1), a read passes leaf l
 *     at thr[t] exactly when l is in its row at any threshold <= thr[t] and that score reaches need_t.  So leaf_units[t] is the
 *     leaf counters' increase of the same reads queried at thr[t], units_hit[t] the number of non-empty rows of that query and
 *     units_unique[t] its one-entry rows.
 *   - A unit without k-mers has need 0 everywhere: its row lists all L leaves and every entry has p = T.
 *   - The state is a pure function of the multiset of (row, scores, n).  It does not depend on call split, replica split, query
 *     path or any knob.
 * pfq_tree_set_sweep copies the list, allocates and zeroes the device state ((2 T + 1) L + T + 1 words, counted in
 * pfq_info.device_bytes) and replaces an earlier list with its counters; n == 0 drops the list and frees the state.  A bad list
 * (n > PFQ_SWEEP_MAX, a NaN, not strictly ascending): PFQ_ERR_ARG.  An empty tree: PFQ_ERR_STATE.  PFQ_ERR_UNSUPPORTED, with a
 * message that says why: superset_verified == 0 (the scores of a read's ancestors are not in its row, so a leaf that fails at
 * thr[t] through an ancestor would be counted), and a subtree shard (units and unique rows would be partial).
 * PFQ_WANT_SWEEP: only together with PFQ_WANT_HITS | PFQ_WANT_SCORES, else PFQ_ERR_ARG; with PFQ_PAIRED: PFQ_ERR_ARG (a
 * fragment's score is the mates' sum, and its row is a union or intersection of per-mate decisions); without a list:
 * PFQ_ERR_STATE; the call's threshold must satisfy threshold <= thr[0] as floats (a NaN fails the comparison), else
 * PFQ_ERR_ARG.  It combines with every other flag and changes none of their results: leaf counters, CSR, scores, stats, LCA,
 * taxonomy, abundance, coverage, best rows.  It reads the whole rows, whatever PFQ_ROWS_BEST says.  It works through
 * pfq_query_batch, pfq_query_batch_device and pfq_text_query; pfq_query_frames keeps flags == 0.  A block whose hit buffer
 * overflowed and ran again is counted once.
 * The counters are zeroed by pfq_sweep_reset and pfq_leaf_counts_reset; pfq_tree_prune and pfq_tree_insert zero them and
 * re-size them to the new leaf count, and the list stays: a pruned or grown superset tree is still one.  Nothing of the sweep is
 * stored by pfq_tree_save.
 * pfq_sweep_get waits for the queued work; before any flagged call it returns zeros, without a list n_thresholds = 0.  The arrays
 * are library-owned until the next sweep call on the tree; leaf_units and leaf_unique are threshold-major.
 * pfq_sweep_absorb sums src's counters into dst's and zeroes src's (replicas of one database): the same conditions as
 * pfq_coverage_absorb, plus bit-identical lists; otherwise PFQ_ERR_ARG. */
#define PFQ_WANT_SWEEP 1024u
#define PFQ_SWEEP_MAX 16
int pfq_tree_set_sweep(pfq_tree *tree, const float *thresholds, uint32_t n);
typedef struct pfq_sweep {
    uint32_t n_thresholds;
    const float *thresholds;
    uint64_t n_leaves, n_units;
    const uint64_t *leaf_units, *leaf_unique;                         /* [n_thresholds * n_leaves], threshold-major */
    const uint64_t *units_hit, *units_unique, *entries, *genomes_hit; /* [n_thresholds] */
} pfq_sweep;
int pfq_sweep_get(pfq_tree *tree, pfq_sweep *out);
int pfq_sweep_reset(pfq_tree *tree);
int pfq_sweep_absorb(pfq_tree *dst, pfq_tree *src);

/* ---- frames and segments (pfq_query_frames) ----
 * Where on a long sequence (an assembled contig, a long read) does a genome match?  Every sequence is cut into overlapping
 * frames of `frame` = F bases every `step` = S bases, k <= F and 1 <= S <= F (else PFQ_ERR_ARG); each frame is classified exactly
 * as pfq_query_batch classifies a read holding those bytes; runs of consecutive frames that hit a leaf become segments, and each
 * segment is refined to k-mer resolution on that leaf's own filter.
 * Frames of a sequence of L bases: L <= F: one frame, [0, L).  Otherwise n = ceil((L - F) / S) + 1 frames, frame j = [s_j, s_j + F)
 *   with s_j = min(j * S, L - F): the last frame is flush with the end, no frame is a short tail.
 * Frame hits: H_j = the ascending leaf set pfq_query_batch(.., threshold, PFQ_WANT_HITS) gives a read made of frame j's bytes:
 *   its own n_kmers and need, guards and the coarse level as they are, any threshold (<= 0 and NaN included); a sequence shorter
 *   than k is one frame without k-mers and passes every leaf, as such a read does.
 * Segments: for a leaf l, a maximal run j0..j1 of consecutive frames with l in H_j:
 *   first_frame = j0, n_frames = j1 - j0 + 1, begin = s_j0, end = s_j1 + len(frame j1) (0-based, half-open);
 *   kmers = the k-mer positions p in [begin, end - k] (0 if end - begin < k);
 *   matched = those whose canonical k-mer has all num_hashes probed bits set in l's own filter (the test PFQ_WANT_SCORES counts);
 *   match_begin = the smallest such p, match_end = the largest such p plus k (matched == 0: both equal begin);
 *   longest_run = the longest run of consecutive matching positions.
 * Order: by sequence, then first_frame, then leaf; seg[offsets[i] .. offsets[i + 1]) are the segments of sequence i.
 * Leaf counters: += 1 per (sequence, distinct leaf among its segments) — they count sequences, as mapped_reads counts reads.
 *   With F >= the longest sequence of a call the counters and the per-sequence leaf sets equal those of
 *   pfq_query_batch(.., PFQ_WANT_HITS) on the same input.  Results do not depend on how the sequences are cut into calls, on the
 *   query path or on any knob.
 * Limits, PFQ_ERR_UNSUPPORTED with a message that says which, nothing counted: a sequence of 2^32 bases or more; 2^32 - 1 frames
 *   or more in one call (the classification takes a block of fewer than 2^31 - 1024: that is the limit in force); frame bytes
 *   (about the input times F / S) that do not fit in device memory.
 * Subtree shards are accepted: a leaf's segments depend only on that leaf's frame hits, so a shard's segments are the whole
 *   tree's for its leaves, with leaf indices local to the shard.
 * flags must be 0 (else PFQ_ERR_ARG): frames do not combine with pairs, LCA, abundance or coverage.  Both calls are synchronous.
 * Afterwards pfq_last_hit_scores and pfq_last_lca answer PFQ_ERR_ARG, as after a call without their flags; pfq_last_stats and
 * pfq_debug_last_capacity describe the inner classification, whose n_reads is the number of frames.  Sticky insert errors, the
 * empty tree (PFQ_ERR_STATE) and the stream-ordering rules are those of pfq_query_batch_device; total_bytes as there (unused).
 * The option PFQ_FRAME_PIECE (a positive multiple of 64, else PFQ_ERR_ARG) is how many k-mer positions one wave refines. */
typedef struct pfq_segment {
    uint32_t leaf, first_frame, n_frames, begin, end, match_begin, match_end, kmers, matched, longest_run;
} pfq_segment;
typedef struct pfq_segments {
    uint64_t n_seqs, n_frames;
    const uint64_t *offsets; /* [n_seqs + 1] */
    const pfq_segment *seg;  /* [offsets[n_seqs]] */
} pfq_segments;              /* library-owned until the next query call on the tree */
int pfq_query_frames(pfq_tree *tree, const uint8_t *seq, const uint64_t *offsets, uint64_t n_seqs, uint32_t frame, uint32_t step,
                     float threshold, uint32_t flags, pfq_segments *out);
int pfq_query_frames_device(pfq_tree *tree, const uint8_t *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t total_bytes,
                            uint32_t frame, uint32_t step, float threshold, uint32_t flags, void *stream, pfq_segments *out);

/* ---- text (pfq_text_parse, pfq_text_query) ----
 * Plain FASTA / FASTQ text parsed on the device into the block a query call takes, at the seam of the reference's readers
 * (file_parser.rs:191-301): the host only hands over file bytes.  Two calls, so that a caller who guessed a record boundary can
 * parse, check the guess and only then let the records reach the counters.
 * pfq_text_parse: the caller claims that text[0] is the first byte of a record's header line; the result is defined relative to
 * the sequential reader started there.  A line is a maximal run of bytes ended by '\n', without the '\n'; an unterminated last
 * run counts as a line only with PFQ_TEXT_FINAL; trimmed = without trailing bytes of {' ', \t, \n, \v, \f, \r}.
 * FASTQ: record r = lines 4r .. 4r + 3, beginning at b = the start of line 4r.  In this order: no byte is left: stop END; bytes are
 *   left but no considered line: MORE; b >= limit: LIMIT; fewer than four considered lines are left: SLOW with PFQ_TEXT_FINAL, else
 *   MORE; the record is not plain: SLOW; otherwise it is taken, its sequence is line 4r + 1 trimmed, and r + 1 follows.  Plain: line
 *   4r begins with '@', line 4r + 1 does not begin with '+' (it may be empty), line 4r + 2 begins with '+', line 4r + 3 trimmed is
 *   not empty.  A plain record is exactly what the sequential reader returns from b, and it goes on at line 4r + 4.
 * FASTA: a header is a line whose first byte is '>'.  Text that does not begin with '>': nothing taken, consumed 0, SLOW.  A
 *   record is complete when a later header is among the considered lines, or with PFQ_TEXT_FINAL.  In order: a record that begins
 *   at or beyond limit: LIMIT; an incomplete record: MORE; otherwise it is taken, its sequence being its other lines, each
 *   trimmed, joined.  All taken: consumed = len, END.
 * Empty text: nothing, END.  consumed is always the begin of the first record not taken, or len: the records taken are a prefix
 * of the sequential reader's, and it would read next at text + consumed.
 * The call changes no counter, log, sketch or query result and may be used on a tree whose filters are never queried.  text is a
 * host buffer (page-locked memory copies fastest) that may be reused when the call returns.  The copy and the parse kernels run
 * on the tree's copy stream into one of two alternating CSR buffer sets, so they overlap the classification of the previous
 * pfq_text_query; the call waits for its own work only, and for an earlier classification only if that one still reads the set
 * about to be reused.  The CSR (sequence buffer padded by 16 bytes) lives until the next pfq_text_parse on the tree or its close;
 * other query calls do not disturb it.  PFQ_ERR_ARG: tree or out NULL, text NULL with len > 0, an unknown format or flag;
 * PFQ_ERR_UNSUPPORTED: len >= 2^31 (ask in pieces).  The option PFQ_TEXT_TILE (a power of two, 256 .. 8192) is the text a block
 * scans.
 * pfq_text_query: exactly pfq_query_batch_device(tree, csr_seq, csr_off, n_records, n_bases, threshold, flags, NULL, hits) on the
 * block parsed last, ordered behind the parse by an event; every rule of that call applies.  It may be repeated (the counters
 * grow each time).  Before any parse: PFQ_ERR_STATE.  The parsed block is sequence data and does not depend on the leaves: a
 * block parsed before pfq_tree_insert or pfq_tree_prune may still be queried after it, and is then classified against the leaves
 * as they are at the query, like the same reads given to pfq_query_batch; pfq_text_format needs a pfq_text_query after the
 * change. */
#define PFQ_TEXT_FASTA 0
#define PFQ_TEXT_FASTQ 1
#define PFQ_TEXT_FINAL 1u         /* the text ends where the file ends */
#define PFQ_TEXT_WANT_RECORDS 2u  /* fill rec_begin */
enum { PFQ_TEXT_END = 0, PFQ_TEXT_LIMIT = 1, PFQ_TEXT_MORE = 2, PFQ_TEXT_SLOW = 3 };
typedef struct pfq_text {
    uint64_t n_records;        /* records taken */
    uint64_t consumed;         /* the records taken are text[0, consumed); the next record starts at text + consumed */
    uint64_t n_bases;          /* bases of the records taken (offsets[n_records] of the CSR) */
    uint32_t stop;             /* why it stopped, PFQ_TEXT_* */
    const uint64_t *rec_begin; /* [n_records + 1] byte offset of every taken record's header line, then consumed; NULL without PFQ_TEXT_WANT_RECORDS; library-owned */
} pfq_text;
int pfq_text_parse(pfq_tree *tree, const uint8_t *text, uint64_t len, uint64_t limit, int format, uint32_t flags, pfq_text *out);
int pfq_text_query(pfq_tree *tree, float threshold, uint32_t flags, pfq_hits *hits);
int pfq_debug_text_csr(pfq_tree *tree, uint8_t *seq_out, uint64_t *off_out);  /* tests: the parsed CSR copied to the host */

/* ---- blocked gzip (pfq_gz_scan, pfq_text_inflate, pfq_text_parse_inflated, pfq_text_read) ----
 * A general gzip stream is one deflate stream and has no independent pieces; blocked gzip (BGZF: what bgzip and the sequencers'
 * converters write and every htslib tool reads) is a sequence of independent gzip members of at most 64 KiB of text each, every
 * member's compressed size in its header and its text size and CRC-32 in its trailer.  So the host finds every member and every
 * output offset by walking headers, without inflating a byte, and the device inflates all members at once.
 * pfq_gz_scan (no device): the members of gz[0, len) from gz[0] on.  The member at p is taken when all of these hold: bytes 1f 8b
 *   08; FLG has FEXTRA and bits 5 - 7 clear; the extra field parses as subfields (SI1 SI2 SLEN data) that fill XLEN exactly, one of
 *   them 'B' 'C' with SLEN 2 (the first such counts; others may precede or follow): its value is BSIZE and the member is BSIZE + 1
 *   bytes; FNAME, FCOMMENT and FHCRC, if flagged, end inside the member; the deflate payload [header end, p + BSIZE + 1 - 8) has at
 *   least one byte; ISIZE <= PFQ_GZ_MEMBER_TEXT_MAX; p + BSIZE + 1 <= len.  Stops, in this order: no byte left: END; fewer bytes
 *   left than the fixed header with XLEN (12), the extra field or the member needs: MORE, with PFQ_TEXT_FINAL FOREIGN (a truncated
 *   file: the host reader will say so); not such a member: FOREIGN; taking it would pass max_text, or 2^31 - 1 bytes of text:
 *   LIMIT.  max_text 0: no limit of the caller's; 0 < max_text < PFQ_GZ_MEMBER_TEXT_MAX: PFQ_ERR_ARG, as are gz NULL with len > 0,
 *   out NULL and flags other than PFQ_TEXT_FINAL.  Boundaries are found only by walking headers, never by searching for magic
 *   bytes; a member of ISIZE 0 (the 28-byte end marker) is an ordinary member.  The tables are library-owned per calling thread
 *   and valid until that thread's next pfq_gz_scan.
 * pfq_text_inflate: scans as pfq_gz_scan does for the same arguments, copies gz[0, consumed) to the device on the tree's copy
 *   stream, inflates every member there (one wave a member; the grid is min(members, PFQ_INFLATE_BLOCKS), unset: two workgroups a
 *   compute unit) into a staging buffer of the tree (counted in pfq_info.device_bytes) and reads the statuses and CRCs back.  The
 *   input is untrusted: a member the device does not follow to the letter is a status, never an error: 0 ok, 1 malformed deflate
 *   (RFC 1951: a reserved block type, LEN != ~NLEN, HLIT > 286, HDIST > 30, a repeat with nothing before it or across the total, an
 *   over-subscribed or incomplete code set - but for no distance code at all or exactly one of length 1 -, no end-of-block code,
 *   symbols 286 / 287, distances 30 / 31, a distance beyond the member's own text, input that ends early), 2 length mismatch (text
 *   beyond or short of ISIZE, payload bytes left over), 3 the text's CRC-32 differs from the trailer's.  When in doubt the device
 *   rejects; the caller then lets zlib decide.  n_good: the leading members with status 0; good_text: their text bytes.  The call
 *   changes no counter, no query result and not the parsed block; it waits for its own work.  The tables and statuses are owned
 *   by the tree and valid until its next pfq_text_inflate.  gz may be reused when the call returns.  PFQ_ERR_ARG as pfq_gz_scan,
 *   and for a NULL tree.
 * pfq_text_parse_inflated: exactly pfq_text_parse(tree, carry ++ staged[0, good_text), carry_len + good_text, limit, format, flags,
 *   out), staged being the text the last pfq_text_inflate on the tree left: the same fields, stops, rec_begin, alternating CSR sets
 *   and follow-up calls (pfq_text_query, pfq_text_format, pfq_debug_text_csr, pfq_text_read see that text, offsets relative to the
 *   carry's first byte).  The text is assembled on the device: the carry's upload, then a device-to-device copy of the staged text
 *   behind it (the parse kernels want the text 16-byte aligned).  It may be repeated after one inflate.  Before an inflate on the
 *   tree: PFQ_ERR_STATE; carry_len + good_text >= 2^31: PFQ_ERR_UNSUPPORTED; carry NULL with carry_len > 0: PFQ_ERR_ARG.
 * pfq_text_read: bytes [from, from + n) of the text parsed last by either parse call, copied to dst (what a caller keeps as the
 *   next carry).  Before a parse: PFQ_ERR_STATE; from + n beyond that text, dst NULL with n > 0: PFQ_ERR_ARG.
 * pfq_debug_last_inflate: device milliseconds of the last pfq_text_inflate that had members, by HIP events: ms[0] the copies to
 *   the device, ms[1] the kernel.  PFQ_ERR_STATE without one. */
#define PFQ_GZ_MEMBER_TEXT_MAX 65536
enum { PFQ_GZ_END = 0, PFQ_GZ_LIMIT = 1, PFQ_GZ_MORE = 2, PFQ_GZ_FOREIGN = 3 };
enum { PFQ_GZ_OK = 0, PFQ_GZ_MALFORMED = 1, PFQ_GZ_LENGTH = 2, PFQ_GZ_CRC = 3 };  /* a member's status */
typedef struct pfq_gz_members {
    uint64_t n_members, consumed, text_bytes; /* whole members taken: gz[0, consumed), the sum of their ISIZE */
    uint32_t stop;                            /* PFQ_GZ_* */
    const uint64_t *begin;                    /* [n_members + 1] byte offset of every member, then consumed */
    const uint64_t *text_begin;               /* [n_members + 1] prefix sums of ISIZE */
} pfq_gz_members;
typedef struct pfq_text_inflated {
    pfq_gz_members members; /* what pfq_gz_scan gives for the same arguments (tree-owned here) */
    uint64_t n_good;        /* leading members with status 0 */
    uint64_t good_text;     /* members.text_begin[n_good]: the text pfq_text_parse_inflated will see */
    const uint8_t *status;  /* [members.n_members], tree-owned */
} pfq_text_inflated;
int pfq_gz_scan(const uint8_t *gz, uint64_t len, uint64_t max_text, uint32_t flags, pfq_gz_members *out);
int pfq_text_inflate(pfq_tree *tree, const uint8_t *gz, uint64_t len, uint64_t max_text, uint32_t flags, pfq_text_inflated *out);
int pfq_text_parse_inflated(pfq_tree *tree, const uint8_t *carry, uint64_t carry_len, uint64_t limit, int format, uint32_t flags, pfq_text *out);
int pfq_text_read(pfq_tree *tree, uint64_t from, uint64_t n, uint8_t *dst);
int pfq_debug_last_inflate(pfq_tree *tree, double *ms);

/* ---- text output (pfq_text_format) ----
 * The POS / NEG records of a device-parsed block formatted on the device, at the seam of the reference's writer
 * (main.rs:345-361,394-404): the bytes `query --pos-filter / --neg-filter` writes, made from the text, the gathered sequences
 * and the hit rows where pfq_text_parse and pfq_text_query left them.
 * Inputs: the block of n records is the one the last pfq_text_parse on the tree took; row H(r) is what the last pfq_text_query of
 * that block gave for record r (the final CSR, after any overflow retry).  Record r has the global index first_index + r and
 * lies in result block (first_index + r) / block.
 * The reference decides POS / NEG per result block, through a map id -> genomes (result_map.rs:20-45): two records of a block
 * with the same id merge their genomes, and a record without a hit is still mapped if its id is in the map.  In a block whose
 * ids are pairwise different neither can happen, so the device formats exactly those blocks and leaves the rest to the caller:
 * Ids and blocks: id(r) = the bytes of the record's header line, trimmed as the parser trims, from index 1 up to the first
 *   separator or the trimmed end — the separator is ' ' in FASTQ and any of {' ', \t, \n, \v, \f, \r} in FASTA; the id may be
 *   empty.  A result block is whole when all `block` records of it are among the n records.  The records before the first block
 *   boundary inside the call are left as one run PFQ_LEFT_HEAD, those behind the last boundary as one run PFQ_LEFT_TAIL; a call
 *   that contains no whole block leaves everything as one run PFQ_LEFT_HEAD (n = 0: no run).  A whole block is plain when the
 *   ids of its records are pairwise different as byte strings (compared exactly: equal hashes are settled by the bytes); a
 *   whole block that is not plain is left as one run PFQ_LEFT_REPEATED_ID.
 * Bytes of one record: a record of a whole plain block is mapped when H(r) is not empty.  With PFQ_FMT_POS a mapped record goes
 *   to the pos stream, with PFQ_FMT_NEG an unmapped one to neg, in ascending r.  Its bytes: '@' (FASTA: '>'), id(r); for a
 *   mapped record " |" and the tax_ids (those of pfq_leaf_counts) of H(r) in row order joined by ','; '\n'; the record's
 *   sequence of the parsed CSR with only 'a' .. 'z' lowered by 32 (bytes >= 0x80 and everything else stay); '\n'; FASTQ only:
 *   "+\n", line 4r + 3 trimmed, '\n'.
 * Left runs: left[i] covers records first .. first + count - 1 (r, relative to the parsed block); pos_at / neg_at are the offsets
 *   in the two streams where the run's bytes belong.  The streams with the caller's own bytes for the left runs spliced in at
 *   these offsets are the whole block's output in record order.
 * PFQ_ERR_STATE: no parse yet; the last query call on the tree was not a successful pfq_text_query of this block with
 * PFQ_WANT_HITS and without PFQ_PAIRED (another query call or another parse in between counts as this case).  PFQ_ERR_ARG: tree or
 * out NULL, block 0 or above PFQ_FMT_BLOCK_MAX, neither PFQ_FMT_POS nor PFQ_FMT_NEG, unknown flag bits.  PFQ_ERR_UNSUPPORTED: a
 * subtree shard (its rows are partial); a record whose output would be 2^32 bytes or more.  A sticky insertion error is returned
 * as everywhere else.
 * The call changes no counter, log, sketch or query result, may be repeated and then gives the same result, runs on the tree's
 * copy stream and waits only for its own work.  pos, neg and left are valid until the next pfq_text_format or pfq_text_parse on
 * the tree; pfq_info.device_bytes counts its buffers.  Options (results never depend on them): PFQ_FMT_GRID caps every grid, so
 * that tiny inputs take several grid-stride trips; PFQ_FMT_HASH_BITS (1 .. 64) keeps only that many bits of the id hash, so that
 * different ids collide and the byte comparison runs (a block's keys hold at most 51 of them); PFQ_FMT_TIME=1 makes the HIP
 * events behind pfq_debug_last_format (PFQ_ERR_STATE without a timed call of at least one record). */
#define PFQ_FMT_POS 1u
#define PFQ_FMT_NEG 2u
#define PFQ_FMT_BLOCK_MAX 8192
enum { PFQ_LEFT_HEAD = 1, PFQ_LEFT_TAIL = 2, PFQ_LEFT_REPEATED_ID = 3 };
typedef struct pfq_text_left { uint64_t first, count, pos_at, neg_at; uint32_t why, pad_; } pfq_text_left;
typedef struct pfq_text_records {
    uint64_t n_records;                                       /* records of the parsed block */
    uint64_t pos_records, neg_records, pos_bytes, neg_bytes;  /* what the two streams hold */
    const uint8_t *pos, *neg;                                 /* library-owned page-locked host memory */
    uint64_t n_left;
    const pfq_text_left *left;                                /* ascending, disjoint; library-owned */
} pfq_text_records;
int pfq_text_format(pfq_tree *tree, uint64_t first_index, uint32_t block, uint32_t flags, pfq_text_records *out);
int pfq_debug_last_format(pfq_tree *tree, double *ms /* [3]: ids + blocks, sizes + scans, emit; HIP events */);

/* ---- blocked gzip written on the device (pfq_bgzf_deflate, pfq_text_format_gz) ----
 * Text deflated where it lies, into members of blocked gzip that every gzip reader, every htslib tool and pfq_text_inflate take.
 * Cutting (a pure function of len and the cuts): a stream of len bytes with n_cuts ascending offsets 0 <= cuts[0] <= .. <=
 *   cuts[n_cuts - 1] <= len has the n_cuts + 1 pieces [0, cuts[0]), [cuts[0], cuts[1]), .., [cuts[n_cuts - 1], len).  Every piece is
 *   cut from its first byte into members of PFQ_BGZF_MEMBER_TEXT text bytes, the last one shorter; an empty piece has no member.
 *   The 28-byte end marker is never written: it belongs to the end of a file, which only the caller knows.
 * Bytes of a member: a pure function of the member's text, stated rule by rule at the head of phagefilter_amd/csrc/
 *   pfq_deflate_core.h (tiles of 256 positions, a hash of 4 bytes into 2^13 entries plus the distance-1 candidate, a greedy
 *   parse, one dynamic block from the member's own counts limited to 15 bits, or one stored block where that is not smaller), so
 *   the device's bytes are those of the stand-alone host program tools/deflate_host.cpp, whatever the grid.  A member is at most
 *   its text + 31 bytes.  There are no levels.
 * pfq_bgzf_deflate: text[0, len) goes to the device on the tree's copy stream, is cut, deflated (one workgroup a member; the grid
 *   is min(members, PFQ_DEFLATE_BLOCKS), unset: one workgroup a compute unit, what their LDS admits) and gathered, and the members
 *   come back, piece after piece, in gz.  piece_begin [n_pieces + 1] and member_begin [n_members + 1] are offsets into gz.
 *   PFQ_ERR_ARG: tree or out NULL, text NULL with len > 0, cuts NULL with n_cuts > 0, cuts not ascending or beyond len;
 *   PFQ_ERR_UNSUPPORTED: len >= 2^31.
 * pfq_text_format_gz: exactly pfq_text_format for the same arguments — the same preconditions, errors, counts and left runs —
 *   except that the two plain streams stay on the device: out->pos and out->neg are NULL, and each stream that flags asks for is
 *   deflated where it lies, cut at left[0].pos_at, .., left[n_left - 1].pos_at (neg_at for the other): piece j of pos_gz is what the
 *   caller writes between its own bytes for left run j - 1 and for left run j, n_left + 1 pieces in all, empty ones without a member.
 *   A later pfq_text_format gives what it would have given.
 * Both change no counter, result or parsed block, wait for their own work, and leave results (library-owned, gz page-locked) that
 * are valid until the tree's next call of either; pfq_info.device_bytes counts the buffers.
 * pfq_debug_last_deflate: device milliseconds of the tree's last deflate that had members (of pfq_text_format_gz: its last
 *   stream), by HIP events: ms[0] the copy to the device (pfq_text_format_gz: none), ms[1] the deflate kernel, ms[2] scan, gather
 *   and the copy back.  PFQ_ERR_STATE without one. */
#define PFQ_BGZF_MEMBER_TEXT 65280
typedef struct pfq_bgzf {
    const uint8_t *gz;            /* the members back to back */
    uint64_t gz_bytes, n_members, n_pieces;
    const uint64_t *piece_begin;  /* [n_pieces + 1] */
    const uint64_t *member_begin; /* [n_members + 1] */
} pfq_bgzf;
int pfq_bgzf_deflate(pfq_tree *tree, const uint8_t *text, uint64_t len, const uint64_t *cuts, uint64_t n_cuts, pfq_bgzf *out);
int pfq_text_format_gz(pfq_tree *tree, uint64_t first_index, uint32_t block, uint32_t flags, pfq_text_records *out, pfq_bgzf *pos_gz, pfq_bgzf *neg_gz);
int pfq_debug_last_deflate(pfq_tree *tree, double *ms /* [3] */);

/* ---- read preprocessing (pfq_prep_reads, pfq_prep_query) ----
 * What a trimmer in front of a classifier does — low-quality and poly-X tails cut, reads that are too short, mostly N or of
 * low complexity dropped — on the device, into the block a query call takes.  Integers only; the result for a read is a pure
 * function of that read (for a fragment: of its two mates).
 * Per read: bases s[0, L); optionally qualities q[0, L), Phred+33: p[j] = max(q[j] - 33, 0).  up(c) = c & 0xDF; a base is an N
 * when up(c) is none of A C G T.  The steps, in this order, give a kept interval [b, e), starting from [0, L):
 *   1. Quality (only if trim_quality = Q > 0 and the read has qualities).  Leading: b = min{ j : p[j] >= Q }; none: the interval
 *      is empty.  Sliding window: w = min(trim_window, L - b); for i = b .. L - w, window i is bad iff p[i] + .. + p[i + w - 1] <
 *      Q w; e = the first bad i, or L if no window is bad.  Trailing: e = 1 + max{ j in [b, e) : p[j] >= Q }; none: empty.
 *   2. Poly-X tail (only if poly_x = P > 0 and the interval is not empty): r = the length of the longest suffix of [b, e) whose
 *      bytes all equal up(s[e - 1]) under up; if r >= P then e -= r.  Applied once.
 *   3. len = e - b; an empty interval is reported as begin = 0, len = 0.
 *   4. The reason, the first that applies: PFQ_PREP_SHORT: len < min_length; PFQ_PREP_N: more than max_n N bases in [b, e)
 *      (0xffffffff: off); PFQ_PREP_COMPLEXITY: min_complexity = C > 0 and 100 d < C max(len - 1, 0), d = the number of j in
 *      [b, e - 1) with up(s[j]) != up(s[j + 1]); else 0: the read is kept (an empty read too).
 *   5. With PFQ_PREP_PAIRED reads 2i and 2i + 1 are mates (an odd n_reads: PFQ_ERR_ARG); a fragment is kept only if both mates
 *      are, and a mate that passed on its own while its partner was dropped gets PFQ_PREP_MATE.
 * Parameters: trim_quality 0 (off) or 1 .. 93; trim_window 1 .. 1024; min_complexity 0 (off) or 1 .. 100; unknown flag bits, a
 * NULL tree, params or out, NULL seq or offsets with n_reads > 0: PFQ_ERR_ARG.  qual shares offsets with seq, NULL: no read has
 * qualities; has_qual is a byte per read, NULL: every read has (if qual is given).  PFQ_ERR_UNSUPPORTED: a read of 2^32 bases or
 * more, 2^31 - 1024 reads or more.
 * pfq_prep: the totals of the call — n_reason[0] = n_kept, n_trimmed = the kept reads with len < L, bases_kept over the kept reads
 * — and, with PFQ_PREP_WANT_READS, library-owned host arrays begin, len, reason [n_reads] and kept [n_kept] (the kept reads'
 * indices, ascending), valid until the next pfq_prep_reads on the tree; without the flag they are NULL and only the totals are
 * copied back.
 * The call changes no counter, log, sketch or query result.  seq, qual, offsets and has_qual are host buffers that may be reused
 * when the call returns.  The copies and the kernels run on the tree's copy stream into one of two alternating CSR buffer sets,
 * so they overlap the classification of the previous pfq_prep_query; the call waits for its own work only, and for an earlier
 * classification only if that one still reads the set about to be reused.  The CSR (the kept intervals, the sequence buffer padded
 * by 16 bytes; qualities are not gathered) lives until the next pfq_prep_reads on the tree or its close; other query calls do not
 * disturb it.
 * pfq_prep_query: exactly pfq_query_batch_device(tree, csr_seq, csr_off, n_kept, bases_kept, threshold, flags, NULL, hits) on the
 * block prepared last, ordered behind the prep by an event; every flag and rule of that call applies.  The units are the kept
 * reads, with PFQ_PAIRED the kept fragments (mates are dropped together, so they stay adjacent); PFQ_PAIRED on a block prepared
 * without PFQ_PREP_PAIRED: PFQ_ERR_ARG.  It may be repeated (the counters grow each time).  Before any prep: PFQ_ERR_STATE.  Like
 * a parsed block, a block prepared before pfq_tree_insert or pfq_tree_prune may still be queried after it, against the leaves as
 * they are at the query. */
#define PFQ_PREP_PAIRED 1u      /* reads 2i and 2i + 1 are mates */
#define PFQ_PREP_WANT_READS 2u  /* fill begin, len, reason, kept */
enum { PFQ_PREP_KEPT = 0, PFQ_PREP_SHORT = 1, PFQ_PREP_N = 2, PFQ_PREP_COMPLEXITY = 3, PFQ_PREP_MATE = 4 };
typedef struct pfq_prep_params {
    uint32_t trim_quality;   /* Q: 0 off, else 1 .. 93 */
    uint32_t trim_window;    /* W: 1 .. 1024 */
    uint32_t poly_x;         /* P: 0 off */
    uint32_t min_length;
    uint32_t max_n;          /* 0xffffffff: off */
    uint32_t min_complexity; /* C, percent: 0 off, else 1 .. 100 */
    uint32_t flags;          /* PFQ_PREP_* */
} pfq_prep_params;
typedef struct pfq_prep {
    uint64_t n_reads, n_kept, bases_in, bases_kept, n_trimmed;
    uint64_t n_reason[5];    /* reads per reason, PFQ_PREP_KEPT .. PFQ_PREP_MATE */
    const uint32_t *begin, *len, *reason; /* [n_reads]; NULL without PFQ_PREP_WANT_READS; library-owned */
    const uint32_t *kept;    /* [n_kept] likewise */
} pfq_prep;
int pfq_prep_reads(pfq_tree *tree, const uint8_t *seq, const uint8_t *qual, const uint64_t *offsets, const uint8_t *has_qual,
                   uint64_t n_reads, const pfq_prep_params *params, pfq_prep *out);
int pfq_prep_query(pfq_tree *tree, float threshold, uint32_t flags, pfq_hits *hits);
int pfq_debug_prep_csr(pfq_tree *tree, uint8_t *seq_out, uint64_t *off_out);  /* tests: the prepared CSR copied to the host */
/* measurements: device milliseconds of the last pfq_prep_reads with reads — ms[0] trim and mark, ms[1] the two scans, ms[2] offsets and gather */
int pfq_debug_last_prep(pfq_tree *tree, double *ms);

/* ---- adapters (pfq_tree_set_adapters, pfq_prep_last_adapters) ----
 * A library whose inserts are shorter than the read length reads through into the 3' adapter; what follows the insert matches no
 * genome.  While adapters are set on a tree, every pfq_prep_reads on it first cuts each read at the leftmost place an adapter
 * matches.  Integers only; no indels.
 * For a read s[0, L) and an adapter A[0, m), with min_overlap = O and max_error_percent = E:
 *   at position p < L the overlap is o = min(m, L - p);
 *   mm = the number of i < o with up(s[p + i]) != A[i], up(c) = c & 0xDF (a read base outside ACGT therefore always mismatches);
 *   p matches iff o >= O and 100 mm <= E o;
 *   cut = the smallest p that matches any adapter of the read's set, or L if none does;
 *   which = the lowest index in the set of an adapter that matches at cut, or 0xff if none does.
 * Steps 1 - 5 of "read preprocessing" then run exactly as written on the read cut to s[0, cut), q[0, cut): step 1's L in
 * w = min(trim_window, L - b) is cut, and a read cut to nothing is an empty read.  begin and len stay relative to the original
 * read; bases_in and the L of n_trimmed (kept reads with len < L) stay the original length, so an adapter-cut read that is kept
 * counts as trimmed.  Hence, with adapters set, begin, len, reason, kept and the prepared CSR of a block equal those of the same
 * call without adapters on the reads cut at cut.
 * pfq_tree_set_adapters: set1 serves unpaired reads and first mates; set2 serves second mates (the odd reads of a call with
 * PFQ_PREP_PAIRED), with n2 == 0 they use set1.  Letters ACGTacgt only (stored in upper case), every length m with O <= m <=
 * PFQ_ADAPTER_LEN_MAX, at most PFQ_ADAPTER_MAX a set, O 1 .. 64, E 0 .. 50, n1 > 0 if n2 > 0; else PFQ_ERR_ARG, the message
 * names the adapter.  n1 == 0 and n2 == 0 drops the state.  The state does not depend on the leaves: pfq_tree_prune and
 * pfq_tree_insert keep it; pfq_tree_save stores nothing of it.  A sticky insertion error is returned as everywhere else.
 * pfq_prep_last_adapters: what the adapter step of the last pfq_prep_reads found, before the mate rule; PFQ_ERR_STATE if there
 * has been no prep yet or the last one ran without adapters.  pfq_prep_params, pfq_prep and the three values of
 * pfq_debug_last_prep keep their meaning: ms[0] does not include the adapter kernels, which pfq_debug_last_adapters reports. */
#define PFQ_ADAPTER_MAX 8        /* per set */
#define PFQ_ADAPTER_LEN_MAX 64
int pfq_tree_set_adapters(pfq_tree *tree, const char *const *set1, uint32_t n1, const char *const *set2, uint32_t n2,
                          uint32_t min_overlap /* O: 1 .. 64 */, uint32_t max_error_percent /* E: 0 .. 50 */);
typedef struct pfq_prep_adapters {
    uint64_t n_reads, n_found, bases_cut;         /* of the last pfq_prep_reads: reads with cut < L, sum of L - cut; before the mate rule */
    uint64_t found[2 * PFQ_ADAPTER_MAX];          /* reads per `which`: set1 at [0, 8), set2 at [8, 16) */
    const uint32_t *cut; const uint8_t *which;    /* [n_reads], only after a call with PFQ_PREP_WANT_READS, else NULL; library-owned */
} pfq_prep_adapters;
int pfq_prep_last_adapters(pfq_tree *tree, pfq_prep_adapters *out);
/* measurements: device milliseconds of the adapter kernels of the last pfq_prep_reads with reads (HIP events) */
int pfq_debug_last_adapters(pfq_tree *tree, double *ms);

/* ---- mate overlap (pfq_tree_set_mate_overlap, pfq_prep_last_overlap) ----
 * When the insert of a paired-end fragment is shorter than its reads, the two mates are reverse complements of each other over
 * the whole insert, and everything behind the insert is adapter, whatever its sequence.  While the overlap is set on a tree,
 * every pfq_prep_reads with PFQ_PREP_PAIRED on it finds each fragment's insert length from its mates and cuts both mates there.
 * Integers only; no indels.
 * A fragment is reads 2i (mate 1, a[0, L1)) and 2i + 1 (mate 2, b[0, L2)).  up(c) = c & 0xDF; comp maps A <-> T and C <-> G on
 * upper-cased letters; a base outside ACGT on either side always mismatches.  min_overlap = O, max_error_percent = E.
 * The hypothesis "the insert has I bases" compares the pairs (i, j = I - 1 - i) with 0 <= i < L1 and 0 <= j < L2, that is i in
 * [max(0, I - L2), min(I, L1)):
 *   o(I) = the number of such pairs;
 *   mm(I) = the pairs with up(a[i]) != comp(up(b[j])), or with either base outside ACGT;
 *   I matches iff o(I) >= O and 100 mm(I) <= E o(I);
 *   insert = the LARGEST matching I in [O, L1 + L2 - O], or PFQ_NO_INSERT if none matches; mismatches = mm(insert) (0 if none).
 * The largest I cuts least: poly-A mates or a tandem repeat, which match at many I, get the longest insert and lose nothing.
 * With an insert found, ocut(mate 1) = min(L1, insert) and ocut(mate 2) = min(L2, insert); otherwise ocut = L1 and L2.  An insert
 * at or above max(L1, L2) is reported and cuts nothing.
 * A fragment with a mate longer than PFQ_OVERLAP_LEN_MAX is not analysed: it counts as n_skipped and gets no insert and no cut.
 * With adapters set too, both steps look at the original reads, independently, and steps 1 - 5 of "read preprocessing" run on
 * s[0, min(cut, ocut)), cut being the adapter step's; pfq_prep_last_adapters reports exactly what it reports without the overlap.
 * begin, len, bases_in and n_trimmed keep the conventions of "adapters": relative to the original read, and a read that is cut and
 * kept counts as trimmed.  Hence, with the overlap set, begin, len, reason, kept and the prepared CSR of a block equal those of
 * the same call without it on the reads cut at min(cut, ocut).
 * pfq_tree_set_mate_overlap: O 1 .. PFQ_OVERLAP_LEN_MAX (0 drops the state, E is then ignored), E 0 .. 50; else PFQ_ERR_ARG, the
 * message names the parameter.  The state does not depend on the leaves: pfq_tree_prune and pfq_tree_insert keep it;
 * pfq_tree_save stores nothing of it.  A sticky insertion error is returned as everywhere else.
 * A pfq_prep_reads without PFQ_PREP_PAIRED does not run the step.
 * pfq_prep_last_overlap: what the step of the last pfq_prep_reads found, before the mate rule; PFQ_ERR_STATE if there has been no
 * prep yet or the last one ran without the step.  n_fragments = n_analysed + n_skipped; n_readthrough: insert < max(L1, L2);
 * reads_cut and bases_cut: the reads with ocut < L and the sum of L - ocut, by ocut alone; hist[I] = the fragments of this call
 * with insert I.  ms[0] of pfq_debug_last_prep does not include the overlap kernel, which pfq_debug_last_overlap reports. */
#define PFQ_OVERLAP_LEN_MAX 512
#define PFQ_OVERLAP_INSERT_MAX 1024
#define PFQ_NO_INSERT 0xffffffffu
int pfq_tree_set_mate_overlap(pfq_tree *tree, uint32_t min_overlap /* O: 0 off, else 1 .. 512 */, uint32_t max_error_percent /* E: 0 .. 50 */);
typedef struct pfq_prep_overlap {
    uint64_t n_fragments, n_analysed, n_skipped, n_overlapped /* insert found */, n_readthrough /* insert < max(L1, L2) */;
    uint64_t reads_cut, bases_cut;            /* by ocut alone, before the mate rule */
    const uint64_t *hist;                     /* [PFQ_OVERLAP_INSERT_MAX + 1] fragments per insert, of this call; library-owned */
    const uint32_t *insert, *mismatches;      /* [n_fragments], only after a call with PFQ_PREP_WANT_READS, else NULL; library-owned */
} pfq_prep_overlap;
int pfq_prep_last_overlap(pfq_tree *tree, pfq_prep_overlap *out);
/* measurements: device milliseconds of the overlap kernel of the last pfq_prep_reads with reads (HIP events) */
int pfq_debug_last_overlap(pfq_tree *tree, double *ms);

/* ---- mate correction (pfq_tree_set_mate_correct, pfq_prep_last_corrections) ----
 * Where the mates of a fragment overlap, every base was read twice.  Where the two calls disagree and one has a high quality and the
 * other a low one, the low one is a sequencing error and the mate says what the base was.  While the correction is set on a tree,
 * the mate overlap step of every pfq_prep_reads on it rewrites such bases and their qualities on the device, before steps 1 - 5 of
 * "read preprocessing" and before the gather.  Integers only; a fragment's correction is a pure function of that fragment.
 * With a[0, L1), b[0, L2), up, comp, O, E, insert, mm as in "mate overlap", qualities q1, q2 (Phred+33), high = H and low = W < H:
 * Which fragments.  A fragment is corrected only if it was analysed and an insert I was found (below max(L1, L2) or not),
 * mm(I) > 0, and both mates have qualities (qual given, and has_qual NULL or set for both).  A fragment with an insert and
 * mm(I) > 0 that lacks qualities counts in n_no_quality.
 * Which pairs.  For every pair (i, j = I - 1 - i) of the hypothesis I that mm(I) counts, with p1 = max(q1[i] - 33, 0) and
 * p2 = max(q2[j] - 33, 0):
 *   if up(a[i]) is one of ACGT, p1 >= H and p2 <= W:  b[j] = comp(up(a[i])), an upper-case letter, and q2[j] = q1[i], the raw byte;
 *   else if up(b[j]) is one of ACGT, p2 >= H and p1 <= W:  a[i] = comp(up(b[j])) and q1[i] = q2[j];
 *   else the pair is unresolved and nothing changes.
 * A low side outside ACGT (an N with quality '#') is therefore repaired; a high side outside ACGT never corrects anything.  Each
 * base lies in exactly one pair of I, so the order of the pairs does not matter.
 * What the other steps see.  The adapter step and the overlap step look at the original reads: insert, mismatches, ocut, every
 * total, the histogram and pfq_prep_last_adapters are unchanged by the correction.  Steps 1 - 5 and the gather see the corrected
 * bases and qualities, cut at min(cut, ocut) as before.  Hence begin, len, reason, kept, the totals and the prepared CSR equal those
 * of the same call without the correction on the corrected mates.  A corrected position behind the cut is harmless and is still
 * reported.
 * pfq_tree_set_mate_correct: high 0 (off, low is then ignored) or 1 .. 93, low < high; else PFQ_ERR_ARG, the message names the
 * parameter.  The step needs the mate overlap: with the correction set but no overlap set, or in a pfq_prep_reads without
 * PFQ_PREP_PAIRED, it does not run.  The state does not depend on the leaves: pfq_tree_prune and pfq_tree_insert keep it;
 * pfq_tree_save stores nothing of it.  A sticky insertion error is returned as everywhere else.
 * pfq_prep_last_corrections: the totals of the last pfq_prep_reads — the fragments with a corrected base, the corrected bases per
 * mate, n_unresolved: the mismatching pairs, in fragments whose mates both have qualities, that were left as they were,
 * n_no_quality — and, only after a call with PFQ_PREP_WANT_READS (else NULL and n_patches 0), the library-owned patch list,
 * ascending by (read, pos): read is an index into the block given to pfq_prep_reads, pos is relative to the original read, base and
 * qual are what the position holds now, old_base and old_qual what it held.  A caller that holds the original records applies the
 * list to get the corrected ones.  The list has exactly n_bases[0] + n_bases[1] entries, whatever their number, and is valid until
 * the next pfq_prep_reads on the tree.  PFQ_ERR_STATE if there has been no prep yet or the last one ran without the step.
 * A call without PFQ_PREP_WANT_READS corrects in the overlap kernel, in place, with no list and no further wait of the host; a
 * call with it waits once more, for the length of the list.  pfq_debug_last_overlap reports the overlap kernel, the correction
 * or its counting included; pfq_debug_last_corrections the scan and the patch kernel of a call with PFQ_PREP_WANT_READS. */
#define PFQ_MATE_CORRECT_HIGH 30   /* the defaults of the CLI and the Python binding */
#define PFQ_MATE_CORRECT_LOW 14
int pfq_tree_set_mate_correct(pfq_tree *tree, uint32_t high /* H: 0 off, else 1 .. 93 */, uint32_t low /* W < H */);
typedef struct pfq_prep_patch {
    uint32_t read, pos;
    uint8_t base, qual, old_base, old_qual;
} pfq_prep_patch;
typedef struct pfq_prep_corrections {
    uint64_t n_fragments_corrected;
    uint64_t n_bases[2];                      /* corrected bases of first and of second mates */
    uint64_t n_unresolved, n_no_quality;
    uint64_t n_patches;                       /* n_bases[0] + n_bases[1] after a call with PFQ_PREP_WANT_READS, else 0 */
    const pfq_prep_patch *patches;            /* [n_patches], only after a call with PFQ_PREP_WANT_READS, else NULL; library-owned */
} pfq_prep_corrections;
int pfq_prep_last_corrections(pfq_tree *tree, pfq_prep_corrections *out);
/* measurements: device milliseconds of the scan and the patch kernel of the last pfq_prep_reads with reads (HIP events) */
int pfq_debug_last_corrections(pfq_tree *tree, double *ms);

/* ---- depletion (pfq_prep_deplete) ----
 * Host and contaminant screening between the trimmer and the classifier: the units of the block prepared last on `tree` that hit a
 * second tree, the screen, on the same device leave the block before pfq_prep_query sees it.
 * What the call does.  The units (the kept reads; with PFQ_PAIRED the kept fragments) are classified against `screen` exactly as
 * pfq_query_batch_device(screen, csr_seq, csr_off, n_kept, bases_kept, threshold, flags, ..) would classify the prepared CSR, with
 * the screen's own k, hashes, seeds and topology.  flags: 0, PFQ_PAIRED or PFQ_PAIRED | PFQ_PAIR_BOTH, anything else PFQ_ERR_ARG.
 * It is a query call on `screen` in the sense of pfq_last_hit_scores: the screen's leaf counters grow by exactly what that call
 * would add, and what the screen's previous query call left becomes invalid.  A unit is removed iff its row on the screen is not
 * empty.  The classifier's rule for a read shorter than the screen's k holds: it has no k-mer, passes every leaf, and is removed;
 * with PFQ_PAIR_BOTH a fragment with such a mate gets the other mate's set, so it is removed iff the other mate hits.  That is
 * what query --neg-filter against the screen followed by a run on NEG_FILTERING does.
 * What is left.  The prepared block of `tree` is the remaining units in their order, mates together, the CSR padded by 16 bytes as
 * before; pfq_prep_query, pfq_debug_prep_csr and a further pfq_prep_deplete see that block, so screens compose (host, then PhiX),
 * and a second call with the same screen removes nothing.
 * What is not touched.  No counter, log, sketch or query result of `tree`; the arrays pfq_prep_reads handed out (begin, len,
 * reason, kept), which stay as that call left them; pfq_prep_last_adapters and pfq_prep_last_overlap.
 * pfq_prep_depleted: the totals of the call and of the block afterwards and, only if the block was prepared with
 * PFQ_PREP_WANT_READS (else NULL), library-owned host arrays valid until the next pfq_prep_deplete or pfq_prep_reads on the tree:
 * kept [n_kept], the remaining reads' indices into the block given to pfq_prep_reads, ascending, and reason [n_reads], the prep's
 * reasons with PFQ_PREP_DEPLETED written over the removed reads (pfq_prep.n_reason keeps its five entries and their meaning).
 * Errors.  PFQ_ERR_ARG: a NULL tree, screen or out, screen == tree, trees on different devices, PFQ_PAIRED on a block prepared
 * without PFQ_PREP_PAIRED; PFQ_ERR_STATE: before any pfq_prep_reads on `tree`, an empty screen; PFQ_ERR_UNSUPPORTED: the screen
 * is a subtree shard (its rows are partial); a sticky insertion error of either tree is returned as everywhere else.  A refused
 * call changes nothing on either tree.  A block with n_kept == 0 is a no-op that returns zeros.
 * Overlap.  The call returns totals, so it waits for its own work: the screen's classification, the mark, the scans and the
 * compaction, all on the stream of the prep.  It neither waits for nor disturbs the classification of the previous block that
 * pfq_prep_query has queued on `tree` (which reads the other CSR set); a pfq_prep_query of this very block is waited for. */
#define PFQ_PREP_DEPLETED 5   /* reason of a read whose unit hit the screen */
typedef struct pfq_prep_depleted {
    uint64_t n_units, units_removed, reads_removed, bases_removed;   /* of this call */
    uint64_t n_kept, bases_kept;                                     /* the prepared block afterwards */
    const uint32_t *kept;    /* [n_kept] indices into the block given to pfq_prep_reads, ascending */
    const uint32_t *reason;  /* [n_reads] the prep's reasons with PFQ_PREP_DEPLETED written over the removed reads */
} pfq_prep_depleted;
int pfq_prep_deplete(pfq_tree *tree, pfq_tree *screen, float threshold, uint32_t flags, pfq_prep_depleted *out);
/* measurements: device milliseconds of the last pfq_prep_deplete with units — ms[0] the screen's classification (host waits
 * between its stages included), ms[1] mark, the two scans, offsets and gather (HIP events) */
int pfq_debug_last_deplete(pfq_tree *tree, double *ms);

/* ---- genome similarity ----
 * Which genomes of a database are related, and how closely?  Every leaf's Bloom filter is in device memory, all built with one
 * geometry and one seed pair; for two filters the set bits and the shared set bits estimate how many k-mers each genome has and
 * how many they share.  The device computes, exactly, for the listed leaves of `a` and of `b`:
 *   shared_bits[i * n_b + j] = popcount(filter of leaves_a[i] AND filter of leaves_b[j]),  bits_a[i], bits_b[j] = their set bits
 * (bit indices below nbits only), and the host derives in double, with m = nbits, h = num_hashes,
 *   n(x) = -(m / h) * log1p(-x / m) for x < m, and n(m) = 0.0: "not estimable", as genome_kmers of the coverage,
 * and for a pair A = bits_a[i], B = bits_b[j], I = shared_bits, U = A + B - I (the set bits of the union of the two filters):
 *   kmers_a = n(A), kmers_b = n(B);
 *   shared_kmers = max(0, n(A) + n(B) - n(U)), and 0 if any of the three is not estimable;
 *   jaccard = shared_kmers / n(U), and 0 where n(U) is 0.
 * Two unrelated filters share about A * B / m bits by chance; the inclusion-exclusion cancels that in expectation.  A leaf against
 * itself gives shared_bits = bits and jaccard = 1.0 exactly.  What a caller derives from these:
 *   containment_a = shared_kmers / kmers_a, the share of a's k-mers that b has (0 where kmers_a is 0); containment_b likewise;
 *   ani = 1 + ln(2 J / (1 + J)) / kmer_size for J = jaccard > 0, else 0: the Mash distance, turned round.
 * leaves_a / leaves_b are leaf indices in pfq_leaf_counts order — the current leaves, after pfq_tree_prune or pfq_tree_insert; on a
 * subtree shard they are local to the shard.  A NULL list means all leaves (its n is ignored); a list may be unordered and may
 * repeat; an explicit empty list (n_a == 0 or n_b == 0) is PFQ_OK with an empty result.  b may be a, or NULL meaning a.
 * PFQ_ERR_ARG: a or out NULL; the trees differ in kmer_size, nbits, num_hashes, seed1 or seed2 (the message names the field) or
 * sit on different devices; a leaf index >= n_leaves.  PFQ_ERR_UNSUPPORTED: n_a * n_b > 2^26 (ask in panels).  PFQ_ERR_STATE: an
 * empty tree.  A sticky insertion error of either tree is returned as by every other call.
 * The call is synchronous: it waits for both trees' queued work, insertions included, and for its own.  It changes no counter,
 * log, sketch or query scratch, so pfq_last_stats, pfq_last_hit_scores and pfq_last_lca still describe the last query.  Its
 * device buffers (8 (n_a + n_b) + 4 n_a n_b bytes and the row lists) live only during the call.  The options PFQ_SIM_SLICES and
 * PFQ_SIM_NAIVE of `a` choose how the device computes the same numbers (DESIGN.md "Similarity"). */
typedef struct pfq_similarity {
    uint64_t n_a, n_b;
    const uint32_t *shared_bits;            /* [n_a * n_b], row-major */
    const uint64_t *bits_a, *bits_b;        /* [n_a], [n_b] set bits of each listed leaf's filter */
    const double *kmers_a, *kmers_b;        /* [n_a], [n_b] */
    const double *shared_kmers, *jaccard;   /* [n_a * n_b] */
} pfq_similarity;                           /* library-owned by `a`, valid until the next similarity call on `a` or its close */
int pfq_tree_similarity(pfq_tree *a, const uint32_t *leaves_a, uint64_t n_a,
                        pfq_tree *b, const uint32_t *leaves_b, uint64_t n_b, pfq_similarity *out);

/* ---- re-clustering ----
 * pfq_tree_build_balanced and pfq_tree_insert decide a tree's shape by the order the genomes arrive in.  pfq_tree_recluster
 * makes a new tree over the same leaves whose shape follows from the leaf filters alone: average-linkage agglomerative
 * clustering of the chance-corrected similarities, on the device, in integers.  The result is a pure function of the filters.
 * Nodes: the L current leaves of `src`, in pfq_leaf_counts order, are nodes 0 .. L - 1; internal nodes are L, L + 1, .. in the
 *   order they are made.
 * Leaf pair: with m = nbits, A and B the set bits of the two filters, I their shared set bits (all three as pfq_tree_similarity
 *   reports them: bit indices below nbits only) and U = A + B - I,
 *     num = max(0, I m - A B),  den = U m - A B,  q = floor(num 2^20 / den), and q = 0 where den = 0:  0 <= q <= 2^20.
 *   A B / m is what two unrelated filters share by chance.
 * Clusters: S(X, Y) = the sum of q over the leaf pairs (x in X, y in Y), w(X, Y) = |X| |Y|; the score of the pair is S / w, and
 *   after X and Y are merged into Z, S(Z, W) = S(X, W) + S(Y, W).
 * Order: (X, Y1) is before (X, Y2) when S1 w2 > S2 w1, compared as 128-bit products; on equality the smaller node index.
 * Rounds: every live node i finds best(i), the first of all other live nodes in that order; every pair with best(i) = j,
 *   best(j) = i, i < j is merged; the pairs are taken in ascending i and get consecutive new indices, left child i, right
 *   child j.  (Of the pairs with the highest score the one with the smallest (i, j) is always such a pair.)  Rounds repeat
 *   until one node is left, the root.  L = 1: that leaf is the root.
 * The new tree: 2 L - 1 nodes on src's device, with src's parameters and seeds.  A leaf keeps its tax_id, its .bf name and its
 * filter words, padding bits included; an internal node's filter is the OR of its children's and its name "Internal_Node_<n>"
 * with a running n that skips names in use, as pfq_tree_insert names with a NULL name; superset_verified is 1; every counter,
 * log and sketch starts at zero.
 * The call is synchronous: it waits for src's queued work, insertions included (a sticky insertion error is returned as by
 * every other call), and changes nothing of src: counters, logs, sketches, query scratch and pfq_last_stats stay.  Its scratch
 * (8 L^2 bytes of scores and a panel of shared bits) is freed before it returns.  src's options PFQ_SIM_SLICES and
 * PFQ_SIM_NAIVE choose how the shared bits are computed, as for pfq_tree_similarity.
 * PFQ_ERR_ARG: src or out NULL.  PFQ_ERR_STATE: an empty tree.  PFQ_ERR_UNSUPPORTED: a subtree shard; two leaves that share one
 * .bf name (the new tree would save two files under it); more than 16384 leaves, or a score matrix that does not fit in device
 * memory beside the two trees (the message says which). */
int pfq_tree_recluster(pfq_tree *src, pfq_tree **out);
/* The merge log of a tree made by pfq_tree_recluster, one entry per internal node in creation order: node = L + its position,
 * left and right its children (indices as above), round the round that made it (from 0), n_leaves the leaves below it,
 * score_sum = S(left, right) and pairs = w(left, right): the similarity the merge happened at is score_sum / (pairs 2^20).
 * *rounds: the rounds run.  Library-owned by the tree until it is closed or its topology changes (pfq_tree_insert,
 * pfq_tree_prune).  Any other tree: *n = 0, *rounds = 0. */
typedef struct pfq_merge {
    uint32_t node, left, right, round, n_leaves, pad_;
    uint64_t score_sum, pairs;
} pfq_merge;
int pfq_tree_merges(pfq_tree *tree, const pfq_merge **merges, uint64_t *n, uint32_t *rounds);

/* get_leaf_counts (query.rs:197-218): leaves left-to-right, zeros included.  Library-owned arrays. */
int pfq_leaf_counts(pfq_tree *tree, const char *const **tax_ids, const uint64_t **counts, uint64_t *n_leaves);
/* save_leaf_counts (query.rs:173-183): "<tax_id>,<count>\n" for count > 0, no header. */
int pfq_save_leaf_counts(pfq_tree *tree, const char *csv_path);

/* Multi-GPU reduction hooks (one process per GPU; the host framework all-reduces with RCCL):
 * copy the u64[n_leaves] device counters out to / in from a device buffer on `stream`. */
int pfq_leaf_counts_export(pfq_tree *tree, uint64_t *d_dst, void *stream);
int pfq_leaf_counts_import(pfq_tree *tree, const uint64_t *d_src, void *stream);
int pfq_leaf_counts_reset(pfq_tree *tree);
/* The same hooks for what THIS replica counted: export_delta writes counters - base, where the base is what the counters held
 * when the tree was opened (BloomNode::mapped_reads stored in tree.bin — non-zero in a database that was saved after a query),
 * last reset, imported or reduced; import_delta(sum of the ranks' deltas) sets counters = base + sum and makes that the new
 * base.  Reducing deltas keeps stored counts from being added once per rank: every rank ends with stored + new, like one
 * device and like the reference (query.rs:143 accumulates on the loaded value).  pfq_leaf_counts_import also sets the base. */
int pfq_leaf_counts_export_delta(pfq_tree *tree, uint64_t *d_dst, void *stream);
int pfq_leaf_counts_import_delta(pfq_tree *tree, const uint64_t *d_src, void *stream);

/* Number of HIP devices this process can use (`--devices all` of the CLI). */
int pfq_device_count(int *n);

/* Several GPUs behind one process (the block loop of main.rs:334-368 dealt over devices): `trees` are replicas of one
 * database (pfq_tree_open of the same directory, same pruning) on any devices, each fed its own share of the reads by its
 * own host thread.  This sums their per-leaf counters so that afterwards EVERY replica holds the job's totals
 * (mapped_reads of query.rs:143 as if one tree had seen all reads): what each replica counted since it was opened (or last
 * reduced) is added — replicas that share a device on that device, then ONE ncclAllReduce(sum, uint64, n_leaves) over RCCL /
 * xGMI across the distinct devices (8 KiB at 1024 leaves) — onto the counts the database was opened with, which therefore
 * count once; calling it again without new queries changes nothing.  The communicator of a device set is created on first
 * use and kept until the last tree of the process is closed.  Waits for the replicas' queued work.  librccl is loaded when this first meets replicas on more than one device
 * (PFQ_RCCL_ALWAYS=1: a one-rank communicator even then, for exercising the path on a one-GPU box). */
int pfq_trees_allreduce_counts(pfq_tree *const *trees, uint32_t n_trees);
/* Number of RCCL ranks the last pfq_trees_allreduce_counts on this thread used (0: no communicator was needed). */
uint32_t pfq_last_allreduce_ranks(void);

/* ---- measurement / test hooks ---- */

/* Tuning / test knobs, e.g. ("PFQ_TILE", "0").  The PFQ_* environment variables of the same names are
 * read once, when a tree is created or opened; this changes one knob of one tree afterwards.  value NULL or "": back
 * to the built-in choice.  Results never depend on a knob. */
int pfq_set_option(pfq_tree *tree, const char *name, const char *value);

/* Scratch capacities of the last pfq_query_batch[_device] and how far its kernels got into them (waits for the stream
 * of that call).  Writes min(n, PFQ_CAPACITY_N) values: [0] deferred-pair cursor, [1] its cap, [2] guard-pair cursor,
 * [3] its cap, [4] k-mer miss-word cursor, [5] its cap, [6] tile-mode miss bytes handed out (saturates at the cap),
 * [7] its cap, [8] hit cursor of the first attempt, [9] its hit cap, [10] attempts (2: the hit buffer overflowed and the
 * block ran again), [11] pairs sorted into the buckets.  A cursor above its cap: that buffer overflowed, the rest was
 * certified inline.  Pair values are 0 on the direct path; hit values are 0 without PFQ_WANT_HITS / PFQ_PAIRED /
 * PFQ_WANT_LCA. */
#define PFQ_CAPACITY_N 12
int pfq_debug_last_capacity(pfq_tree *tree, uint64_t *out, uint64_t n);

/* Position slots: every leaf or guard column whose filter has at most 8192 set bits in each 2^20-bit tile
 * keeps the tile-relative positions of those bits, 8192 u32 per tile, and the LDS-tile certificates at theta = 1 rebuild such
 * a tile from its slot instead of loading its 128 KiB.  Made with the device layout (builds it if need be); option
 * PFQ_TILE_LISTS=0: none.  out[0] columns with slots, [1] bytes the slots hold, [2] tiles the last query call built from
 * slots, [3] tiles it loaded dense (both 0 unless its certificates ran as k_tile_test<0>; waits for that call). */
int pfq_tile_lists_info(pfq_tree *tree, uint64_t out[4]);
/* The dense screen of k_classify at theta = 1: 4 k-mers of 16 reads a pass, or — the lean build — 2 k-mers of 32
 * reads where four rows a read keep false candidates rare: E = sum over the leaves of (set bits / nbits)^4 <= 2^-10, rows of
 * at most 32 words, one leaf group, not block mode (option PFQ_SCREEN_KMERS: 0 / unset this rule, 2 wherever the rows allow,
 * 4 never).  Results do not depend on the build; n_candidates may.  out[0] k-mers a read the screen of the last query call
 * took (2: the lean build ran, 4, 0: the call had no such screen — direct path, thresholds below 1), [1] E of the tree as it
 * is (builds the device layout and counts the leaves' bits if need be, once per topology), [2] words of a row, [3] column
 * groups.  (A call of its own and not a bit of pfq_stats.pair_stage: callers compare the bits of pair_stage above 3 with the
 * tail shapes.) */
int pfq_screen_info(pfq_tree *tree, double out[4]);
/* The pair slots of k_classify at theta = 1: a wave appends its deferred pairs to ranges of the pair buffer
 * that it reserves in whole chunks of 32 slots with one atomic on the buffer's cursor.  A batched emission that has to reserve
 * asks, beyond what its pass needs, for min(A x 32, pairs of the pass x groups of reads the wave still has to screen) slots,
 * rounded up to 32, so that the next passes find their slots reserved; what a wave leaves unused is voided (at most
 * (A + 1) x 32 slots a wave).  Option PFQ_PAIR_AHEAD: A = 0 .. 16, unset 8; 0: every pass reserves what it needs and no more.
 * Option PFQ_CLASSIFY_BLOCKS (tests): a cap on the grid of the classify launches — without it every wave of a small input has
 * one group of reads and never reserves ahead.  Results do not depend on either.  out[1] A of the last query call's classify
 * launches (0: it deferred no leaf pairs a pass at a time — direct path, thresholds below 1, block mode, PFQ_BATCH_EMIT=0),
 * [2] reservations those launches made (waits for the call); [0] and [3] are 0: they are kept for the bucket histogram made
 * from the pair buffer by a kernel of its own, which was measured and not built. */
int pfq_pair_info(pfq_tree *tree, uint64_t out[4]);
/* Copy min(n, 8192) entries of the slot of (column, tile) to the host: positions < 2^20 in any order, unused entries
 * 0xffffffff.  A column without slots: PFQ_ERR_STATE. */
int pfq_debug_tile_list(pfq_tree *tree, uint64_t col, uint64_t tile, uint32_t *out, uint64_t n);
/* tests: one probe bucket of the last query call's LDS-tile passes at theta = 1 (not block mode), copied to the host after the
 * call (waits for it).  The buckets are reused pass after pass: a chunk's bucket holds its entries only if no later pass took
 * its place.  out, of cap >= PFQ_TILE_BUCKET_WORDS u32: [0] fill mark in 32-bit words (may exceed the capacity: what did not
 * fit took the fallback), [1] the words of the bucket the format uses (packed: 4/5 of its capacity, room for as many entries), [2] first sorted pair of the chunk, [3] its pairs, [4] its column, [5] its
 * pass, [6] 1: packed entries, [7] chunks of the call (written even when `chunk` is out of range), [8] rounds the chunk was
 * binned in, [16 .. 272) the first pair of every round (both only with packed entries), [272 .. 1296) the read of each of the
 * chunk's pairs, then min(fill, capacity, cap - PFQ_TILE_BUCKET_WORDS) words of the bucket.
 * Packed entries: a 16-byte vector is five 24-bit entries [pair of the round : 4][offset in tile : 20], entry j in bits
 * 24 j .. 24 j + 23, and the round's number in bits 120 .. 127; a run (one round's entries) is padded to a whole vector with
 * copies of its last entry. */
#define PFQ_TILE_BUCKET_WORDS 1296
int pfq_debug_tile_bucket(pfq_tree *tree, uint64_t chunk, uint64_t tile, uint32_t *out, uint64_t cap);


/* Per-call statistics of the last pfq_query_batch[_device] (valid after the stream is synchronised). */
typedef struct pfq_stats {
    uint64_t n_reads, n_candidates, n_hits, n_allhit_reads;
    uint64_t algorithmic_bytes; /* sum_r L(r) + |hits(r)| * need(r) * num_hashes * 32 */
    uint32_t path;              /* 0 = direct kernel, 1 = bucketed (screen, pairs sorted by leaf, certificates out of LDS tiles / L2 slices) */
    uint32_t n_slices;
    uint32_t tile_mode;         /* 1: certificates tested out of LDS tiles (k_tile_*), k_verify_rec only as fallback
                                 * (thresholds < 1: entries name k-mers, the passes leave per-chunk miss bytes);
                                 * 2: block mode — pairs are (read, block of 8 leaves, candidate mask), one entry tests a probe for
                                 * all candidates of the block (chosen when reads pass several related leaves; any threshold in (0, 1]) */
    uint32_t n_fallback_pairs;  /* pairs the LDS-tile pass could not bin (certified by the fallback kernel) */
    uint64_t n_chunks, tile_entries;
    uint32_t tile_passes_launched, tile_passes_needed;  /* LDS-tile stage: passes over the reused probe buckets */
    /* two-level frontier (trees of more than 2048 leaves): the reads are screened against a coarse level of internal
     * nodes first and every group of leaf columns only sees the reads with a live ancestor there (query.rs:119-141) */
    uint32_t leaf_groups;       /* groups of leaf columns of the sliced matrix (1 for trees of up to 2048 columns) */
    uint32_t coarse_cols;       /* columns (internal nodes) of the coarse level this call used; 0: flat frontier */
    uint32_t coarse_probes;     /* probes per k-mer its screens looked at */
    uint32_t tile_bin_build;    /* build of k_tile_bin the LDS-tile passes of this call ran: waves << 16 | bin capacity
                                 * (e.g. 16 << 16 | 512, 8 << 16 | 128); 0: no pass ran */
    uint64_t group_reads;       /* (read, leaf group) combinations the coarse level let through to the leaf level */
    uint32_t pair_stage;        /* bucketed path, between classify and the certificates.  Bits 0-1: how the pairs were sorted by leaf —
                                 * 1: slices of slots counted in an LDS histogram, one global atomic per bucket and slice;
                                 * 2: one global atomic per pair (more buckets than LDS holds).  Bit 2 (0x4): k_classify only deferred
                                 * its survivors and k_tail_records made all their probe records, 64 k-mers a pass
                                 * (theta = 1 with records unless PFQ_SPLIT_RECORDS=0).  Bits 4-6: the shapes of
                                 * last-window pass that served at least one pair — 0x10: sixteen reads x 4 k-mers,
                                 * 0x20: four x 16, 0x40: two x 32 (none: no last window was left to the batched kernel).
                                 * Bit 3 (0x8): k_classify emitted at least one pair a pass at a time (theta = 1, leaf pairs — not in block mode — unless PFQ_BATCH_EMIT=0).
                                 * Bit 7 (0x80): at least one pass ran the slots-only build of k_tile_test<0> (theta = 1, not in block
                                 * mode, every column of the tree has position slots, unless PFQ_TILE_STREAM=0) */
    uint32_t entry_pack;        /* 1: the LDS-tile passes wrote and read packed entries, five 24-bit entries and a round number per
                                 * 16 bytes (theta = 1, not in block mode; option PFQ_ENTRY_PACK: 0 never, 1 / unset where the call's
                                 * mean read length makes the format's 16 pairs a round free, 2 always).  (A field of its own, in the
                                 * padding behind pair_stage: the bits of pair_stage above 3 are the tail shapes and bit 7.) */
} pfq_stats;
int pfq_last_stats(pfq_tree *tree, pfq_stats *out);
/* Force a query path: -1 auto, 0 direct, 1 bucketed. */
int pfq_set_path(pfq_tree *tree, int path);

/* Per-kernel device time of the query path, measured with HIP events recorded on the stream the kernels are
 * launched on.  begin: record around the kernels of the next (up to max_calls) query calls; end: synchronise and sum. */
typedef struct pfq_profile {
    uint64_t calls;
    double classify_ms; /* k_classify (pre-screen, frontier, inline certificates) + k_expand_guards + k_tail_records (the probe
                         * records of the deferred reads at theta = 1; only their last windows with PFQ_SPLIT_RECORDS=0) */
    double bucket_ms;   /* bucket scan + scatter */
    double bin_ms;      /* k_tile_plan + k_tile_bin (probes binned by leaf chunk and filter tile) */
    double test_ms;     /* k_tile_test (tiles tested out of LDS) */
    double verify_ms;   /* k_verify_rec / k_verify (L2-sliced certificates; only the fallback pairs in tile mode) */
    double finalize_ms; /* k_finalize */
} pfq_profile;
int pfq_profile_begin(pfq_tree *tree, uint32_t max_calls);
int pfq_profile_end(pfq_tree *tree, pfq_profile *out);

/* K1 parity hook: the num_hashes bit indices of every canonical k-mer of `seq` (HOST buffers), exactly what
 * BloomFilter::contains probes (bloom_filter.rs:312-332 via hash_iter.rs:13-45): out_idx[(kmer * num_hashes) + i]. */
int pfq_debug_kmer_indices(pfq_tree *tree, const uint8_t *seq, uint64_t len, uint64_t *out_idx, uint64_t *n_kmers);
/* The last pfq_tree_similarity call on `a` that had pairs to compute: the slices it cut the filter words into (PFQ_SIM_NAIVE: 1)
 * and, if the option PFQ_SIM_TIME was 1 during it, the device time of its intersection kernel alone in milliseconds, between two
 * HIP events round the launch (no copy, no clearing, no host arithmetic); without the option no call makes events and the time
 * is 0.  Either pointer may be NULL.  Before any such call: 0 and 0. */
int pfq_debug_last_similarity(pfq_tree *a, double *kernel_ms, uint32_t *slices);
/* The last pfq_tree_recluster call on `src` that ran rounds: ms[0] the shared bits and scores of all leaf pairs, ms[1] all rounds
 * (kernels, read-backs and the unions of the new filters), ms[2] the nearest-neighbour kernel alone over all rounds, in device
 * milliseconds between HIP events — measured only if src's option PFQ_CLUSTER_TIME was 1 during the call, else 0;
 * *nn_bytes: the score-matrix bytes the nearest-neighbour kernel read over all rounds; *rounds.  Any pointer may be NULL. */
int pfq_debug_last_recluster(pfq_tree *src, double *ms, uint64_t *nn_bytes, uint32_t *rounds);
/* Copy one node's filter words (Lsb0 u64, bloom_filter.rs:86) to the host; node = pre-order index. */
int pfq_debug_node_filter(pfq_tree *tree, uint64_t node, uint64_t *out_words, uint64_t n_words);

/* Synthetic workload generators of SURVEY §8d on the device (counter-based splitmix64); bench/test data only. */
int pfq_synth_genomes_device(uint8_t *d_out, uint64_t n_genomes, uint64_t genome_len, uint64_t seed_base,
                             void *stream);
int pfq_synth_reads_device(uint8_t *d_out, uint64_t first_read, uint64_t n_reads, uint64_t read_len,
                           const uint8_t *d_genomes, uint64_t genome_len, uint64_t n_genomes, uint64_t seed,
                           void *stream);

/* Page-locked host memory for the buffers handed to pfq_query_batch: the host-to-device copy then runs at PCIe rate
 * instead of going through the runtime's pageable staging path.  (The reference keeps reads in ordinary Vec<u8>s,
 * file_parser.rs:150-172; this is the transfer-side counterpart of that buffer.)  A tree must be open on the device. */
int pfq_host_alloc(uint64_t bytes, void **out);
int pfq_host_free(void *p);

const char *pfq_last_error(void);
const char *pfq_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PFQ_H */
