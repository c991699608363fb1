// pfq_kernels.h — argument blocks and launch wrappers shared by the kernels (pfq_kernels.hip) and the host
// side of libpfq (pfq_host.cpp).  Device layout, see DESIGN.md §3:
//
//   bits   u64[n_filters][n_words]   node-major filters in the reference's own bit order (BitVec<usize,Lsb0>,
//                                    bloom_filter.rs:86): bit idx = word idx>>6, mask 1<<(idx&63).
//   S      u32[groups][n_words*64 + 1][rw]   "sliced" matrix (last row of a group: all ones, the target of predicated-off
//                                    gathers): row = bit index, column = leaf (left-to-right DFS order) followed by guard
//                                    columns (ancestors whose ⊇ check failed).  One 128-B line answers the same probe for
//                                    1024 leaves.  Trees of more than 2048 columns are cut into column groups of 2048
//                                    (rw = 64 each); the frontier kernels run once per group.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfq_device.h"

namespace pfq {

// Per-wave reservations in the deferred-pair buffer (slots) and in the miss-word buffer (u64 words): every wave of every
// classify launch may leave one of each partly used, which the host adds to the buffers' sizes.
// Experiment switches of k_tile_bin that give wrong results are compiled in with -DPFQ_EXPERIMENTS only: no environment
// variable or option can change the results of the library as shipped.
#ifdef PFQ_EXPERIMENTS
#define PFQ_DEBUG_BITS(a) ((a).debug)
#else
#define PFQ_DEBUG_BITS(a) 0u
#endif
constexpr uint32_t PAIR_RESERVE = 32, MISS_RESERVE = 256;
enum StatSlot { ST_CANDIDATES = 0, ST_HITS = 1, ST_ALLHIT = 2, ST_ALG_BYTES = 3, ST_DEFERRED = 4, ST_LISTED = 5 /* (read, leaf group) entries of a two-level frontier */, ST_BATCHED = 6 /* pairs emitted a pass at a time */, ST_PAIR_RESERVATIONS = 7 /* reservations the classify launches made in the pair buffer */, ST_N = 8 };

struct QueryArgs {
    HashParams hp;
    const uint8_t *seq;
    const uint64_t *off;
    uint64_t n_reads;
    float threshold;
    // sliced matrix
    const uint32_t *S;           // the column group this launch screens
    const uint32_t *S_all;       // group 0 (certificates of arbitrary columns: guards may live in another group)
    uint64_t group_stride;       // dwords between the matrices of consecutive groups
    uint32_t col0;               // first column of this launch's group (columns are global everywhere else)
    uint32_t group_log2;         // log2 of the columns per group of the sliced matrix (11; 10 for trees with a coarse level)
    // two-level frontier (trees of several column groups): the launch of a leaf group only sees the reads the coarse launch
    // (k_coarse) listed for it — reads with a live ancestor of one of the group's leaves
    const uint32_t *read_list;   // reads of this launch (entries 0xffffffff: unused slots of a reservation), nullptr: all reads
    const unsigned int *n_list;  // slots of read_list in use
    // ONE launch serves every leaf group of a two-level frontier: blockIdx.y = the group; S, col0, n_leaves, read_list, n_list
    // (and long_list / n_long) of the group follow from these (the host passes group 0's pointers)
    uint32_t grid_groups;        // leaf groups of the launch (0: the launch is for the one group the fields above describe)
    uint32_t total_leaves;       // leaves of the tree
    uint32_t list_cap;           // slots per group in read_list and long_list
    uint32_t first_group;        // 1: this launch accounts for the per-read statistics (read bytes, all-hit reads)
    uint32_t ones_row;           // index of the all-ones row stored behind the last bit row of S
    uint32_t rw, rw_log2;        // row words (power of two <= 64)
    uint32_t n_leaves, n_cols;   // leaf columns of this group; leaf+guard columns of the tree
    const uint32_t *guard_off;   // [total leaves + 1] CSR into guard_col (may be all zeros), indexed by global leaf column
    const uint32_t *guard_col;   // global columns
    // results
    unsigned long long *counts;  // [n_leaves]  mapped_reads, accumulating (query.rs:143)
    uint2 *hit_pairs;            // (read, leaf) or nullptr
    uint64_t hit_cap;
    unsigned long long *hit_cursor;
    uint8_t *allhit_flag;        // per read: passes everything (need == 0), or nullptr
    unsigned long long *stats;   // [ST_N]
    // deferral to the bucketed verify pass (DEFER kernels only)
    uint2 *pairs;
    uint64_t pair_cap;
    unsigned long long *pair_cursor;
    uint32_t *bucket_cnt;        // [n_leaves << sub_log2]: bucket = (leaf << sub_log2) | (read & (subs-1))
    uint32_t sub_log2;           // sub-buckets per leaf (so that no counter is a hot spot when leaves are few)
    uint32_t pair_ahead;         // A: a batched emission that has to reserve asks for up to A further reservations of PAIR_RESERVE slots
                                 // for the wave's next passes (PFQ_PAIR_AHEAD; 0: what the pass needs and no more)
    uint4 *recs;                 // probe records, indexed by (read byte offset + k-mer position), or nullptr
    uint64_t rec_cap;            // entries in recs (reads whose records would not fit are certified inline)
    uint32_t *long_list;         // thresholds < 1: reads of >= 256 k-mers, classified by a second launch (wider counters)
    unsigned int *n_long;
    uint32_t batch_tails;        // theta == 1 with records: last windows of <= batch_tails k-mers (0: none, 16 or 32) are left to k_tail_records
    uint32_t split_recs;         // 1 (theta == 1 with records): k_classify only defers; k_tail_records makes every record of a deferred read
    uint32_t block_pairs;        // 1 (DEFER, theta == 1, no guard columns): defer (read, block of 8 leaves | candidate mask << 24)
    uint32_t batch_emit;         // 1 (DEFER, theta == 1, leaf pairs): the survivors of a pass of the dense screen are emitted together (PFQ_BATCH_EMIT)
    uint32_t screen_recs;        // thresholds < 1: the dense counting screen writes the probe records of the k-mers it hashes
    uint32_t screen_only;        // (launches without deferral) count the frontier's candidate leaves, certify nothing, count no read
    uint32_t lean_screen;        // 1 (DEFER, theta == 1, leaf pairs, all reads, rw <= 32): the build whose dense screen takes 2 k-mers of 32 reads a pass (PFQ_SCREEN_KMERS)
    // thresholds < 1: every deferred pair owns ceil(n/64) u64 words of k-mer miss bits.  k_classify only accounts for
    // them (per bucket, and against the buffer's capacity through per-wave reservations); k_bucket_scatter places them.
    uint32_t *bucket_words;            // [n_leaves << sub_log2] miss words per bucket, or nullptr (threshold 1)
    unsigned long long *miss_cursor;   // words reserved so far
    uint64_t miss_cap;                 // words in the buffer
};

// Two-level frontier (k_coarse).  A tree of more than one column group gets a COARSE sliced matrix over an antichain of
// internal nodes that covers every leaf (each node as close to the leaves as <= 1024 / 2048 columns allow).  A read that
// does not pass a node reaches no leaf below it (query.rs:119-141 descends with the survivors only), whatever the
// threshold and whether or not the node's filter is a superset of its children's; the screens of the leaf groups then run
// on the reads listed for them instead of on every read.  Filters of internal nodes are fuller than those of leaves, so
// the coarse screens look at n_probes probes per k-mer instead of one (two at threshold 1).
constexpr uint32_t MAX_LEAF_GROUPS = 64;   // groups a coarse launch can list reads for (wider trees: flat frontier)
constexpr uint32_t COARSE_MAX_PROBES = 6;  // probes per k-mer of the coarse AND-screen (threshold 1); the counting screen takes <= 4
struct CoarseArgs {
    const uint32_t *cgrp;        // [coarse columns] first leaf group | last leaf group << 16 of the leaves below the column's node
    uint32_t n_groups;           // leaf groups (<= MAX_LEAF_GROUPS)
    uint32_t *lists;             // [n_groups][list_cap] reads per leaf group, appended through per-wave reservations of 32
    unsigned int *cursors;       // [n_groups] slots handed out
    uint32_t list_cap;           // >= n_reads + 32 per wave of the launch: no list can overflow
    uint32_t n_probes;           // probes per k-mer the coarse screen looks at
    uint32_t scr_extra;          // counting screen: k-mers looked at beyond maxmiss + 1
    uint32_t total_leaves;       // reads that pass every node count at every leaf of the tree
};
void launch_coarse(const QueryArgs &a, const CoarseArgs &ca, bool counts_mode, int blocks, hipStream_t st);
// out[i] = set bits of filter row rows[i]
void launch_row_popcount(const uint64_t *bits, uint64_t n_words, const uint32_t *d_rows, uint32_t n_rows, unsigned long long *d_out, hipStream_t st);

// Guard pairs (k_expand_guards): second region of the pair buffer, slots slot0 .. slot0 + cap of the whole buffer.
struct GuardArgs {
    uint2 *pairs;                // = pair buffer + slot0
    uint64_t cap;                // slots in the region (whole reservations of 32)
    unsigned long long *cursor;  // slots reserved so far
    uint32_t slot0;              // index of the region's first slot in the whole pair buffer
    uint32_t *owner;             // [whole pair buffer] slot of the leaf pair a slot belongs to (a leaf pair owns itself)
    uint32_t *gfail;             // [whole pair buffer] indexed by the leaf pair's slot: a guard of it did not pass
};
void launch_expand_guards(const QueryArgs &a, const GuardArgs &ga, int blocks, hipStream_t st);

struct ChunkDesc;
struct VerifyArgs {
    HashParams hp;
    const uint8_t *seq;
    const uint64_t *off;
    const uint64_t *bits;        // node-major filters
    const uint32_t *col_row;     // column -> filter row
    uint64_t n_words;
    const uint2 *sorted;         // (read, leaf) sorted by leaf
    const uint4 *meta;           // per sorted pair: (read byte offset lo, hi, read length, filter row)
    const uint32_t *n_pairs_ptr; // &bucket_off[n_leaves]
    uint32_t *fail;              // [pair_cap]
    uint32_t n_slices, slice_bits;
    unsigned int *queue;         // work cursors: [n_slices] (re-hash kernel) / [8 * n_sub] (record kernel)
    uint32_t n_sub;              // sub-queues per XCD (record kernel)
    uint32_t only_flagged;       // fallback after the LDS-tile pass, pairs whose fail word has bit 1 set: 1 = from the compact
                                 // list when they are few, 2 = by walking all sorted pairs when they are many
    uint32_t flag_cap;           // entries of flag_list
    // the tile passes are launched without waiting for the plan: chunks of passes >= launched_passes (their number
    // was guessed from the previous call) are certified here as well (mode 2)
    const uint32_t *pair_chunk;
    const struct ChunkDesc *chunks;
    const unsigned long long *entry_cursor;
    uint64_t entry_cap;
    uint32_t launched_passes;
    const unsigned int *n_flagged;  // number of such pairs (kernel returns at once when 0)
    const uint32_t *flag_list;      // their sorted-pair indices
    const uint4 *recs;           // probe records written by k_classify<DEFER> (nullptr: re-hash per slice)
    unsigned long long *miss_words;  // thresholds < 1: bit q of the pair's words = a probed bit of its k-mer q is 0
    const uint32_t *miss_pos;        // [sorted pair] first word of the pair (nullptr at threshold 1: any miss fails the pair)
    uint32_t chunk;
};

struct FinalizeArgs {
    HashParams hp;
    const uint64_t *off;
    const uint2 *sorted;
    const uint32_t *bucket_off;  // [(n_leaves << sub_log2) + 1]
    uint32_t sub_log2;
    const uint32_t *fail;
    const unsigned long long *miss_words;  // thresholds < 1 (see VerifyArgs); nullptr at threshold 1
    const uint32_t *miss_pos;
    float threshold;
    uint32_t c0, c1;             // buckets (columns) of this launch: the guard columns first, then the leaves
    uint32_t guards;             // 1: guard columns — a pair that does not pass marks its leaf pair in gfail; no counts, no hits
    const uint32_t *owner_sorted;  // trees with guard columns: per sorted pair, the slot of its leaf pair (else nullptr)
    uint32_t *gfail;             // per pair slot: a guard of this leaf pair did not pass
    unsigned long long *counts;
    uint2 *hit_pairs;
    uint64_t hit_cap;
    unsigned long long *hit_cursor;
    unsigned long long *stats;
    unsigned long long *n_dirty;  // thresholds < 1: += pairs with at least one k-mer missing (sizes the next call's certificate stage)
    const uint8_t *failb;         // block mode (else nullptr): sorted pairs are (read, block | mask << 24), [pair][8] failure bytes
    // thresholds < 1 after LDS-tile passes with k-mer entries: a pair that was binned in a launched pass and never flagged
    // has its miss bits in its chunk's bitmap (kmiss); every other pair in its own miss words (written by k_verify_rec)
    const uint8_t *kmiss;         // nullptr: miss words only
    const uint8_t *kall;          // block mode with k-mer entries (see TileArgs)
    const uint32_t *pair_kpos;
    const uint32_t *pair_chunk;
    const ChunkDesc *chunks;
    uint32_t launched_passes;
};

// ---- LDS-tile certificates (bucketed path, records available) ------------------------------------------------------
// Every probe of every sorted pair is binned by (chunk of <= 4096 pairs of one leaf, 2^20-bit tile of the filter);
// a block then loads one tile of one leaf into LDS and tests all its probes there.
constexpr uint32_t TILE_LOG2 = 20;                 // bits per tile = 128 KiB of filter (one 1024-thread test block per CU;
                                                   // 64 KiB tiles, two blocks per CU: bin 11.4 / test 5.9 ms vs 10.8 / 5.9)
constexpr uint32_t CHUNK_PAIRS_LOG2 = 10;          // pairs per chunk: local pair id and tile offset share one u32 entry; a chunk
                                                   // is the work item of k_tile_bin (one block bins it alone)
constexpr uint32_t MAX_TILES = 1024;               // tiles per filter the passes take (k_tile_bin keeps a bin per tile in LDS)
// Thresholds < 1: the passes must tell WHICH k-mers are not contained, so an entry names a k-mer instead of a pair:
// [round tag : 2][k-mer of the round : 11][offset in tile : 19] — k_tile_bin bins a chunk in rounds of <= 2^11 flattened
// k-mers, the four entries of a 16-byte vector (runs are 16-byte aligned) carry the round's number in their tag bits, and
// round_k0[chunk][round] turns (round, k-mer of the round) into the k-mer's position in the chunk's miss bitmap.
constexpr uint32_t TILE_LOG2_COUNTS = 19;          // 64 KiB tiles (twice the tiles, 128-entry deeper bins than needed)
constexpr uint32_t ROUND_KMERS_LOG2 = 11;          // flattened k-mers per round of k_tile_bin (= 2 windows x 16 waves)
constexpr uint32_t MAX_ROUNDS = 256;               // rounds per chunk the tags can name; later pairs take the fallback
// Threshold 1, packed entries (TileArgs::entry_pack): a 16-byte vector of a bucket holds FIVE 24-bit entries [pair of the
// round : 4][offset in tile : 20], entry j in bits 24 j .. 24 j + 23, and in bits 120..127 the number of the k_tile_bin round
// the run belongs to.  round_p0[chunk][round] is the round's first pair (in the chunk); a run — the entries of one (round,
// tile) — is padded to a whole vector with copies of its last entry.  Fill marks and capacities stay in 32-bit words.
constexpr uint32_t PACK_PAIRS = 16;                // pairs per round the 4-bit id can name
constexpr uint32_t PACK_ROUNDS = 256;              // rounds per chunk the tag can name; later pairs take the fallback
// 32-bit words of a bucket of `cap` words that packed entries use: room for `cap` entries, as with 32-bit entries — the same
// probes overflow into the fallback in either format, and the plan's capacities can shrink by the spare fifth later.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t pack_bucket_words(uint32_t cap) { return cap / 5u * 4u; }
// k-mers a round of k_tile_bin<waves, cap> takes: the bins fill to 3/4 on average (shallow bins of many tiles — block mode —
// to 1/2: an overflow costs the round's pairs the fallback, and 30 +- 5.5 entries must stay below 60), and at most
// TILE_BIN_WPI windows of 64 k-mers a wave.  (The host chooses the entry format of a call from it.)
constexpr uint32_t TILE_BIN_WPI = 2;
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t tile_bin_kmer_budget(uint32_t waves, uint32_t cap, uint32_t n_tiles, uint32_t num_hashes, bool counts) {
    uint32_t kb = (uint32_t)(((uint64_t)(cap < 128 ? cap / 2 : cap - cap / 4) * n_tiles) / (num_hashes ? num_hashes : 1u));
    if (kb > TILE_BIN_WPI * waves * 64u) kb = TILE_BIN_WPI * waves * 64u;
    if (counts && kb > (1u << ROUND_KMERS_LOG2)) kb = 1u << ROUND_KMERS_LOG2;
    return kb ? kb : 1u;
}
// Reads that pass several related leaves (a phage database is full of strains): BLOCK MODE.  A pair is (read, block of 8
// consecutive leaf columns, mask of the candidate leaves in it); the block's "filter" is a byte per Bloom bit index — bit j =
// that bit of leaf 8b + j — so ONE entry tests a probe for all candidate leaves of the block: a read that passes 8 strains
// costs the probes of one pair instead of eight.  The pairs are bucketed by (block, candidate mask): all pairs of a chunk
// share their mask, which travels in the chunk's descriptor, and the entries stay [pair of the chunk:10][byte offset in a
// 128 KiB tile:17] (threshold 1) or [round tag:2][k-mer:11][byte offset:17] (thresholds below 1: the miss array then holds
// 8 bytes per k-mer, one per leaf of the block).  The columns of the passes are the blocks, whatever the buckets.
constexpr uint32_t TILE_LOG2_BLOCK = 17;           // 2^17 bit indices x 8 leaves = 128 KiB
constexpr uint32_t BLOCK_LEAVES_LOG2 = 3;
struct ChunkDesc {
    uint32_t row;      // filter row of the leaf (block mode: the block)
    uint32_t first;    // first sorted pair
    uint32_t n;        // pairs
    uint32_t cap;      // entries per (chunk, tile) bucket; 0: no room, the chunk's pairs take the fallback
    uint64_t base;     // first entry of tile 0's bucket
    uint32_t leaf;
    uint32_t pass;     // the probe buckets are reused: chunks are binned and tested pass after pass
    uint32_t kbase;    // thresholds < 1: where the chunk's k-mer miss array starts, in 16-byte units (a byte per k-mer of the chunk
                       // in the order of its pairs; block mode: 8 bytes per k-mer, one per leaf of the block)
    uint32_t kwords;   //                 its size in 16-byte units
    uint32_t mask;     // block mode with k-mer entries: the candidate mask all pairs of the chunk share
    uint32_t pad_;
};
struct TileArgs {
    uint32_t pass;               // k_tile_bin / k_tile_test: only the chunks of this pass
    HashParams hp;
    const uint64_t *bits;
    uint64_t n_words;
    const uint4 *recs;
    const uint4 *meta;           // per sorted pair (read offset lo, hi, length, row)
    const uint32_t *col_row;     // column -> filter row
    const uint32_t *bucket_off;  // [(n_leaves << sub_log2) + 1]
    uint32_t sub_log2, n_leaves, n_tiles;   // n_leaves: buckets = leaf + guard columns
    uint32_t bin_shape;          // 0 auto, 1 force the 8 x 128 build of k_tile_bin, 2 force 16 x 256
    uint32_t debug;              // builds with -DPFQ_EXPERIMENTS only (timing experiments, results wrong): 1 no bucket stores, 2 no LDS binning,
                                 // 8 / 16 block mode without the flags of full bins / full buckets.  The default build ignores the field.
    ChunkDesc *chunks;           // [max_chunks]
    uint32_t max_chunks;
    uint32_t *leaf_chunk0;       // [n_leaves + 1] first chunk of each leaf (chunks of a leaf are contiguous)
    uint32_t *pair_chunk;        // [pair_cap] chunk of each sorted pair
    unsigned int *n_chunks;      // counter
    unsigned long long *entry_cursor;  // virtual: pass = cursor / entry_cap, position in the pass = cursor % entry_cap
    uint64_t entry_cap;
    uint32_t *entries;
    unsigned int *gfill;         // [max_chunks * n_tiles] entries (and padding) in every bucket, written by k_tile_bin
    unsigned int *bin_queue;     // k_tile_bin of this pass: next chunk to take
    uint32_t *fail;              // bit 0: a probed bit was 0; bit 1: pair must be verified by the fallback kernel
    unsigned int *n_flagged;     // pairs with bit 1
    uint32_t *flag_list;         // [flag_cap] their sorted-pair indices
    uint32_t flag_cap;
    const uint32_t *n_pairs_ptr;
    // block mode (see TILE_LOG2_BLOCK)
    uint32_t blocks;             // 1: pairs are (read, block | mask << 24), meta.w likewise; bits = block tables, n_words = bytes / 8 of one
                                 // (with `counts`: buckets = (block << 8) | mask, n_leaves = blocks: a column of the passes is a block)
    uint32_t chunk_log2;         // pairs per chunk (CHUNK_PAIRS_LOG2)
    uint8_t *failb;              // block mode: [sorted pair][8] a probed bit of that candidate leaf was 0
    // thresholds < 1 (entries name k-mers, see TILE_LOG2_COUNTS)
    float threshold;             // (which prefix of a read's k-mers is binned depends on it)
    uint32_t counts;             // 1: k-mer entries, 64 KiB tiles, miss bits; 0: pair entries, 128 KiB tiles, fail words
    uint8_t *kmiss;              // k-mer miss bytes of all chunks (a byte, not a bit: set with plain stores from any XCD)
    uint64_t kmiss_cap;          // its bytes, < 2^32 (chunks that find no room take the fallback)
    unsigned long long *kmiss_used;  // bytes handed out by k_tile_assign (cleared before the passes)
    uint8_t *kall;               // block mode: [k-mer] the k-mer is in no candidate leaf of its pair's block (one byte for all eight)
    uint32_t *round_k0;          // [max_chunks][MAX_ROUNDS] position (in the chunk) of the first k-mer of every round
    uint32_t *n_rounds;          // [max_chunks]
    uint32_t *pair_kpos;         // [sorted pair] position of the pair's first k-mer in its chunk
    // position slots of sparse columns (k_tile_test<0> only; both null: every tile is loaded dense)
    const uint32_t *tile_list_row;  // [n_leaves] the column's row of slots, TILE_LIST_NONE: dense
    const uint32_t *tile_lists;     // [row][n_tiles][TILE_LIST_CAP]
    unsigned long long *tile_list_stats;  // [0] += tiles built from slots, [1] += tiles loaded dense (k_tile_test<0>)
    uint32_t tile_stream;           // 1: EVERY column has slots (tile_list_row[c] == c for all columns): the slots-only build runs
    // packed entries (threshold 1 outside block mode, see PACK_PAIRS)
    uint32_t entry_pack;            // 1: five 24-bit entries and the round's number per 16-byte vector; n_rounds is written too
    uint32_t *round_p0;             // [max_chunks][PACK_ROUNDS] first pair (in the chunk) of every round
    uint8_t *round_fail;            // [max_chunks][PACK_ROUNDS][PACK_PAIRS] 1: a probed bit of that pair of the round was 0 (cleared
                                    // by k_tile_bin with the round, set by k_tile_test with plain stores, read by k_pack_fail)
};
// after the last pass of a call with packed entries: the failures k_tile_test left in round_fail become fail words
void launch_pack_fail(const TileArgs &a, hipStream_t st);
// the build of k_tile_bin that launch_tile_bin launches for these arguments: BIN_WAVES << 16 | BIN_CAP
uint32_t tile_bin_build(const TileArgs &a);
// Position slots (pfq_tilelist.hip): a column whose filter has at most TILE_LIST_CAP set bits in every 2^TILE_LOG2-bit tile
// keeps, per tile, the tile-relative positions of the set bits in any order, the unused entries TILE_LIST_NONE — 32 KiB
// in the place of the tile's 128 KiB.  The cap is what 1024 threads hold as two 16-byte loads each.
constexpr uint32_t TILE_LIST_CAP = 8192;
constexpr uint32_t TILE_LIST_NONE = 0xffffffffu;
// col_max[col] = max over the column's tiles of the tile's set bits (the caller zeroes col_max)
void launch_tile_list_count(const uint64_t *bits, uint64_t n_words, const uint32_t *col_row, uint32_t n_cols, uint32_t n_tiles, uint32_t *col_max,
                            hipStream_t st);
// row r of `lists` = the slots of column list_cols[r]
void launch_tile_list_fill(const uint64_t *bits, uint64_t n_words, const uint32_t *col_row, const uint32_t *list_cols, uint32_t n_list_cols, uint32_t n_tiles,
                           uint32_t *lists, hipStream_t st);
void launch_tile_plan(const TileArgs &a, hipStream_t st);
// returns the build it launched: BIN_WAVES << 16 | BIN_CAP of k_tile_bin (chosen from n_tiles by its LDS need, and bin_shape)
uint32_t launch_tile_bin(const TileArgs &a, int blocks, hipStream_t st);
void launch_tile_test(const TileArgs &a, int blocks, hipStream_t st);

// launches (all asynchronous on `st`)
void launch_classify(const QueryArgs &a, bool defer, bool counts_mode, int blocks, hipStream_t st);
// after launch_classify when a.batch_tails or a.split_recs; ORs into *shapes which passes served a pair: TAIL_SHAPE_4 / _16 /
// _32 (last windows, a.batch_tails) and TAIL_SHAPE_FULL (a.split_recs: the 64-k-mer pass made a read's other windows);
// shapes[2] is the kernel's work counter and must be zero (the host clears both with the call's cursors)
constexpr uint32_t TAIL_SHAPE_4 = 1, TAIL_SHAPE_16 = 2, TAIL_SHAPE_32 = 4, TAIL_SHAPE_FULL = 8;
void launch_tail_records(const QueryArgs &a, unsigned int *shapes, int blocks, hipStream_t st);
void launch_bucket_scan(const uint32_t *bucket_cnt, uint32_t *bucket_off, uint32_t *bucket_cur, uint32_t n, hipStream_t st);
// words_off / words_cur / miss_pos: thresholds < 1 (miss words of a bucket start at words_off[bucket]); else nullptr
// key_mode 0: the bucket of a pair is its column; 1 (block mode): the block = low 24 bits of its second word, which goes to
// meta.w whole; 2 (block mode with k-mer entries): (block << 8) | candidate mask
// Returns the kernel the bucket count selected: SORT_SLICED (an LDS histogram per slice of slots, one global atomic per
// bucket and slice) or SORT_PER_PAIR (more buckets than LDS holds: one global atomic per pair).
constexpr uint32_t SORT_SLICED = 1, SORT_PER_PAIR = 2;
uint32_t launch_bucket_scatter(const uint2 *pairs, const unsigned long long *n_pairs_ptr, uint64_t pair_cap,
                               const uint32_t *bucket_off, uint32_t *bucket_cur, uint32_t n_buckets, uint32_t sub_log2, uint2 *sorted,
                               uint4 *meta, const uint64_t *read_off, const uint32_t *col_row, const uint32_t *words_off,
                               uint32_t *words_cur, uint32_t *miss_pos, uint32_t kmer_size, const uint32_t *owner,
                               uint32_t *owner_sorted, uint32_t key_mode, hipStream_t st);
// block tables: T[b][i] = byte whose bit j is bit i of the filter of leaf column 8b + j (zero for columns past the last leaf)
void launch_block_tables(const uint64_t *bits, uint64_t n_words, const uint32_t *d_col_row, uint32_t n_leaves, uint8_t *T, hipStream_t st);
// block mode: flagged pairs (fail bit 1) certified leaf by leaf against the sliced matrix; then the counts / hits of all pairs
// (chunks == nullptr: no tile passes ran, every pair is certified here)
// (n_flagged / flag_list: the compact list of the flagged pairs, when the tile passes ran)
void launch_block_fallback(const QueryArgs &a, const uint2 *sorted, const uint32_t *n_pairs_ptr, const uint32_t *fail, uint8_t *failb,
                           const uint32_t *pair_chunk, const ChunkDesc *chunks, uint32_t launched_passes, const unsigned int *n_flagged,
                           const uint32_t *flag_list, uint32_t flag_cap, hipStream_t st);
// block mode with k-mer entries: turns the miss bytes of the binned pairs into failure bytes (FinalizeArgs: fail, kmiss, kall,
// pair_kpos, pair_chunk, chunks, launched_passes, sorted, off, hp, threshold)
void launch_block_count(const FinalizeArgs &a, const uint32_t *n_pairs_ptr, uint8_t *failb, hipStream_t st);
// block mode on trees with guard columns: a candidate leaf that has not failed passes only if its guards pass (certified
// against the sliced matrix)
void launch_block_guards(const QueryArgs &a, const uint2 *sorted, const uint32_t *n_pairs_ptr, uint8_t *failb, hipStream_t st);
void launch_verify(const VerifyArgs &a, int blocks, int threads, hipStream_t st);
// list = the sorted pairs with a non-zero fail word, in order within runs; *n_out += their number (thresholds < 1 after tile passes)
void launch_collect_open(const uint32_t *fail, const uint32_t *n_pairs_ptr, uint32_t *list, uint32_t cap, unsigned int *n_out, hipStream_t st);
void launch_finalize(const FinalizeArgs &a, hipStream_t st);
// thresholds < 1 after tile passes with k-mer entries: flags (fail bit 1) the binned pairs whose prefix of k-mers does not decide them
void launch_prefix_open(const FinalizeArgs &a, const uint4 *meta, const uint32_t *n_pairs_ptr, uint32_t *fail, hipStream_t st);

void launch_insert(const HashParams &hp, const uint8_t *d_genomes, const uint64_t *d_goff, uint32_t n_genomes,
                   const uint32_t *d_leaf_row, uint64_t *bits, uint64_t n_words, hipStream_t st);
// one genome (device memory, len bytes) into filter row `row`
void launch_insert_one(const HashParams &hp, const uint8_t *d_genome, uint64_t len, uint32_t row, uint64_t *bits, uint64_t n_words, hipStream_t st);
// The greedy placement of one new leaf (BloomTree::insert, bloom_tree.rs:187-245) walked on the device in one launch; the tree's
// shape is mirrored in device memory: a TopoNode per node, state[0] = the root's index (-1: empty; state[2 + (seq & 1)] is
// where launch number seq reads it, state[2 + (~seq & 1)] where it leaves it), state[1] = error word
// (1: a node with one child was met; 2: the grid's barrier timed out; a launch that finds it set returns at once),
// sync = GREEDY_SYNC_LINES lines of GREEDY_SYNC_STRIDE bytes, zeroed once (the barrier's counters, generation words and
// distance accumulators, a line each: see grid_turn).
// `blocks` must not exceed the number of CUs (every block has to be resident).
struct TopoNode {
    int32_t left, right;   // node indices, -1: none
    uint32_t row;          // filter row
    uint32_t pad_;
};
constexpr int GREEDY_MAX_BLOCKS = 256;
constexpr uint32_t GREEDY_SYNC_STRIDE = 4096, GREEDY_SYNC_LINES = 49;
void launch_greedy_insert(uint64_t *bits, uint64_t n_words, TopoNode *topo, int *state, unsigned long long *sync, int leaf_node, int internal_node,
                          uint32_t new_row, uint32_t int_row, uint32_t seq, int blocks, hipStream_t st);
// dst[i] = a[i] | b[i] over rows given as triples (dst,a,b); b == 0xffffffff: copy a.
void launch_union(uint64_t *bits, uint64_t n_words, const uint32_t *d_triples, uint32_t n_triples, hipStream_t st);
// bits[cur] |= bits[new]; per-block partial Hamming distances: sum_b d_out[2b] = hamming(bits[left], bits[new]),
// sum_b d_out[2b+1] = hamming(bits[right], bits[new]), b < INSERT_STEP_BLOCKS
constexpr uint32_t INSERT_STEP_BLOCKS = 1024;
void launch_insert_step(uint64_t *bits, uint64_t n_words, uint32_t cur_row, uint32_t new_row, uint32_t left_row,
                        uint32_t right_row, unsigned long long *d_out, hipStream_t st);
// fail[e] != 0 iff child has a bit the parent lacks
void launch_superset(const uint64_t *bits, uint64_t n_words, const uint32_t *d_edges /*(parent,child)*/, uint32_t n_edges,
                     uint32_t *d_fail, hipStream_t st);
void launch_transpose(const uint64_t *bits, uint64_t n_words, const uint32_t *d_col_row, uint32_t n_cols, uint32_t *S,
                      uint32_t rw, uint64_t group_stride, uint32_t group_log2, hipStream_t st);
// dst[i] = a[i] + b[i], or a[i] - b[i] (u64 counters; the count reductions over replicas / ranks work on what a replica
// counted since it was opened: counters - base)
void launch_counts_op(unsigned long long *dst, const unsigned long long *a, const unsigned long long *b, uint32_t n, bool subtract, hipStream_t st);
// PFQ_WANT_HITS: the CSR read -> leaves from the unordered (read, leaf) hit pairs, on the device.  launch_hits_csr: counts per
// read (d_cnt, zeroed by the caller; reads flagged in d_allhit list every leaf) and their exclusive scan d_off[n_reads + 1];
// launch_hits_fill: the leaves, ascending within a read.  d_sums: ceil(n_reads / 4096) + 1 words of scratch.
void launch_hits_csr(const uint2 *d_pairs, uint64_t n_pairs, const uint8_t *d_allhit, uint64_t n_reads, uint32_t n_leaves, bool any_allhit,
                     uint32_t *d_cnt, unsigned long long *d_sums, unsigned long long *d_off, hipStream_t st);
void launch_hits_fill(const uint2 *d_pairs, uint64_t n_pairs, const uint8_t *d_allhit, uint64_t n_reads, const unsigned long long *d_off,
                      uint32_t *d_cnt, uint32_t *d_leaves, hipStream_t st);
// PFQ_WANT_SCORES: d_scores[j] = the number of k-mers of read r contained in the filter of hit leaf d_hit_leaves[j],
// d_hit_off[r] <= j < d_hit_off[r + 1] (the CSR of launch_hits_fill); column c's filter is row d_col_row[c] of d_bits.
void launch_hit_scores(const HashParams &hp, const uint8_t *d_seq, const uint64_t *d_off, uint64_t n_reads, float threshold,
                       const unsigned long long *d_hit_off, const uint32_t *d_hit_leaves, const uint32_t *d_col_row, const uint64_t *d_bits,
                       uint64_t n_words, uint32_t *d_scores, hipStream_t st);
// PFQ_PAIRED: reads 2f and 2f + 1 are the mates of fragment f; its hit set is the union (both = false) or the intersection of
// theirs.  Input: the mate CSR of launch_hits_csr / launch_hits_fill with any_allhit = false (all-hit mates: d_allhit only).
// launch_pair_combine: the fragment CSR's offsets d_frag_off[n_frag + 1] (count, then the scan of launch_hits_csr; d_cnt
// [n_frag], d_sums as there, d_long [n_frag] a queue for waves, d_misc [2] zeroed by the caller: queued fragments, all-leaf
// fragments left unlisted).  list_all: an all-leaf fragment lists every leaf (else it only counts, in d_misc[1]).
// launch_pair_fill: the lists, ascending.  launch_pair_leaf_counts: adds the fragments' leaf counts to d_counts (d_total =
// d_frag_off + n_frag; max_entries: a bound on it, sizes the grid).  launch_pair_scores: per listed (fragment, leaf), the
// k-mers of both mates the leaf's filter contains.
void launch_pair_combine(const unsigned long long *d_hit_off, const uint32_t *d_hit_leaves, const uint8_t *d_allhit, uint64_t n_frag, bool both,
                         uint32_t n_leaves, bool list_all, uint32_t *d_cnt, uint32_t *d_long, unsigned long long *d_misc, unsigned long long *d_sums,
                         unsigned long long *d_frag_off, hipStream_t st);
void launch_pair_fill(const unsigned long long *d_hit_off, const uint32_t *d_hit_leaves, const uint8_t *d_allhit, uint64_t n_frag, bool both,
                      uint32_t n_leaves, const uint32_t *d_long, const unsigned long long *d_misc, const unsigned long long *d_frag_off,
                      uint32_t *d_frag_leaves, hipStream_t st);
void launch_pair_leaf_counts(const uint32_t *d_frag_leaves, const unsigned long long *d_total, const unsigned long long *d_misc, uint32_t n_leaves,
                             uint64_t max_entries, unsigned long long *d_counts, hipStream_t st);
void launch_pair_scores(const HashParams &hp, const uint8_t *d_seq, const uint64_t *d_off, uint64_t n_frag, float threshold, bool both,
                        const unsigned long long *d_frag_off, const uint32_t *d_frag_leaves, const uint32_t *d_col_row, const uint64_t *d_bits,
                        uint64_t n_words, uint32_t *d_scores, hipStream_t st);
// PFQ_WANT_LCA (pfq_lca.hip): d_lca[u] = clade of the lowest common ancestor of unit u's hit leaves (LCA_NO_CLADE: no hit) and
// here[that clade] += 1.  The tables describe the current leaf set: leaf_clade [n_leaves]; gap_min [levels][n_leaves], level j
// entry i = the smallest clade index among the LCAs of adjacent leaves (i, i + 1) .. (i + 2^j - 1, i + 2^j) — clades are in
// pre-order, so that is their shallowest; top_clade = the LCA of all leaves.
//   launch_lca_pairs: units = reads, from the unordered (read, leaf) hit pairs and the all-hit flags; d_span [n_reads], filled
//     with 0xff by the caller.
//   launch_lca_rows: units = rows of an ascending CSR; pair_mode 1 (either) / 2 (both): rows are fragments, d_allhit holds the
//     mates' flags and an empty row of an all-leaf fragment stands for every leaf; 0: d_allhit is not read.
//   launch_lca_best: rows reduced to the entries with the row's highest score first; d_span [n_units], d_long [n_units],
//     d_n_long zeroed by the caller.
constexpr uint32_t LCA_NO_CLADE = 0xffffffffu;
struct LcaTables {
    uint32_t n_leaves, n_clades, top_clade;
    const uint32_t *leaf_clade, *gap_min;
    unsigned long long *here;
};
void launch_lca_pairs(const uint2 *d_pairs, uint64_t n_pairs, const uint8_t *d_allhit, uint64_t n_reads, uint2 *d_span, const LcaTables &tb,
                      uint32_t *d_lca, hipStream_t st);
void launch_lca_rows(const unsigned long long *d_off, const uint32_t *d_leaves, uint64_t n_units, const uint8_t *d_allhit, int pair_mode,
                     const LcaTables &tb, uint32_t *d_lca, hipStream_t st);
void launch_lca_best(const unsigned long long *d_off, const uint32_t *d_leaves, const uint32_t *d_scores, uint64_t n_units, uint2 *d_span,
                     uint32_t *d_long, unsigned long long *d_n_long, const LcaTables &tb, uint32_t *d_lca, hipStream_t st);
// PFQ_ROWS_BEST (pfq_best.hip): the rows of the ascending CSR d_off / d_leaves [n_units], scored by d_scores (one score per
// entry), reduced to the entries at the row's highest score: d_best_off [n_units + 1], d_best_leaves [at most the rows'
// entries], ascending within a row like the rows themselves; an empty row stays empty, a row whose scores are all equal is
// kept whole.  Scratch: d_cnt [n_units], d_sums [ceil(n_units / 4096) + 1], d_long [n_units], d_n_long [1] zeroed by the caller.
// n_units = 0: nothing is written.
void launch_best_rows(const unsigned long long *d_off, const uint32_t *d_leaves, const uint32_t *d_scores, uint64_t n_units, uint32_t *d_cnt,
                      unsigned long long *d_sums, uint32_t *d_long, unsigned long long *d_n_long, unsigned long long *d_best_off,
                      uint32_t *d_best_leaves, hipStream_t st);
// PFQ_WANT_SWEEP (pfq_sweep.hip): the rows of the ascending CSR off / leaves [n_units] of reads, scored by scores (one score per
// entry), counted against the n_thr ascending thresholds thr (pfq.h "threshold sweep"): per entry pass[p * n_leaves + leaf] += 1
// with p = the thresholds whose need_kmers(thr[t], the read's k-mers) the score reaches; per unit tops[max p] += 1 and
// uniq[t * n_leaves + arg] += 1 for second <= t < max p.  read_off [n_units + 1]: the reads' offsets (for their lengths), k: the
// k-mer size.  long_list [n_units] and n_long [1] zeroed by the caller: the queue of rows a wave takes.  lds: count `pass` in the
// block's LDS where its (n_thr + 1) * n_leaves bins fit; needs (n_thr + 1) * n_leaves < 2^32.  n_units = 0: nothing runs.
constexpr uint32_t SWEEP_MAX = 16;          // (PFQ_SWEEP_MAX)
constexpr uint32_t SWEEP_GRID_ROWS = 1024;  // blocks of 256 threads of the thread-per-row kernel: units of one grid trip / 256
constexpr uint32_t SWEEP_GRID_LONG = 1024;  // blocks of WAVES_PER_BLOCK waves of the wave-per-row kernel
struct SweepArgs {
    const unsigned long long *off;
    const uint32_t *leaves, *scores;
    const uint64_t *read_off;
    uint64_t n_units;
    uint32_t k, n_thr, n_leaves;
    float thr[SWEEP_MAX];
    unsigned long long *pass, *uniq, *tops;
    uint32_t *long_list;
    unsigned long long *n_long;
};
void launch_sweep(const SweepArgs &a, bool lds, hipStream_t st);
// PFQ_WANT_TAXA (pfq_tax.hip): the units of the call's final ascending CSR d_off / d_leaves [n_units] counted on the nodes of the
// user's taxonomy (pfq.h "taxonomy"): d_node[u] = the deepest node above every leaf of row u (TAX_NO_NODE: an empty row),
// here[that node] += 1, any[t] += 1 for every node t above at least one leaf of the row.  The tables describe the current leaf
// set: rank, leaf_node [n_leaves]; parent, first_rank [n_nodes]; gap_min [levels][n_leaves], level j entry i = the smallest node
// index among the lowest common nodes of the adjacent ranks (i, i + 1) .. (i + 2^j - 1, i + 2^j) — nodes are in pre-order, so
// that is their shallowest; top_node = the deepest node above every leaf (nodes 0 .. top_node are the root's one-child chain).
// What the kernels leave out of here / any, exact and cheap to add at read-out: misc[TAX_MISC_HIT] += units with a hit, which is
// any[t] of every t <= top_node (the walks stop below them); misc[TAX_MISC_ALL] += rows that list all n_leaves leaves, each a
// unit of here[top_node] and of any[t] for every t > top_node (they walk nothing).  hot: up to TAX_HOT nodes below top_node that
// a wave counts with ballots instead of one atomic per lane (unused slots: TAX_NO_NODE).  Up to TAX_HIST_LDS nodes a block
// counts here and any in two u32 LDS histograms (dynamic LDS, 8 bytes per node: 64 KiB at the bound) and flushes once per node;
// above, global atomics.
// d_long [n_units]: queue of the rows of more than 64 entries, *d_n_long zeroed by the caller.
constexpr uint32_t TAX_NO_NODE = 0xffffffffu;
constexpr uint32_t TAX_HIST_LDS = 8192;
constexpr uint32_t TAX_HOT = 4;
enum { TAX_MISC_HIT = 0, TAX_MISC_ALL = 1, TAX_MISC_N = 2 };
struct TaxTables {
    uint32_t n_leaves, n_nodes, top_node;
    uint32_t hot[TAX_HOT];
    const uint32_t *rank, *leaf_node, *parent, *first_rank, *gap_min;
    unsigned long long *here, *any, *misc;
};
void launch_tax_rows(const unsigned long long *d_off, const uint32_t *d_leaves, uint64_t n_units, const TaxTables &tb, uint32_t *d_node,
                     uint32_t *d_long, unsigned long long *d_n_long, hipStream_t st);
// PFQ_WANT_ABUNDANCE (pfq_abund.hip): the device log of the calls' ambiguous rows and the EM over it.
//   launch_abund_count: d_cnt[ABUND_CNT_*] += what the CSR d_off [n_units] would add to the log, per class (a row's class
//     follows from its length: 0 unhit, 1 unique, n_leaves > 1 all leaves, else ambiguous) and the ambiguous rows' entries.
//   launch_abund_append: rows of the ascending CSR d_off / d_leaves [n_units].  A row of one leaf l: unique[l] += 1; a row of two
//     or more leaves that does not list all n_leaves: appended — cursors[0] rows and cursors[1] entries are in use, and the
//     caller has made room for what this CSR adds (row_cap, entry_cap: nothing is written beyond them).  Other rows: nothing.
//   launch_abund_start: a = 1 << ABUND_Q, nxt = unique << ABUND_Q.  launch_abund_step: nxt[l] += (a[l] << ABUND_Q) / D over the
//     rows (D = the row's sum of a; rows with D = 0 add nothing); blocks = 0: the built-in grid; lds = false: global atomics
//     only.  launch_abund_delta: *d_delta = max(*d_delta, max |nxt - a|), then a = unique << ABUND_Q (the next iteration's nxt).
constexpr uint32_t ABUND_Q = 16;
constexpr uint32_t ABUND_HIST_LDS = 8192;  // step: per-block u64 histogram in LDS up to this many leaves (64 KiB, two blocks per CU)
constexpr uint32_t ABUND_A_LDS = 4096;     // ... and a[] beside it up to this many
enum { ABUND_CNT_UNHIT = 0, ABUND_CNT_UNIQUE, ABUND_CNT_ALL, ABUND_CNT_ROWS, ABUND_CNT_ENTRIES, ABUND_CNT_N };
struct AbundLog {
    unsigned long long *row_start;  // [row_cap] first entry of the row
    uint32_t *row_len;              // [row_cap]
    uint32_t *entries;              // [entry_cap] leaf columns
    unsigned long long *cursors;    // [2] rows, entries in use
    unsigned long long *unique;     // [n_leaves]
    unsigned long long row_cap, entry_cap;
};
struct AbundStep {
    const unsigned long long *row_start;
    const uint32_t *row_len;
    const uint32_t *entries;
    uint64_t n_rows;
    uint32_t n_leaves;
    const unsigned long long *a;
    unsigned long long *nxt;
};
void launch_abund_count(const unsigned long long *d_off, uint64_t n_units, uint32_t n_leaves, unsigned long long *d_cnt, hipStream_t st);
void launch_abund_append(const unsigned long long *d_off, const uint32_t *d_leaves, uint64_t n_units, uint32_t n_leaves, const AbundLog &g,
                         hipStream_t st);
void launch_abund_start(unsigned long long *d_a, unsigned long long *d_nxt, const unsigned long long *d_unique, uint32_t n_leaves, hipStream_t st);
void launch_abund_step(const AbundStep &s, uint32_t blocks, bool lds, hipStream_t st);
void launch_abund_delta(unsigned long long *d_a, const unsigned long long *d_nxt, const unsigned long long *d_unique, uint32_t n_leaves,
                        unsigned long long *d_delta, hipStream_t st);
// PFQ_WANT_COVERAGE (pfq_cover.hip): per leaf a HyperLogLog sketch of the k-mers its units matched.  launch_cover_sketch: over
// the rows of the call's final CSR d_row_off / d_row_leaves [n_units] (pair_mode 0: unit u is read u; 1 either / 2 both: unit f
// is reads 2f, 2f + 1), per listed leaf l: units[l] += 1, matched[l] += the unit's k-mers whose probed bits are all set in l's
// filter (row d_col_row[l] of d_bits; what launch_hit_scores / launch_pair_scores count), and each of those k-mers raises one
// register of l: registers[l << precision | j] = max(.., rho).  blocks = 0: the built-in grid.
struct CoverArgs {
    uint8_t *registers;                   // [n_leaves << precision], 4-byte aligned
    unsigned long long *units, *matched;  // [n_leaves]
    uint32_t n_leaves, precision;         // precision: COVER_P_MIN .. COVER_P_MAX
};
constexpr uint32_t COVER_P_MIN = 4, COVER_P_MAX = 16, COVER_P_DEFAULT = 12;
void launch_cover_sketch(const HashParams &hp, const uint8_t *d_seq, const uint64_t *d_off, uint64_t n_units, float threshold, int pair_mode,
                         const unsigned long long *d_row_off, const uint32_t *d_row_leaves, const uint32_t *d_col_row, const uint64_t *d_bits,
                         uint64_t n_words, const CoverArgs &cv, uint32_t blocks, hipStream_t st);
// The exclusive scan behind launch_hits_csr on its own: d_off[i] = d_cnt[0] + .. + d_cnt[i - 1], i <= n (d_off[n]: the total);
// d_sums: ceil(n / 4096) + 1 words of scratch.  n = 0: nothing is written.
void launch_scan_u32(const uint32_t *d_cnt, uint64_t n, unsigned long long *d_sums, unsigned long long *d_off, hipStream_t st);
// pfq_query_frames (pfq_frames.hip): sequences cut into overlapping frames, the frames classified like reads, runs of frames
// that list a leaf merged into segments, every segment refined to k-mer resolution on the leaf's own filter.
//   launch_frame_count: per sequence its frames (d_cnt) and, for a sequence of one frame, what that frame is shorter than
//     `frame` (d_deficit); *d_err |= 1 if a sequence has 2^32 bases or more.  The caller scans both (launch_scan_u32).
//   launch_frame_cut: the frame table (sequence, start, byte offset of every frame) and the frames' bytes gathered into d_out,
//     a CSR buffer behind frame_off that the classify kernels read like any block of reads.
//   launch_seg_count: open_cnt[f] = entries of frame f's row that open a segment; the caller scans them into seg_pos.
//   launch_seq_seg_off: d_seq_seg_off[i] = first segment of sequence i, i <= n_seqs.
//   launch_seg_fill: the segments' leaf, first_frame, n_frames, begin, end, in CSR order; seg_seq their sequences; the leaf
//     counters += 1 per (sequence, distinct leaf among its segments).  queue [n_segs], *n_queued zeroed by the caller.
//   launch_piece_count: d_cnt[p] = pieces of at most `piece` k-mer positions of segment p; the caller scans them.
//   launch_seg_refine: one wave per piece probes the leaf's filter (row d_col_row[leaf] of d_bits) and leaves a FramePart;
//     then the pieces of a segment are folded in order into kmers, matched, match_begin, match_end, longest_run.
struct Segment {  // = pfq_segment (pfq.h)
    uint32_t leaf, first_frame, n_frames, begin, end, match_begin, match_end, kmers, matched, longest_run;
};
struct FramePart {  // a stretch of k-mer positions reduced (see part_join)
    uint32_t len, matched, first, last, pre, suf, best, pad_;
};
struct FrameArgs {
    const uint64_t *seq_off;                 // [n_seqs + 1] the caller's offsets
    uint64_t n_seqs, n_frames;
    uint32_t frame, step;
    const unsigned long long *seq_frame0;    // [n_seqs + 1] first frame of every sequence
    const unsigned long long *seq_deficit;   // [n_seqs + 1] scan of d_deficit
    uint32_t *frame_seq, *frame_start;       // [n_frames]
    uint64_t *frame_off;                     // [n_frames + 1]
};
struct SegArgs {
    const unsigned long long *row_off;       // [n_frames + 1] the frames' ascending CSR rows
    const uint32_t *row_leaves;
    uint64_t n_frames;
    uint32_t n_leaves;
    const uint32_t *frame_seq, *frame_start;
    const uint64_t *frame_off;
    const unsigned long long *seq_frame0;
    uint32_t *open_cnt;                      // [n_frames]
    const unsigned long long *seg_pos;       // [n_frames + 1]
    Segment *seg;
    uint32_t *seg_seq;                       // [n_segs]
    uint32_t *queue;                         // [n_segs] segments still open after the opening lane's walk
    unsigned long long *n_queued;
    unsigned long long *counts;              // the tree's leaf counters
};
void launch_frame_count(const uint64_t *d_seq_off, uint64_t n_seqs, uint32_t frame, uint32_t step, uint32_t *d_cnt, uint32_t *d_deficit,
                        unsigned long long *d_err, hipStream_t st);
void launch_frame_cut(const FrameArgs &fa, const uint8_t *d_seq, uint8_t *d_out, hipStream_t st);
void launch_seg_count(const SegArgs &sa, hipStream_t st);
void launch_seq_seg_off(const unsigned long long *d_seq_frame0, const unsigned long long *d_seg_pos, uint64_t n_seqs, unsigned long long *d_seq_seg_off,
                        hipStream_t st);
void launch_seg_fill(const SegArgs &sa, const unsigned long long *d_seq_seg_off, uint64_t n_seqs, uint64_t n_segs, hipStream_t st);
void launch_piece_count(const Segment *d_seg, uint64_t n_segs, uint32_t k, uint32_t piece, uint32_t *d_cnt, hipStream_t st);
void launch_seg_refine(const HashParams &hp, const uint8_t *d_seq, const uint64_t *d_seq_off, Segment *d_seg, const uint32_t *d_seg_seq,
                       const unsigned long long *d_piece_off, uint64_t n_segs, uint64_t n_pieces, uint32_t piece, const uint32_t *d_col_row,
                       const uint64_t *d_bits, uint64_t n_words, FramePart *d_parts, hipStream_t st);
constexpr uint32_t FRAME_PIECE_DEFAULT = 16384;  // k-mer positions per piece of the refinement (PFQ_FRAME_PIECE)
// pfq_tree_similarity (pfq_sim.hip): d_out[i * n_b + j] += the bits below nbits that filter row d_rows_a[i] of bits_a and filter
// row d_rows_b[j] of bits_b (both of n_words words) have in common.  d_out [n_a * n_b] must be zero: the tiled kernel cuts the
// words into `slices` ranges (0: the built-in choice; clamped to 1 .. chunks of 16 words) whose blocks add their partial counts
// with u32 atomics — the sums are exact whatever the slices and the order.  naive: one block per pair, no tiling, no atomics
// (the A/B baseline).  The rows may repeat and need no order; bits_a and bits_b may be one array.  Returns the slices launched
// (naive: 1; nothing to do: 0).  launch_filter_row_bits: d_out[i] = the bits below nbits of filter row d_rows[i].
uint32_t launch_filter_intersections(const uint64_t *bits_a, const uint32_t *d_rows_a, uint32_t n_a, const uint64_t *bits_b, const uint32_t *d_rows_b,
                                     uint32_t n_b, uint64_t n_words, uint64_t nbits, uint32_t slices, bool naive, uint32_t *d_out, hipStream_t st);
void launch_filter_row_bits(const uint64_t *bits, const uint32_t *d_rows, uint32_t n_rows, uint64_t n_words, uint64_t nbits, unsigned long long *d_out,
                            hipStream_t st);
// pfq_tree_recluster (pfq_cluster.hip): average linkage over the chance-corrected scores of the leaf filters, in integers.
// The score matrix d_S is u64 [n_slots][pitch] (pitch: a multiple of 16 columns, >= n_slots), a slot per cluster: the leaves
// start in slots 0 .. L - 1, a merge leaves the new cluster in its left child's slot and retires the right child's.
// d_meta [pitch]: (node index or CLUSTER_NONE, leaves of the cluster) per slot; d_slot_of [2 L - 1]: node -> slot or CLUSTER_NONE.
//   launch_cluster_scores: a panel of launch_filter_intersections — leaves r0 .. r0 + n_r against leaves r0 .. r0 + n_c, d_shared
//     [n_r][n_c] — turned into q (pfq.h "re-clustering") with d_pop = launch_filter_row_bits of all leaves; pairs above the
//     diagonal are written to both halves of d_S (the caller zeroes d_S once).
//   launch_cluster_nearest: d_best[slot] = the slot of the best other live cluster (score descending, node index ascending).
//   launch_cluster_mutual: d_flag[n] = 1 for a live node n whose best chose it back and has the larger index, n < n_nodes; the
//     caller scans the flags (launch_scan_u32) into d_pos.  launch_cluster_list: the flagged pairs at d_list[d_pos[n]].
//   launch_cluster_merge: the rows and the columns of the right children are added to the left children's, the slots retired,
//     merge p becomes node first_node + p.
constexpr uint32_t CLUSTER_NONE = 0xffffffffu;
constexpr uint32_t CLUSTER_MAX_LEAVES = 16384;
constexpr uint32_t CLUSTER_Q = 20;  // a leaf pair's score is in units of 2^-20
struct ClusterMerge {
    uint32_t slot_a, slot_b, node_a, node_b;  // left child (the smaller node index) and right child
    unsigned long long score;                 // S(left, right) before the merge
};
void launch_cluster_scores(const uint32_t *d_shared, const unsigned long long *d_pop, uint32_t r0, uint32_t n_r, uint32_t n_c, uint64_t nbits,
                           unsigned long long *d_S, uint64_t pitch, hipStream_t st);
void launch_cluster_nearest(const unsigned long long *d_S, uint64_t pitch, const uint2 *d_meta, uint32_t n_slots, uint32_t *d_best, hipStream_t st);
void launch_cluster_mutual(const uint32_t *d_slot_of, uint32_t n_nodes, const uint32_t *d_best, const uint2 *d_meta, uint32_t *d_flag, hipStream_t st);
void launch_cluster_list(const uint32_t *d_slot_of, uint32_t n_nodes, const uint32_t *d_best, const uint2 *d_meta, const uint32_t *d_flag,
                         const unsigned long long *d_pos, const unsigned long long *d_S, uint64_t pitch, ClusterMerge *d_list, uint32_t list_cap,
                         hipStream_t st);
void launch_cluster_merge(unsigned long long *d_S, uint64_t pitch, uint2 *d_meta, uint32_t *d_slot_of, uint32_t n_slots, const ClusterMerge *d_list,
                          uint32_t n_merges, uint32_t first_node, hipStream_t st);
// pfq_text_parse (pfq_text.hip): plain FASTA / FASTQ text in device memory parsed into the CSR the classifier takes.  d_text is
// 16-byte aligned and holds 16 bytes beyond len rounded up to 16; len < 2^31.
//   launch_text_count: d_blk_cnt[b] = newlines of text[b * tile, (b + 1) * tile), b < ceil(len / tile); tile: a power of two from
//     TEXT_TILE_MIN.  The caller scans them (launch_scan_u32) and reads the total back: the considered lines are the newlines,
//     plus an unterminated last run with PFQ_TEXT_FINAL.
//   launch_text_lines: line_start [n_lines + 1]: line i is text[line_start[i], line_start[i + 1] - 1).
//   launch_text_roles: line_len[i] = the trimmed length of a sequence line, 0 of any other; FASTQ: *first_bad (set to n_lines / 4
//     by the caller) = the first whole record that is not plain; FASTA: d_is_header[i].  The caller scans line_len into dst and,
//     FASTA, d_is_header into rec_idx; launch_text_rec_lines then lists the header lines in rec_line.
//   launch_text_finish: result[TEXT_RES_*] by the rules of pfq.h; d_csr_off[j], j <= records taken; d_rec_begin likewise unless
//     NULL; the sequence lines of the records taken copied to d_csr_seq.  FASTA: line 0 must be a header.
constexpr uint32_t TEXT_TILE_MIN = 256, TEXT_TILE_DEFAULT = 8192;
constexpr uint32_t PFQ_TEXT_STOP_END = 0, PFQ_TEXT_STOP_LIMIT = 1, PFQ_TEXT_STOP_MORE = 2, PFQ_TEXT_STOP_SLOW = 3;  // = PFQ_TEXT_* of pfq.h
enum TextResult { TEXT_RES_RECORDS = 0, TEXT_RES_CONSUMED = 1, TEXT_RES_BASES = 2, TEXT_RES_STOP = 3, TEXT_RES_LINES = 4, TEXT_RES_N = 8 };
struct TextArgs {
    const uint8_t *text;
    uint32_t len, n_lines;
    uint64_t limit;
    int fastq, final;
    const uint32_t *line_start;            // [n_lines + 1]
    uint32_t *line_len;                    // [n_lines]
    const unsigned long long *dst;         // [n_lines + 1] scan of line_len
    uint32_t *first_bad;                   // FASTQ
    const unsigned long long *rec_idx;     // FASTA: [n_lines + 1] scan of the header flags
    const uint32_t *rec_line;              // FASTA: [headers]
    unsigned long long *result;            // [TEXT_RES_N]
};
void launch_text_count(const uint8_t *d_text, uint32_t len, uint32_t tile, uint32_t *d_blk_cnt, hipStream_t st);
void launch_text_lines(const uint8_t *d_text, uint32_t len, uint32_t tile, const unsigned long long *d_blk_off, uint32_t *d_line_start, uint32_t n_lines,
                       bool unterminated, hipStream_t st);
void launch_text_roles(const TextArgs &a, uint32_t *d_is_header, hipStream_t st);
void launch_text_rec_lines(const uint32_t *d_is_header, const unsigned long long *d_rec_idx, uint32_t n_lines, uint32_t *d_rec_line, hipStream_t st);
void launch_text_finish(const TextArgs &a, uint8_t *d_csr_seq, uint64_t *d_csr_off, uint64_t *d_rec_begin, hipStream_t st);
// pfq_text_format (pfq_emit.hip): the POS / NEG records of the block pfq_text_parse took, formatted by the rules of pfq.h "text
// output" from what the parse left (text, line_start, FASTA: rec_line), the CSR it gathered (seq, seq_off) and the final hit
// rows of pfq_text_query (row_off, row_leaves).  Records head .. head + n_whole * block - 1 are the whole result blocks.
//   launch_fmt_ids: id_beg, id_len, hash [n] (the hash cut to hash_bits bits); then state [n_whole] (zeroed by the caller) = 1
//     for a block in which two records have the same id, exactly: equal hashes are settled by the bytes.
//   launch_fmt_sizes: len[0] / len[1] [n] = the bytes a record adds to the POS / NEG stream, 0 for a record that is not emitted;
//     res[FMT_RES_POS_RECORDS / NEG_RECORDS] += the records emitted, res[FMT_RES_ERR] |= 1 for a record of 2^32 bytes or more;
//     long_rows: rows of more than 64 names may occur (res[FMT_RES_LONG] counts long_list [n]).  res is zeroed by the caller,
//     who scans len[s] into dst[s] (launch_scan_u32).
//   launch_fmt_bounds: bounds[2 i + s] = dst[s][head + i * block], i <= n_whole; bounds[2 (n_whole + 1) + s] = dst[s][n].
//   launch_fmt_emit: the records written to out[s] + dst[s][r].  names: the leaves' tax_ids back to back, name_off [n_leaves + 1].
// grid: 0, or a cap on every grid (PFQ_FMT_GRID).  n = 0: nothing runs.
constexpr uint32_t FMT_POS = 1, FMT_NEG = 2, FMT_BLOCK_MAX = 8192;  // = PFQ_FMT_* of pfq.h
enum FmtResult { FMT_RES_LONG = 0, FMT_RES_ERR = 1, FMT_RES_POS_RECORDS = 2, FMT_RES_NEG_RECORDS = 3, FMT_RES_N = 4 };
struct FmtArgs {
    const uint8_t *text;
    const uint32_t *line_start, *rec_line;
    int fastq;
    uint32_t n, head, block, n_whole, flags, hash_bits, grid;
    const uint8_t *seq;
    const uint64_t *seq_off;                 // [n + 1]
    const unsigned long long *row_off;       // [n + 1]
    const uint32_t *row_leaves;
    const uint8_t *names;
    const uint32_t *name_off;
    uint32_t *id_beg, *id_len;               // [n]
    uint64_t *hash;                          // [n]
    uint32_t *state;                         // [n_whole]
    uint32_t *len[2];                        // [n]
    const unsigned long long *dst[2];        // [n + 1]
    uint32_t *long_list;                     // [n]
    unsigned long long *res;                 // [FMT_RES_N]
    unsigned long long *bounds;              // [2 (n_whole + 2)]
    uint8_t *out[2];
};
void launch_fmt_ids(const FmtArgs &a, hipStream_t st);
void launch_fmt_sizes(const FmtArgs &a, bool long_rows, hipStream_t st);
void launch_fmt_bounds(const FmtArgs &a, hipStream_t st);
void launch_fmt_emit(const FmtArgs &a, hipStream_t st);
// pfq_prep_reads (pfq_prep.hip): reads trimmed and filtered by the rules of pfq.h "read preprocessing", the kept intervals
// gathered into the CSR the classifier takes.  seq and qual are 16-byte aligned and hold 16 bytes beyond off[n_reads]; qual
// shares off with seq (nullptr: no read has qualities), has_qual is a byte per read (nullptr: all have).
//   launch_prep_trim: begin, len, reason [n_reads] before the mate rule; totals[PREP_TOT_ERR] |= 1 if a read has 2^32 bases or
//     more (or the offsets descend).  Three builds of one kernel share the reads by length: groups of 16 lanes up to
//     PREP_SHORT_MAX bases, a wave up to PREP_WAVE_MAX, a block beyond; a group takes 16 bytes a lane and piece.
//   launch_prep_mark: the mate rule (paired: reads 2i, 2i + 1; n_reads even), keep and klen [n_reads], totals[0 .. PREP_TOT_ERR)
//     += the call's (zeroed by the caller).  The caller scans keep into kpos and klen into koff (launch_scan_u32).
//   launch_prep_gather: kept [n_kept], csr_off [n_kept + 1], the kept intervals copied to out (16 bytes beyond the kept bases).
// n_reads = 0: nothing runs.
constexpr uint32_t PREP_SHORT = 1, PREP_N = 2, PREP_COMPLEXITY = 3, PREP_MATE = 4;  // = PFQ_PREP_* of pfq.h
constexpr uint32_t PREP_SHORT_MAX = 512, PREP_WAVE_MAX = 4096;
constexpr uint32_t PREP_GRID = 1024;  // blocks of every kernel: reads of one grid trip / 256 (the 16-lane trim build: / its block size)
enum PrepTotal { PREP_TOT_REASON = 0 /* .. 4 */, PREP_TOT_BASES_IN = 5, PREP_TOT_BASES_KEPT = 6, PREP_TOT_TRIMMED = 7, PREP_TOT_ERR = 8, PREP_TOT_N = 9 };
struct PrepArgs {
    const uint8_t *seq, *qual;
    const uint64_t *off;                     // [n_reads + 1]
    const uint8_t *has_qual;
    uint64_t n_reads;
    uint32_t trim_quality, trim_window, poly_x, min_length, max_n, min_complexity, paired;
    uint32_t *begin, *len, *reason;          // [n_reads]
    uint32_t *keep, *klen;                   // [n_reads]
    unsigned long long *totals;              // [PREP_TOT_N]
    const unsigned long long *kpos, *koff;   // [n_reads + 1] scans of keep and klen
    uint32_t *kept;                          // [n_kept]
    uint64_t *csr_off;                       // [n_kept + 1]
    uint8_t *out;
    const uint32_t *cut;                     // [n_reads] of launch_prep_adapter or launch_prep_overlap: read r is s[0, min(L, cut[r])); nullptr: neither ran
};
// The adapter step (pfq_adapt.hip; the rule is pfq.h "adapters"): cut and which [n_reads], totals[0 .. ADAPT_TOT_N) += the
// call's (zeroed by the caller).  An adapter is 4 words of 2-bit codes, base i at bits 2i, 2i + 1 of word i / 16, code
// (letter >> 1) & 3; set 1 at [0, ADAPT_MAX), set 2 (odd reads of a paired call, if it has any) at [ADAPT_MAX, 2 ADAPT_MAX).
constexpr uint32_t ADAPT_MAX = 8, ADAPT_LEN_MAX = 64;  // = PFQ_ADAPTER_* of pfq.h
enum AdaptTotal { ADAPT_TOT_FOUND = 0, ADAPT_TOT_BASES = 1, ADAPT_TOT_WHICH = 2 /* .. 17 */, ADAPT_TOT_N = 18 };
struct AdaptSet {
    uint32_t n[2], min_overlap, max_error_percent;
    uint8_t len[2 * ADAPT_MAX];
    uint32_t code[2 * ADAPT_MAX][4];
};
struct AdaptArgs {
    const uint8_t *seq;                      // as PrepArgs
    const uint64_t *off;
    uint64_t n_reads;
    uint32_t paired;
    uint32_t *cut;                           // [n_reads]
    uint8_t *which;                          // [n_reads]
    unsigned long long *totals;              // [ADAPT_TOT_N]
    AdaptSet set;
};
// The mate overlap step (pfq_overlap.hip; the rule is pfq.h "mate overlap"): a wave per fragment (reads 2f, 2f + 1).  insert and
// mismatches [n_reads / 2]; cut [n_reads] = min(ocut, adapter_cut[r]) (adapter_cut nullptr: ocut), which launch_prep_trim then
// takes as PrepArgs::cut; totals[0 .. OVL_TOT_N + OVL_HIST) += the call's (zeroed by the caller), the histogram of the inserts
// behind the counters.  A fragment with a mate of more than OVL_LEN_MAX bases is skipped: no insert, cut = the adapter's or L.
constexpr uint32_t OVL_LEN_MAX = 512, OVL_HIST = 2 * OVL_LEN_MAX + 1;  // = PFQ_OVERLAP_LEN_MAX, PFQ_OVERLAP_INSERT_MAX + 1 of pfq.h
enum OvlTotal { OVL_TOT_ANALYSED = 0, OVL_TOT_SKIPPED = 1, OVL_TOT_FOUND = 2, OVL_TOT_THROUGH = 3, OVL_TOT_READS = 4, OVL_TOT_BASES = 5, OVL_TOT_N = 6 };
enum CorTotal { COR_TOT_FRAGMENTS = 0, COR_TOT_BASES = 1 /* , 2: per mate */, COR_TOT_UNRESOLVED = 3, COR_TOT_NO_QUALITY = 4, COR_TOT_N = 5 };
struct CorPatch {                            // = pfq_prep_patch of pfq.h
    uint32_t read, pos;
    uint8_t base, qual, old_base, old_qual;
};
struct OverlapArgs {
    const uint8_t *seq;                      // as PrepArgs
    const uint64_t *off;
    uint64_t n_reads;                        // even
    uint32_t min_overlap, max_error_percent;
    const uint32_t *adapter_cut;             // [n_reads] of launch_prep_adapter, or nullptr
    uint32_t *insert, *mismatches;           // [n_reads / 2]
    uint32_t *cut;                           // [n_reads]
    unsigned long long *totals;              // [OVL_TOT_N + OVL_HIST]
    // mate correction (the rule is pfq.h "mate correction"): cor_high == 0: off, and nothing below is looked at
    uint32_t cor_high, cor_low;
    uint8_t *cor_seq, *cor_qual;             // seq and the qualities that share off with it, writable; cor_qual nullptr: no read has qualities
    const uint8_t *has_qual;                 // [n_reads] or nullptr: every read has
    unsigned long long *cor_totals;          // [COR_TOT_N], zeroed by the caller
    uint32_t *cor_count;                     // [n_reads / 2] zeroed by the caller: the overlap kernel leaves the reads as they are and writes
                                             // the corrections of a fragment that has any, for launch_prep_patches; nullptr: it corrects in place
    const unsigned long long *cor_at;        // [n_reads / 2 + 1] the exclusive scan of cor_count (launch_prep_patches)
    CorPatch *patches;                       // [cor_at[n_reads / 2]] (launch_prep_patches)
};
void launch_prep_adapter(const AdaptArgs &a, hipStream_t st);
// cor_high == 0: the kernel without the correction; else the build with it
void launch_prep_overlap(const OverlapArgs &a, hipStream_t st);
// behind launch_prep_overlap with cor_count and the scan of it: a wave per fragment with corrections writes its patches at
// cor_at[f], ascending by (read, pos), from the reads as they came, and then corrects them
void launch_prep_patches(const OverlapArgs &a, hipStream_t st);
void launch_prep_trim(const PrepArgs &a, hipStream_t st);
void launch_prep_mark(const PrepArgs &a, hipStream_t st);
void launch_prep_gather(const PrepArgs &a, hipStream_t st);
// pfq_prep_deplete (pfq_deplete.hip; the rule is pfq.h "depletion"): the verdict of the screen's classification of the prepared
// block, turned into the prep's keep flags.  The caller then scans keep and klen again and runs launch_prep_gather.
//   launch_deplete_pairs: hit[r] = 1 for every hit pair (r, leaf) of the screen's call on reads (hit zeroed by the caller).
//   launch_deplete_mark: a unit (pair_mode 0: kept read u = read kept[u] of the block; 1 either / 2 both: kept fragment u = reads
//     kept[2u], kept[2u + 1]) is removed iff its row on the screen is not empty — reads: hit[u] or allhit[u]; fragments: row u
//     of frag_off (nullptr: no row was built) or the all-hit bytes of its mates, as launch_lca_rows reads them.  The reads of a
//     removed unit get keep = klen = 0 and reason = PREP_DEPLETED; totals[0 .. DEPL_TOT_N) += the call's (zeroed by the caller).
constexpr uint32_t PREP_DEPLETED = 5;  // = PFQ_PREP_DEPLETED of pfq.h
enum DepleteTotal { DEPL_TOT_UNITS = 0, DEPL_TOT_READS = 1, DEPL_TOT_BASES = 2, DEPL_TOT_N = 3 };
struct DepleteArgs {
    const uint32_t *hit;                     // [n_units] (reads)
    const uint8_t *allhit;                   // [n_units] (reads), [2 n_units] (fragments): of the screen's call
    const unsigned long long *frag_off;      // [n_units + 1] (fragments): the screen's final CSR offsets, or nullptr
    int pair_mode;
    uint64_t n_units, n_reads;               // n_reads: of the block given to pfq_prep_reads
    const uint32_t *kept;                    // [n_units or 2 n_units]
    uint32_t *keep, *klen, *reason;          // [n_reads]
    unsigned long long *totals;              // [DEPL_TOT_N]
};
void launch_deplete_pairs(const uint2 *d_pairs, uint64_t n_pairs, uint64_t n_units, uint32_t *d_hit, hipStream_t st);
void launch_deplete_mark(const DepleteArgs &a, hipStream_t st);
void launch_debug_indices(const HashParams &hp, const uint8_t *d_seq, uint64_t len, uint64_t *d_out, hipStream_t st);
void launch_synth_genomes(uint8_t *d_out, uint64_t n_genomes, uint64_t genome_len, uint64_t seed_base, hipStream_t st);
void launch_synth_reads(uint8_t *d_out, uint64_t first, uint64_t n_reads, uint64_t read_len, const uint8_t *d_genomes,
                        uint64_t genome_len, uint64_t n_genomes, uint64_t seed, hipStream_t st);
// pfq_text_inflate (pfq_inflate.hip): the members of a blocked gzip chunk inflated, one wave a member, a grid-stride loop over
// the members.  d_gz: the chunk, 16-byte aligned, allocated (not necessarily filled) up to a multiple of GZ_STAGE beyond its last
// payload byte; members: what the host's header walk found (nothing in them comes from the device's reading of the bytes);
// d_text: the texts back to back, text_begin + isize <= its size.  d_result [2 n_members]: per member its status
// (pfq_inflate::Status, never ST_CRC: the host compares) and the CRC-32 of the text it produced (0 unless the status is 0).
constexpr uint32_t GZ_STAGE = 2048;  // compressed bytes a wave stages into LDS at a time
struct GzMember {
    uint64_t pay_begin, text_begin;  // of the deflate payload in d_gz, of the text in d_text
    uint32_t pay_len, isize;
};
void launch_gz_inflate(const uint8_t *d_gz, const GzMember *d_members, uint64_t n_members, uint8_t *d_text, uint32_t *d_result, uint32_t blocks,
                       hipStream_t st);
// pfq_bgzf_deflate / pfq_text_format_gz (pfq_deflate.hip): text deflated into members of blocked gzip, one workgroup a member, a
// grid-stride loop over the members.  d_text: 16-byte aligned and allocated 16 bytes beyond the last member's text; members: the
// host's cutting (text_len <= BGZF_TOKENS).  d_tokens: BGZF_TOKENS words for every workgroup of the grid min(n_members, blocks);
// member m is written to d_slots + m * BGZF_SLOT and its bytes to d_sizes[m].  The caller scans the sizes (launch_scan_u32) into
// d_off, and launch_bgzf_gather moves the members to d_gz + d_off[m] (d_gz: 4-byte aligned).
constexpr uint32_t BGZF_SLOT = 65536, BGZF_TOKENS = 65280;
struct BgzfMember {
    uint64_t text_begin;  // in d_text
    uint32_t text_len, piece;
};
void launch_bgzf_deflate(const uint8_t *d_text, const BgzfMember *d_members, uint64_t n_members, uint32_t *d_tokens, uint8_t *d_slots, uint32_t *d_sizes,
                         uint32_t blocks, hipStream_t st);
void launch_bgzf_gather(const uint8_t *d_slots, const unsigned long long *d_off, uint64_t n_members, uint8_t *d_gz, hipStream_t st);

}  // namespace pfq
