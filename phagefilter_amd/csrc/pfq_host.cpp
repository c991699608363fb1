// pfq_host.cpp — host side of libpfq: the tree model (BloomTree/BloomNode, bloom_tree.rs:29-61), the
// tree.bin / .bf reader and writer (bincode 1.3.3 + bitvec 1.0.1 layouts, bloom_tree.rs:339-386,
// bloom_filter.rs:153-205), the HBM layout builder and the query orchestration behind the C ABI of include/pfq.h.
// Compiled with hipcc together with pfq_kernels.hip.  No CPU compute path exists here: all filter work is
// done by the kernels and every entry point fails with PFQ_ERR_DEVICE when no gfx950 device is usable.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is loaded when pfq_trees_allreduce_counts first needs it
#include <dlfcn.h>

#include <algorithm>
#include <thread>
#include <mutex>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <unordered_set>
#include <vector>

#include "../../include/pfq.h"
#include "pfq_inflate_core.h"
#include "pfq_kernels.h"
#include "pfq_taxonomy.h"

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(PFQ_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                                            std::to_string(__LINE__) + ")");                                 \
    } while (0)
#define PFQ_TRY(expr)              \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != PFQ_OK) return rc_; \
    } while (0)

struct Node {
    int32_t left = -1, right = -1, parent = -1;
    std::string bf_path;  // relative file name, joined to the db dir like cache.rs:62
    bool has_tax = false;
    std::string tax_id;
    uint64_t mapped_reads = 0;
    uint64_t base_reads = 0;  // mapped_reads as stored / last reset, imported or reduced (see pfq_tree::d_counts_base)
    uint32_t filter = 0;  // row of d_bits
    uint32_t depth = 0;
    bool is_leaf() const { return left < 0 && right < 0; }  // bloom_tree.rs:416-418
};

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t ensure(size_t want) {
        if (want <= n) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, want * sizeof(T));
        if (e == hipSuccess) n = want;
        return e;
    }
    size_t bytes() const { return n * sizeof(T); }
};
// The page-locked host counterpart.  A buffer that grows takes a quarter more than asked plus 4 KiB and drops its contents;
// what it held before (pointers handed to a caller) stays valid until then.
template <typename T>
struct HostBuf {
    T *p = nullptr;
    size_t cap = 0;  // bytes
    ~HostBuf() { if (p) (void)hipHostFree(p); }
    hipError_t ensure(size_t want) {
        const size_t bytes = want * sizeof(T), grown = bytes + bytes / 4 + 4096;
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc((void **)&p, grown, hipHostMallocDefault);
        if (e == hipSuccess) cap = grown;
        return e;
    }
};
// One HIP event, made by the first ensure() and destroyed with its owner.  ensure() of an event that exists does nothing, so a
// set-up that failed part of the way is completed by the next call that runs it.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept {
        std::swap(e, o.e);
        return *this;
    }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t ensure(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};
static_assert(!std::is_copy_constructible<Event>::value && std::is_nothrow_move_constructible<Event>::value,
              "an event has one owner; std::vector<Event> moves it");
// A stream of the library's own, likewise.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t ensure(unsigned flags) { return s ? hipSuccess : hipStreamCreateWithFlags(&s, flags); }
    operator hipStream_t() const { return s; }
};
// N timing events round the N - 1 stages of a call.  valid: the last call that marks them has recorded all of them and has
// been waited for, so read() may ask for the intervals.
template <int N>
struct StageTimes {
    Event ev[N];
    bool valid = false;
    hipError_t ensure() {
        for (Event &e : ev)
            if (hipError_t r = e.ensure(); r != hipSuccess) return r;
        return hipSuccess;
    }
    hipError_t mark(int i, hipStream_t st) { return hipEventRecord(ev[i], st); }
    hipError_t read(double *ms) const {
        for (int i = 0; i + 1 < N; ++i) {
            float f = 0.0f;
            if (hipError_t r = hipEventElapsedTime(&f, ev[i], ev[i + 1]); r != hipSuccess) return r;
            ms[i] = f;
        }
        return hipSuccess;
    }
};
// Two alternating sets of buffers that one call fills while the kernels of another still read the other set.  free[s] is
// recorded behind the last reader of set s (used[s]: there has been one); cur is the set that holds the current block.  When
// cur moves is the call site's business: a set that is being filled becomes current only where its filling cannot fail any more.
struct TwoSets {
    Event free[2];
    bool used[2] = {false, false};
    int cur = 0;
    hipError_t ensure() {
        for (Event &e : free)
            if (hipError_t r = e.ensure(hipEventDisableTiming); r != hipSuccess) return r;
        return hipSuccess;
    }
    int other() const { return cur ^ 1; }
    hipError_t wait(int s) const { return used[s] ? hipEventSynchronize(free[s]) : hipSuccess; }  // the last reader of set s is done
    hipError_t read_by(int s, hipStream_t st) {  // what `st` holds so far reads set s
        const hipError_t r = hipEventRecord(free[s], st);
        if (r == hipSuccess) used[s] = true;
        return r;
    }
};

// Tuning / test knobs.  Never needed for correct results.  The environment is read ONCE, when a tree is
// created or opened; afterwards pfq_set_option changes a knob of that tree.  -1 / unset = the built-in choice.
struct Knobs {
    long long record_gb = -1, tile_gb = -1, tile_entries = -1, slice_kb = -1;
    long long verify_blocks = -1, verify_chunk = -1, verify_sub = -1, verify_threads = -1, bin_blocks = -1, test_blocks = -1;
    long long tile = -1, tile_counts = -1, no_tail_batch = -1, split_records = -1, bin_narrow = -1, bin_wide = -1, bin_debug = -1, block = -1, batch_emit = -1;
    long long coarse = -1, coarse_cols = -1, coarse_probes = -1, group_log2 = -1, screen_recs = -1, coarse_min_leaves = -1, greedy_host = -1;
    long long pair_slots = -1, guard_slots = -1, miss_words = -1, kmiss_bytes = -1, hit_slots = -1;  // tests: capacities below the built-in ones
    long long abund_slots = -1, abund_blocks = -1, abund_lds = -1;  // PFQ_WANT_ABUNDANCE: cap on the log's leaf entries; grid and LDS use of the EM step
    long long cover_p = -1, cover_blocks = -1;  // PFQ_WANT_COVERAGE: registers per leaf = 2^cover_p (4..16, unset: 12); grid of the sketch kernel
    long long frame_piece = -1;                 // pfq_query_frames: k-mer positions per piece of the refinement (a positive multiple of 64)
    long long sim_slices = -1, sim_naive = -1, sim_time = -1;  // pfq_tree_similarity: slices of the filter words (0 / unset: built-in); 1: the one-block-per-pair kernel; 1: time the kernel
    long long cluster_time = -1;                // pfq_tree_recluster: 1: time the stages with HIP events (pfq_debug_last_recluster)
    long long text_tile = -1;                   // pfq_text_parse: bytes of text a block scans (a power of two, 256 .. the built-in 8192)
    long long sweep_lds = -1;                   // PFQ_WANT_SWEEP: 0: count `pass` with global atomics although its bins fit the block's LDS
    long long tile_lists = -1;                  // 0: no position slots, k_tile_test loads every tile dense (unset: slots for every sparse column)
    long long tile_stream = -1;                 // 0: the generic k_tile_test<0> even where every column has slots (unset: the slots-only build there)
    long long screen_kmers = -1;                // k-mers a read of the dense screen at threshold 1: 0 / unset chosen per tree from its leaves' fill, 2 wherever rows have <= 32 words, 4 always
    long long entry_pack = -1;                  // packed tile entries at threshold 1: 0 never, 1 / unset chosen per call from its read lengths, 2 always
    long long pair_ahead = -1;                  // reservations of 32 pair slots a batched emission of k_classify asks for beyond what its pass needs: 0 .. 16, unset: 8
    long long classify_blocks = -1;             // tests: a cap on the grid of the classify launches (a wave then screens several groups of a small input)
    long long fmt_grid = -1, fmt_hash_bits = -1, fmt_time = -1;  // pfq_text_format: a cap on every grid; bits of the id hash that are kept (1 .. 64); 1: time the stages with HIP events
    long long inflate_blocks = -1;              // pfq_text_inflate: a cap on the grid of k_gz_inflate (1 .. 65535; unset: two workgroups a CU, what their LDS admits)
    long long deflate_blocks = -1;              // pfq_bgzf_deflate, pfq_text_format_gz: a cap on the grid of k_bgzf_deflate (1 .. 65535; unset: one workgroup a CU)
};
struct KnobName {
    const char *name;
    long long Knobs::*field;
};
const KnobName KNOBS[] = {
    {"PFQ_RECORD_GB", &Knobs::record_gb},       {"PFQ_TILE_GB", &Knobs::tile_gb},
    {"PFQ_TILE_ENTRIES", &Knobs::tile_entries}, {"PFQ_SLICE_KB", &Knobs::slice_kb},
    {"PFQ_VERIFY_BLOCKS", &Knobs::verify_blocks}, {"PFQ_VERIFY_CHUNK", &Knobs::verify_chunk},
    {"PFQ_VERIFY_SUB", &Knobs::verify_sub},     {"PFQ_VERIFY_THREADS", &Knobs::verify_threads},
    {"PFQ_BIN_BLOCKS", &Knobs::bin_blocks},     {"PFQ_TEST_BLOCKS", &Knobs::test_blocks},
    {"PFQ_TILE", &Knobs::tile},                 {"PFQ_TILE_COUNTS", &Knobs::tile_counts},
    {"PFQ_NO_TAIL_BATCH", &Knobs::no_tail_batch}, {"PFQ_BIN_NARROW", &Knobs::bin_narrow},
    {"PFQ_BIN_WIDE", &Knobs::bin_wide},         {"PFQ_SPLIT_RECORDS", &Knobs::split_records},
#ifdef PFQ_EXPERIMENTS  // (timing experiments with wrong results: not in the library as shipped)
    {"PFQ_BIN_DEBUG", &Knobs::bin_debug},
#endif
    {"PFQ_BLOCK", &Knobs::block},               {"PFQ_BATCH_EMIT", &Knobs::batch_emit},
    {"PFQ_COARSE", &Knobs::coarse},             {"PFQ_COARSE_COLS", &Knobs::coarse_cols},
    {"PFQ_COARSE_PROBES", &Knobs::coarse_probes}, {"PFQ_GROUP_LOG2", &Knobs::group_log2},
    {"PFQ_SCREEN_RECS", &Knobs::screen_recs},   {"PFQ_COARSE_MIN_LEAVES", &Knobs::coarse_min_leaves},
    {"PFQ_GREEDY_HOST", &Knobs::greedy_host},
    {"PFQ_PAIR_SLOTS", &Knobs::pair_slots},     {"PFQ_GUARD_SLOTS", &Knobs::guard_slots},
    {"PFQ_MISS_WORDS", &Knobs::miss_words},     {"PFQ_KMISS_BYTES", &Knobs::kmiss_bytes},
    {"PFQ_HIT_SLOTS", &Knobs::hit_slots},
    {"PFQ_ABUND_SLOTS", &Knobs::abund_slots},   {"PFQ_ABUND_BLOCKS", &Knobs::abund_blocks},
    {"PFQ_ABUND_LDS", &Knobs::abund_lds},
    {"PFQ_COVER_P", &Knobs::cover_p},           {"PFQ_COVER_BLOCKS", &Knobs::cover_blocks},
    {"PFQ_FRAME_PIECE", &Knobs::frame_piece},
    {"PFQ_SIM_SLICES", &Knobs::sim_slices},     {"PFQ_SIM_NAIVE", &Knobs::sim_naive},
    {"PFQ_SIM_TIME", &Knobs::sim_time},         {"PFQ_CLUSTER_TIME", &Knobs::cluster_time},
    {"PFQ_TEXT_TILE", &Knobs::text_tile},       {"PFQ_SWEEP_LDS", &Knobs::sweep_lds},
    {"PFQ_TILE_LISTS", &Knobs::tile_lists},     {"PFQ_TILE_STREAM", &Knobs::tile_stream},
    {"PFQ_ENTRY_PACK", &Knobs::entry_pack},     {"PFQ_SCREEN_KMERS", &Knobs::screen_kmers},
    {"PFQ_FMT_GRID", &Knobs::fmt_grid},         {"PFQ_FMT_HASH_BITS", &Knobs::fmt_hash_bits},
    {"PFQ_FMT_TIME", &Knobs::fmt_time},
    {"PFQ_PAIR_AHEAD", &Knobs::pair_ahead},     {"PFQ_CLASSIFY_BLOCKS", &Knobs::classify_blocks},
    {"PFQ_INFLATE_BLOCKS", &Knobs::inflate_blocks},
    {"PFQ_DEFLATE_BLOCKS", &Knobs::deflate_blocks},
};
bool set_knob(Knobs &k, const char *name, const char *value) {
    for (const KnobName &kn : KNOBS)
        if (!strcmp(kn.name, name)) {
            k.*(kn.field) = (value && *value) ? strtoll(value, nullptr, 10) : -1;
            return true;
        }
    return false;
}
Knobs knobs_from_env() {
    Knobs k;
    for (const KnobName &kn : KNOBS)
        if (const char *e = getenv(kn.name)) set_knob(k, kn.name, e);
    return k;
}

}  // namespace

namespace {
std::atomic<long> g_open_trees{0};
void release_communicators();  // (the kept RCCL communicators go when the last tree of the process is closed)
}  // namespace

// Slots of pfq_tree::d_cursors, 8 bytes each.  Every attempt of a query call clears all CUR_ALLOC of them; the kernels only
// ever receive pointers to single slots.
enum CursorSlot {
    CUR_HIT = 0,             // hit pairs written (may exceed the hit buffer: the call then runs again)
    CUR_PAIR = 1,            // deferred-pair slots reserved
    CUR_TILE_ENTRIES = 2,    // tile entries the plan asks for
    CUR_CHUNKS_FLAGGED = 3,  // lo: chunks, hi: flagged pairs
    CUR_LONG = 4,            // lo: reads of >= 256 k-mers queued by a classify launch (thresholds < 1)
    CUR_MISS_WORDS = 5,      // miss words handed out
    CUR_DIRTY = 6,           // pairs with a k-mer missing
    CUR_OPEN = 7,            // lo: open pairs after the tile passes (thresholds < 1)
    CUR_GUARD = 8,           // guard-pair slots reserved
    CUR_KMISS = 9,           // k-mer miss bytes handed out
    CUR_TAIL_SHAPES = 10,    // lo: tail shapes that served a pair (pfq::TAIL_SHAPE_*)
    CUR_TAIL_WORK = 11,      // lo: k_tail_records' work counter
    CUR_TILE_LIST = 12,      // k_tile_test<0>: tiles built from position slots
    CUR_TILE_DENSE = 13,     //                 tiles loaded dense
    CUR_N = 14,
    CUR_ALLOC = 16,          // slots allocated and cleared
};
static_assert(CUR_N <= CUR_ALLOC, "an attempt clears CUR_ALLOC slots");
static_assert(CUR_HIT == 0 && CUR_PAIR == 1, "read_hits reads slots 0 and 1 with one 16-byte copy");
static_assert(CUR_TAIL_WORK == CUR_TAIL_SHAPES + 1, "k_tail_records finds its work counter at shapes[2]");
static_assert(CUR_TILE_DENSE == CUR_TILE_LIST + 1, "k_tile_test finds its dense counter at tile_list_stats[1]");
// Slots of pfq_tree::h_pair_cursor, the pinned mirror a bucketed call leaves for the next call's sizing (HINT_N allocated).
enum HintSlot {
    HINT_PAIRS = 0,         // CUR_PAIR
    HINT_TILE_ENTRIES = 1,  // CUR_TILE_ENTRIES
    HINT_DIRTY = 2,         // CUR_DIRTY
    HINT_SORTED = 3,        // lo: pairs sorted (the pair cursor also counts partly used reservations)
    HINT_CANDIDATES = 4,    // ST_CANDIDATES
    HINT_PLAN = 5,          // not a hint: block mode reads CUR_TILE_ENTRIES back here after the plan
    HINT_N = 8,
};
static_assert(CUR_TILE_ENTRIES == CUR_PAIR + 1 && HINT_TILE_ENTRIES == HINT_PAIRS + 1, "one 16-byte copy fills both hints");

struct pfq_tree {
    pfq_tree() { ++g_open_trees; }
    pfq_tree(const pfq_tree &) = delete;
    ~pfq_tree() {
        if (--g_open_trees == 0) release_communicators();
    }
    int device = 0;
    Knobs knobs = knobs_from_env();
    // ---- model
    std::vector<Node> nodes;  // pre-order, root = 0
    int32_t root = -1;
    float false_pos_rate = 0.001f;
    uint32_t largest_expected_genome = 0;
    uint64_t kmer_size = 0, nbits = 0, seed1 = 0, seed2 = 0, n_words = 0;
    uint32_t num_hashes = 0;
    std::vector<std::string> filter_paths;
    std::unordered_set<std::string> path_set;  // filter_paths as a set, kept by pfq_tree_insert (a name's .bf must be new: a scan per insertion was 40 us at 2000 nodes)
    std::vector<uint8_t> edge_ok;  // per node: parent(v) ⊇ v verified
    bool superset_all = true;
    uint64_t shard_first_leaf = 0, tree_leaves = 0;  // subtree shards (pfq_tree_open_subtree)
    bool is_shard = false;
    // deferred pairs per read seen by recent calls (related genomes: a read passes several leaves): sizes the pair
    // buffer and the probe buckets of the next call.  The cursor of a call lands in pinned memory asynchronously.
    HostBuf<unsigned long long> h_pair_cursor;
    Event hint_ev;
    uint64_t hint_reads = 0, hint_entry_cap = 0, passes_hint = 1;
    double pairs_per_read = 1.0, hits_per_read = 1.0;
    double dirty_frac = 1.0;           // thresholds < 1: share of the last call's deferred pairs with a k-mer missing (1: unknown)
    bool hint_counts = false;
    uint32_t last_sub_log2 = 0;
    bool topology_dirty = false;       // nodes appended by pfq_tree_insert: renumber + verify before the next use
    uint64_t internal_counter = 0;     // names of internal nodes created by pfq_tree_insert
    size_t n_rows = 0, row_capacity = 0;  // filter rows in use / allocated in d_bits
    DevBuf<uint32_t> d_build;          // insert scratch: leaf row, union triple
    DevBuf<unsigned long long> d_dist; // insert scratch: the device walk's barrier lines (GREEDY_SYNC_*); the host walk's per-block partials
    // pfq_tree_insert walks the tree on the device (k_greedy_insert): its shape is mirrored there and the host's left / right /
    // root are brought up to date when they are next needed (finish_topology)
    DevBuf<pfq::TopoNode> d_topo;
    DevBuf<int> d_walk;                // [0] root (for the host), [1] error word, [2..3] the root as the walk's launches hand it on
    bool topo_on_device = false;       // d_topo / d_walk mirror the host's nodes
    bool topo_pending = false;         // insertions ran since the host last read the shape back
    DevBuf<uint8_t> d_gseq[4];         // genomes of the insertions in flight (ring)
    Event gseq_free[4], gseq_copied[4];
    HostBuf<uint8_t> h_gseq[4];        // page-locked staging of the same ring (the caller's buffer is free when pfq_tree_insert returns)
    uint32_t gseq_next = 0;
    int greedy_blocks = 0;
    uint32_t walk_seq = 0;             // launches of the device walk since d_walk was written (parity: where the root is read / left)
    // the first insertion that failed (a one-child node on the walk, the device walk's barrier): every call that needs the
    // topology returns it from then on — the ancestors have absorbed the leaf, the shape on the device is half made
    int insert_err = PFQ_OK;
    std::string insert_err_msg;

    pfq::HashParams hp{};
    // ---- device: node-major filters
    DevBuf<uint64_t> d_bits;
    // ---- device: layout of the current leaf set
    bool layout_valid = false;
    std::vector<int32_t> leaves;     // node ids, left-to-right
    std::vector<uint32_t> col_row;   // column -> filter row
    std::vector<uint32_t> guard_off, guard_col;
    uint32_t rw = 1, rw_log2 = 0, n_cols = 0;
    uint64_t leaf_cap = 0, guard_cap = 0;  // regions of the deferred-pair buffer
    uint32_t n_groups = 1;           // column groups of the sliced matrix (2^group_log2 columns each when there are several)
    uint32_t group_log2 = 11;
    uint64_t group_stride = 0;       // dwords per group: (n_words * 64 + 1) * rw
    // two-level frontier (trees of several leaf groups): coarse sliced matrix over an antichain of internal nodes
    bool coarse_valid = false;
    uint32_t coarse_cols = 0, coarse_rw = 0, coarse_rw_log2 = 0;
    double coarse_fill = 0.0;        // mean share of set bits of the coarse columns' filters
    DevBuf<uint32_t> d_Sc, d_cgrp, d_glists, d_glong;
    DevBuf<unsigned int> d_gcur;
    uint32_t last_coarse_cols = 0, last_coarse_probes = 0, last_leaf_groups = 0;
    DevBuf<uint32_t> d_S, d_col_row, d_guard_off, d_guard_col;
    // position slots of the sparse columns (pfq_tilelist.hip): made with the layout, gone with it; none is never an error
    DevBuf<uint32_t> d_tile_list_row, d_tile_lists;  // [n_cols] row of slots or TILE_LIST_NONE; [rows][tiles][TILE_LIST_CAP]
    uint32_t tile_list_cols = 0;     // columns with slots (0: d_tile_lists is not in use)
    void drop_tile_lists() {
        d_tile_list_row.release();
        d_tile_lists.release();
        tile_list_cols = 0;
    }
    DevBuf<uint32_t> d_owner, d_owner_sorted, d_gfail;  // trees with guard columns, bucketed path: leaf pair of every pair slot
    DevBuf<unsigned long long> d_counts;
    // what the counters held when the tree was opened (BloomNode::mapped_reads stored in tree.bin), last reset, imported or
    // reduced: the reductions over replicas / ranks add up counters - base, so that stored counts are not added once per replica
    DevBuf<unsigned long long> d_counts_base, d_counts_delta;
    // ---- query scratch
    DevBuf<unsigned long long> d_stats, d_cursors;  // d_cursors: one slot per CursorSlot
    unsigned int *cur_lo(CursorSlot s) const { return reinterpret_cast<unsigned int *>(d_cursors.p + s); }  // a slot's halves
    unsigned int *cur_hi(CursorSlot s) const { return cur_lo(s) + 1; }
    DevBuf<uint32_t> d_entries, d_pair_chunk, d_leaf_chunk0, d_flag_list;  // LDS-tile certificates
    DevBuf<pfq::ChunkDesc> d_chunks;
    DevBuf<unsigned int> d_gfill, d_binq;
    DevBuf<uint8_t> d_kmiss;
    DevBuf<uint8_t> d_kall;            // block mode with k-mer entries: per k-mer, "in no candidate leaf of the block"
    DevBuf<uint8_t> d_T, d_failb;      // block mode: byte-per-index tables of the blocks of 8 leaves; failure bytes per (pair, leaf)
    bool tables_valid = false;         // d_T matches the current leaf set
    double cand_per_read = 1.0;        // candidate leaves per read seen by recent calls (related genomes: several): chooses block mode
    bool have_cand_hint = false;       // cand_per_read describes this tree's workload (else a sample of the block is screened first)
    uint32_t last_block_mode = 0;
    DevBuf<uint32_t> d_round_k0, d_n_rounds, d_pair_kpos;  // thresholds < 1: LDS-tile passes with k-mer entries
    DevBuf<uint32_t> d_round_p0;       // threshold 1, packed entries: first pair of every round of every chunk (and d_n_rounds)
    DevBuf<uint8_t> d_round_fail;      //                              a failure byte per (chunk, round, pair of the round)
    bool last_entry_pack = false;      // the last call's passes wrote and read packed entries
    uint32_t last_n_tiles = 0;         // tiles per filter of the last call's passes (pfq_debug_tile_bucket)
    uint32_t last_tile_mode = 0, last_passes = 1;
    uint32_t last_sort = 0;            // kernel the last call sorted its pairs with (pfq::SORT_SLICED / SORT_PER_PAIR); 0: direct path
    bool last_tile_stream = false;     // the last call's passes ran the slots-only build of k_tile_test<0>
    uint32_t last_tile_bin = 0;        // build of k_tile_bin the last call launched (waves << 16 | bin capacity); 0: no pass
    DevBuf<uint2> d_hit_pairs, d_pairs, d_sorted;
    DevBuf<uint32_t> d_bucket, d_fail;  // bucket: cnt[n], off[n+1], cur[n]
    DevBuf<unsigned int> d_queue;
    DevBuf<uint8_t> d_allhit, d_seq, d_seq2;  // d_seq / d_seq2, d_off / d_off2: input buffers of pfq_query_batch, alternating
    DevBuf<uint64_t> d_off2;
    Stream copy_stream;                // made by ensure_copy_stream
    TwoSets in_sets;                   // d_seq / d_off and d_seq2 / d_off2 (stage_input)
    DevBuf<unsigned long long> d_miss_words;  // thresholds < 1: k-mer miss bits of every deferred pair
    DevBuf<uint32_t> d_miss_pos, d_bucket_w;  // first word per sorted pair; per-bucket word counts / offsets / cursors
    DevBuf<uint32_t> d_long;
    DevBuf<uint4> d_recs;  // probe records of the bucketed path (16 B per read byte)
    DevBuf<uint4> d_meta;  // resolved per-pair metadata for the record-driven verify
    DevBuf<uint64_t> d_off;
    DevBuf<unsigned long long> d_counts_snapshot;
    // the stream of the last query call, for comparison only: the caller may destroy it once it is synchronised, so what
    // waits for that call is last_done, recorded on it after the call's work
    hipStream_t last_stream = nullptr;
    bool have_last_stream = false;
    Event last_done;
    int force_path = -1;
    // ---- profiling (HIP events on the launch stream)
    std::vector<Event> prof_ev;  // PROF_EV events per recorded call
    size_t prof_cap = 0, prof_used = 0;
    std::vector<uint8_t> prof_bucketed;
    uint32_t last_path = 0, last_slices = 1;
    uint64_t last_n_reads = 0;
    // pfq_debug_last_capacity: the caps the last call gave the kernels, its first attempt's hit cursor, its attempts
    uint64_t last_pair_cap = 0, last_guard_cap = 0, last_miss_cap = 0, last_kmiss_cap = 0, last_hit_cap0 = 0, last_hit_cursor0 = 0;
    uint64_t last_nb = 0;  // buckets of the last bucketed call (0: direct path): d_bucket[2 * last_nb] = pairs sorted
    uint32_t last_attempts = 0;
    // ---- outputs (library-owned)
    std::vector<std::string> out_tax;
    std::vector<const char *> out_tax_ptr;
    std::vector<uint64_t> out_counts;
    // per-read hit lists of the last PFQ_WANT_HITS call: built on the device, copied into page-locked host memory
    DevBuf<uint32_t> d_hit_cnt, d_hit_leaves;
    DevBuf<unsigned long long> d_hit_sums, d_hit_off;
    HostBuf<uint64_t> h_hit_off;
    HostBuf<uint32_t> h_hit_leaves;
    // PFQ_WANT_SCORES: one score per entry of h_hit_leaves (pfq_last_hit_scores); valid only after a call that asked for them
    DevBuf<uint32_t> d_hit_scores;
    HostBuf<uint32_t> h_hit_scores;
    bool scores_valid = false;
    uint64_t scores_n = 0;
    // PFQ_PAIRED: the mates' increments land in d_pair_sink (never read); the fragment CSR is built into d_frag_off /
    // d_frag_leaves and its histogram goes into d_counts.  d_pair_long: fragments queued for a wave; d_pair_misc: [0] queued,
    // [1] all-leaf fragments left unlisted
    DevBuf<unsigned long long> d_pair_sink, d_frag_off, d_pair_misc;
    DevBuf<uint32_t> d_frag_leaves, d_pair_long;
    // PFQ_WANT_LCA: the clades (nodes reachable from the root, pre-order) and the device tables over the current leaf set are
    // built on first use and again after the layout changed (ensure_lca); the counters d_clade_here live as long as the tables
    bool lca_valid = false;
    std::vector<pfq_clade> clades;
    std::vector<std::string> clade_names;
    uint32_t top_clade = 0;                // LCA of all leaves
    DevBuf<uint32_t> d_leaf_clade, d_gap_min, d_lca, d_lca_long;
    DevBuf<unsigned long long> d_clade_here, d_lca_misc;
    DevBuf<uint2> d_lca_span;
    std::vector<uint64_t> out_here, out_below;
    // PFQ_WANT_ABUNDANCE: the log of the calls' rows.  Ambiguous rows live in device memory (row r = d_ab_entries[d_ab_start[r]
    // .. + d_ab_len[r])), rows of one leaf in d_ab_unique; the class counters and the numbers of rows and entries in use are
    // kept on the host: k_abund_count says what a call adds (d_ab_cur[2..]: five words read back per call) before anything is
    // appended, so the host makes exactly that much room or refuses the call (d_ab_cur[0..1] hands ab_rows / ab_entries to the
    // append kernel).  The buffers grow geometrically, with a copy (DevBuf::ensure drops the contents).
    DevBuf<unsigned long long> d_ab_start, d_ab_unique, d_ab_cur, d_ab_a, d_ab_b, d_ab_delta;
    DevBuf<uint32_t> d_ab_len, d_ab_entries;
    uint64_t ab_rows = 0, ab_entries = 0, ab_units = 0, ab_unhit = 0, ab_unique = 0, ab_all = 0;
    bool ab_incomplete = false;            // a call's rows did not fit: no estimate until the log is reset
    std::vector<uint64_t> out_mass, out_unique;
    // PFQ_WANT_COVERAGE: d_cov_regs u8[n_leaves << cov_p] (HyperLogLog registers, [leaf << cov_p | j]), d_cov_cnt
    // [2][n_leaves] (units, matched); made by the first flagged call, freed by cover_clear.  cov_units: units sketched.
    // cov_bits: the leaves' filter popcounts, computed once per topology (cov_bits_valid).
    DevBuf<uint8_t> d_cov_regs;
    DevBuf<unsigned long long> d_cov_cnt;
    uint32_t cov_p = 0;
    uint64_t cov_units = 0;
    bool cov_bits_valid = false;
    std::vector<uint64_t> cov_bits, out_cov_units, out_cov_matched;
    // The lean dense screen (QueryRun::plan): screen_E = sum over the leaves of (popcount / nbits)^4, made with cov_bits;
    // last_screen_kmers: k-mers a read the dense screen of the last call's deferring launch took (2: the lean build, 4, 0: none ran).
    double screen_E = 0.0;
    uint32_t last_screen_kmers = 0;
    uint32_t last_pair_ahead = 0;  // QueryArgs::pair_ahead of the last call's classify launches (pfq_pair_info); 0: none deferred
    std::vector<uint8_t> out_cov_regs;
    std::vector<double> out_cov_distinct, out_cov_genome;
    // pfq_query_frames: the frame table of the call (per sequence its first frame and the scan of the lone frames' deficits; per
    // frame its sequence, start and byte offset), the frames' bytes — the block the inner classification reads, d_fr_bytes
    // behind d_fr_foff — and what the post-stage makes of the frames' rows: per frame where its segments go, the segments,
    // their sequences, the queue of long runs, the refinement's pieces.  d_fr_cnt / d_fr_sums: input and scratch of the scans.
    DevBuf<uint32_t> d_fr_cnt, d_fr_def, d_fr_seq, d_fr_start, d_fr_segseq, d_fr_queue;
    DevBuf<unsigned long long> d_fr_seq0, d_fr_defoff, d_fr_sums, d_fr_segpos, d_fr_seqseg, d_fr_pieceoff, d_fr_misc;
    DevBuf<uint64_t> d_fr_foff;
    DevBuf<uint8_t> d_fr_bytes;
    DevBuf<pfq::Segment> d_fr_segs;
    DevBuf<pfq::FramePart> d_fr_parts;
    HostBuf<uint64_t> h_fr_off;
    HostBuf<pfq_segment> h_fr_segs;
    // pfq_tree_similarity: the last call's result (its device buffers live only during the call)
    std::vector<uint32_t> out_sim_shared;
    std::vector<uint64_t> out_sim_bits_a, out_sim_bits_b;
    std::vector<double> out_sim_kmers_a, out_sim_kmers_b, out_sim_shared_kmers, out_sim_jaccard;
    float sim_kernel_ms = 0.0f;            // pfq_debug_last_similarity: device time of the last call's intersection kernel, its slices
    uint32_t sim_slices = 0;
    // pfq_tree_recluster: the merge log of the tree the call made (pfq_tree_merges), until its topology changes; on the source
    // tree, what pfq_debug_last_recluster reports of the last call
    std::vector<pfq_merge> merges;
    uint32_t merge_rounds = 0;
    float cluster_ms[3] = {0.0f, 0.0f, 0.0f};
    uint64_t cluster_nn_bytes = 0;
    uint32_t cluster_rounds = 0;
    // pfq_text_parse: the text, what the parse kernels leave per tile and per line (scratch of one call: the call waits for its
    // kernels), and two alternating CSR sets — the classification of pfq_text_query reads set tx_slot while the next parse fills
    // the other.  tx_sets: set s is read by the classification; tx_parsed: behind the parse kernels.
    DevBuf<uint8_t> d_tx_text, d_tx_seq[2];
    DevBuf<uint64_t> d_tx_off[2], d_tx_rec_begin;
    DevBuf<uint32_t> d_tx_blk, d_tx_line, d_tx_len, d_tx_hdr, d_tx_rec_line, d_tx_bad;
    DevBuf<unsigned long long> d_tx_blk_off, d_tx_sums, d_tx_dst, d_tx_rec_idx, d_tx_res;
    HostBuf<unsigned long long> h_tx_res;  // page-locked: the result words, the newline count
    TwoSets tx_sets;
    Event tx_parsed;
    bool tx_have = false;
    uint64_t tx_records = 0, tx_bases = 0;
    std::vector<uint64_t> out_rec_begin;
    int tx_fastq = 0;
    uint64_t tx_len = 0;  // bytes of the text parsed last (pfq_text_read)
    // pfq_text_inflate: the compressed chunk, the members the host's header walk found, the texts back to back (what
    // pfq_text_parse_inflated copies behind the carry), per member its status and CRC; the walk's tables and the statuses as
    // the caller sees them.  gz_time: before the copy, behind it, behind the kernel.
    DevBuf<uint8_t> d_gz, d_gz_text;
    DevBuf<pfq::GzMember> d_gz_mem;
    DevBuf<uint32_t> d_gz_res;
    std::vector<uint64_t> gz_begin, gz_text_begin;
    std::vector<pfq::GzMember> gz_mem;
    std::vector<uint32_t> gz_res;
    std::vector<uint8_t> gz_status;
    bool gz_have = false;
    uint64_t gz_good_text = 0;
    StageTimes<3> gz_time;
    // pfq_bgzf_deflate / pfq_text_format_gz: the text of a host caller, the members as the host cut them, a slab of tokens for
    // every workgroup, a slot for every member and their sizes with the scan (scratch of one call: the call waits for its
    // kernels); per stream (0: pfq_bgzf_deflate and pos, 1: neg) the gathered members, their page-locked copy and the tables the
    // caller sees.  df_time: before the copy in, behind it, behind the kernel, behind the copy out.
    DevBuf<uint8_t> d_df_text, d_df_slots, d_df_gz[2];
    DevBuf<pfq::BgzfMember> d_df_mem;
    DevBuf<uint32_t> d_df_tokens, d_df_sizes;
    DevBuf<unsigned long long> d_df_off, d_df_sums;
    HostBuf<uint8_t> h_df_gz[2];
    HostBuf<unsigned long long> h_df_off;
    std::vector<pfq::BgzfMember> df_mem;
    std::vector<uint64_t> df_piece_begin[2], df_member_begin[2];
    StageTimes<4> df_time;
    // pfq_text_format: what the kernels leave per record (ids, hashes, lengths and their scans), the small words that go back to
    // the host in one copy (d_fm_small: FMT_RES_N result words | the streams' offsets at the block boundaries | the block states),
    // the leaves' names (uploaded when they differ from fm_names), the two streams and their page-locked copies, which only
    // grow.  fm_rows: the last query call was a successful pfq_text_query of the parsed block with PFQ_WANT_HITS and without
    // PFQ_PAIRED, so d_hit_off / d_hit_leaves hold its rows, of a tree of fm_rows_leaves leaves.
    DevBuf<uint32_t> d_fm_idb, d_fm_idl, d_fm_len[2], d_fm_long, d_fm_name_off;
    DevBuf<uint64_t> d_fm_hash;
    DevBuf<unsigned long long> d_fm_dst[2], d_fm_sums, d_fm_small;
    DevBuf<uint8_t> d_fm_names, d_fm_out[2];
    HostBuf<uint8_t> h_fm_out[2];
    HostBuf<unsigned long long> h_fm_small;
    std::vector<uint8_t> fm_names;
    std::vector<uint32_t> fm_name_off;
    std::vector<pfq_text_left> out_fm_left;
    bool fm_rows = false;
    uint64_t fm_rows_leaves = 0;
    StageTimes<4> fm_time;  // pfq_debug_last_format: ids + blocks, sizes + scans, emit
    // pfq_prep_reads: the block as the caller gave it and what the kernels leave per read (scratch of one call: the call waits
    // for its kernels), and two alternating CSR sets as above (pp_sets); pp_ready: behind the prep kernels.
    DevBuf<uint8_t> d_pp_in, d_pp_qual, d_pp_hq, d_pp_seq[2];
    DevBuf<uint64_t> d_pp_inoff, d_pp_off[2];
    DevBuf<uint32_t> d_pp_begin, d_pp_len, d_pp_reason, d_pp_keep, d_pp_klen, d_pp_kept;
    DevBuf<unsigned long long> d_pp_kpos, d_pp_koff, d_pp_sums, d_pp_tot;
    HostBuf<unsigned long long> h_pp_tot;  // page-locked: the totals, then the kept reads
    TwoSets pp_sets;
    Event pp_ready;
    StageTimes<4> pp_time;  // pfq_debug_last_prep: round trim + mark, the scans, offsets + gather
    bool pp_have = false, pp_paired = false;
    uint64_t pp_kept = 0, pp_bases = 0;
    std::vector<uint32_t> out_pp_begin, out_pp_len, out_pp_reason, out_pp_kept;
    // pfq_prep_deplete on this tree's prepared block: pp_reads / pp_want_reads of the prep that made it (d_pp_keep, d_pp_klen,
    // d_pp_kept, d_pp_reason, d_pp_begin and the raw block stay on the device until the next prep, and the call compacts from
    // them), the per-unit hit flags of a screen's call on reads, the totals and their page-locked copy (behind them the kept
    // reads and bases of the new scans), the host copies of kept and reason after the last call (dp_have: there has been one
    // since the prep; out_pp_* stay the prep's).
    uint64_t pp_reads = 0;
    bool pp_want_reads = false, dp_have = false;
    DevBuf<uint32_t> d_dp_hit;
    DevBuf<unsigned long long> d_dp_tot;
    HostBuf<unsigned long long> h_dp_tot;
    StageTimes<3> dp_time;  // pfq_debug_last_deplete: the screen's classification, mark + scans + compaction
    std::vector<uint32_t> out_dp_kept, out_dp_reason;
    // pfq_tree_set_adapters: the sets as the kernel takes them (ad_on: any is set) and what the adapter step of the last
    // pfq_prep_reads left: cut and which per read (scratch of one call, as d_pp_begin), the totals (h_pp_tot behind the kept
    // reads), the host copies of a PFQ_PREP_WANT_READS call.  ad_last: the last prep ran with adapters.
    bool ad_on = false, ad_last = false, ad_last_reads = false;
    pfq::AdaptSet ad_set{};
    DevBuf<uint32_t> d_pp_cut;
    DevBuf<uint8_t> d_pp_which;
    DevBuf<unsigned long long> d_pp_atot;
    StageTimes<2> ad_time;  // pfq_debug_last_adapters
    pfq_prep_adapters ad_out{};
    std::vector<uint32_t> out_pp_cut;
    std::vector<uint8_t> out_pp_which;
    // pfq_tree_set_mate_overlap (ov_on) and what the overlap step of the last paired pfq_prep_reads left: insert and mismatches
    // per fragment, the merged cut per read that the trim kernel takes (d_pp_ecut = min(adapter cut, ocut)), the totals and
    // the histogram (h_pp_tot behind the adapter totals).  ov_last: the last prep ran the step.
    bool ov_on = false, ov_last = false, ov_last_reads = false;
    uint32_t ov_min_overlap = 0, ov_max_error_percent = 0;
    DevBuf<uint32_t> d_pp_oins, d_pp_omm, d_pp_ecut;
    DevBuf<unsigned long long> d_pp_otot;
    StageTimes<2> ov_time;  // pfq_debug_last_overlap
    pfq_prep_overlap ov_out{};
    std::vector<uint64_t> out_ov_hist;
    std::vector<uint32_t> out_ov_insert, out_ov_mm;
    // pfq_tree_set_mate_correct (mc_high > 0: on) and what the correction of the last paired pfq_prep_reads left: the totals
    // (h_pp_tot behind the overlap's, then the length of the patch list) and, for a PFQ_PREP_WANT_READS call only, the
    // corrections per fragment, their scan and the patch list.  mc_last: the last prep ran the correction.
    uint32_t mc_high = 0, mc_low = 0;
    bool mc_last = false, mc_last_reads = false;
    DevBuf<unsigned long long> d_pp_ctot, d_pp_cat;
    DevBuf<uint32_t> d_pp_ccnt;
    DevBuf<pfq::CorPatch> d_pp_patch;
    StageTimes<2> mc_time;  // pfq_debug_last_corrections: the scan and the patch kernel
    pfq_prep_corrections mc_out{};
    std::vector<pfq_prep_patch> out_mc_patch;
    std::vector<uint32_t> out_lca;
    bool lca_last = false;                 // the last query call set PFQ_WANT_LCA
    uint64_t lca_units = 0;
    // PFQ_WANT_TAXA: the user's taxonomy over the current leaves (pfq_tree_set_taxonomy): the node table, its device tables
    // (pfq_kernels.h TaxTables) and the counters d_tax_here / d_tax_any [n_nodes], d_tax_misc [TAX_MISC_N: units with a hit,
    // all-leaf units — applied at read-out] and d_tax_cur [1: the queue cursor of a call's long rows].  Dropped by tax_clear.
    bool tax_set = false;
    pfq_taxonomy::NodeTable tax;
    uint32_t tax_hot[pfq::TAX_HOT] = {PFQ_NO_CLADE, PFQ_NO_CLADE, PFQ_NO_CLADE, PFQ_NO_CLADE};
    DevBuf<uint32_t> d_tax_rank, d_tax_leaf_node, d_tax_parent, d_tax_first, d_tax_gap_min, d_tax_node, d_tax_long;
    DevBuf<unsigned long long> d_tax_here, d_tax_any, d_tax_misc, d_tax_cur;
    std::vector<uint64_t> out_tax_here, out_tax_below, out_tax_any;
    std::vector<uint32_t> out_tax_node;
    bool taxa_last = false;                // the last query call set PFQ_WANT_TAXA
    uint64_t taxa_units = 0;
    // PFQ_ROWS_BEST: the last flagged call's best rows, a second CSR in device memory (d_best_off [best_units + 1],
    // d_best_leaves) that the taxonomy, the abundance log and the coverage sketch read in place of the call's own; d_best_cnt /
    // d_best_sums: input and scratch of the scan, d_best_long / d_best_cur: the queue of rows a wave takes and its cursor.
    // Scratch like d_lca_span / d_tax_long: reused call after call, copied to the host only by pfq_last_best_rows.
    DevBuf<uint32_t> d_best_cnt, d_best_long, d_best_leaves;
    DevBuf<unsigned long long> d_best_sums, d_best_off, d_best_cur;
    std::vector<uint64_t> out_best_off;
    std::vector<uint32_t> out_best_leaves;
    bool best_last = false;                // the last query call set PFQ_ROWS_BEST
    bool best_built = false;               // ... and built rows (else: every best row is empty)
    uint64_t best_units = 0;
    // PFQ_WANT_SWEEP: the list (pfq_tree_set_sweep) and the counters of the flagged calls, one buffer of u64 sized for sw_nl
    // leaves and T thresholds: pass [(T + 1) * sw_nl] | uniq [T * sw_nl] | tops [T + 1] (sweep_ensure makes it, zeroed;
    // pfq_tree_prune and pfq_tree_insert drop it, and the next use makes it anew for the new leaves).  sw_units: units counted
    // (those of calls that built no row are counted here only: they belong to tops[0], which no read-out uses).  d_sw_long /
    // d_sw_cur: a call's queue of long rows.
    std::vector<float> sw_thr;
    DevBuf<unsigned long long> d_sw_state, d_sw_cur;
    DevBuf<uint32_t> d_sw_long;
    size_t sw_nl = 0;
    uint64_t sw_units = 0;
    std::vector<uint64_t> out_sw_leaf_units, out_sw_leaf_unique, out_sw_sums;
    std::vector<float> out_sw_thr;
};

namespace {

// ------------------------------------------------------------------------------------------------------------
// bincode cursor
// ------------------------------------------------------------------------------------------------------------
struct Cur {
    const uint8_t *b;
    size_t n, p = 0;
    bool ok = true;
    const uint8_t *take(size_t k) {
        if (!ok || k > n - p) {
            ok = false;
            return nullptr;
        }
        const uint8_t *r = b + p;
        p += k;
        return r;
    }
    uint8_t u8() { auto q = take(1); return q ? *q : 0; }
    uint32_t u32() { auto q = take(4); uint32_t v = 0; if (q) memcpy(&v, q, 4); return v; }
    uint64_t u64() { auto q = take(8); uint64_t v = 0; if (q) memcpy(&v, q, 8); return v; }
    float f32() { auto q = take(4); float v = 0; if (q) memcpy(&v, q, 4); return v; }
    std::string str() {
        uint64_t len = u64();
        if (!ok || len > n - p) { ok = false; return {}; }
        auto q = take((size_t)len);
        return q ? std::string((const char *)q, (size_t)len) : std::string();
    }
};

bool read_file(const std::string &path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(sz > 0 ? (size_t)sz : 0);
    size_t got = out.empty() ? 0 : fread(out.data(), 1, out.size(), f);
    fclose(f);
    return got == out.size();
}

// BloomNode, pre-order (bloom_tree.rs:50-61): left, right, bloom_filter_path, tax_id, mapped_reads
int parse_node(Cur &c, pfq_tree &t, int32_t parent, uint32_t depth, int32_t &out_idx) {
    if (depth > 100000) return fail(PFQ_ERR_FORMAT, "tree.bin: nesting too deep");
    int32_t v = (int32_t)t.nodes.size();
    t.nodes.emplace_back();
    t.nodes[v].parent = parent;
    t.nodes[v].depth = depth;
    for (int side = 0; side < 2; ++side) {
        uint8_t tag = c.u8();
        if (!c.ok || tag > 1) return fail(PFQ_ERR_FORMAT, "tree.bin: bad Option tag in BloomNode");
        int32_t child = -1;
        if (tag == 1) PFQ_TRY(parse_node(c, t, v, depth + 1, child));
        (side == 0 ? t.nodes[v].left : t.nodes[v].right) = child;
    }
    t.nodes[v].bf_path = c.str();
    uint8_t tag = c.u8();
    if (!c.ok || tag > 1) return fail(PFQ_ERR_FORMAT, "tree.bin: bad Option tag for tax_id");
    if (tag == 1) {
        t.nodes[v].has_tax = true;
        t.nodes[v].tax_id = c.str();
    }
    t.nodes[v].mapped_reads = c.u64();
    t.nodes[v].base_reads = t.nodes[v].mapped_reads;
    if (!c.ok) return fail(PFQ_ERR_FORMAT, "tree.bin: truncated BloomNode");
    out_idx = v;
    return PFQ_OK;
}

uint64_t pow2_64_mod(uint64_t d) {  // 2^64 mod d
    uint64_t r = (~0ull) % d;       // (2^64 - 1) mod d
    return (r + 1 == d) ? 0 : r + 1;
}

int setup_hash_params(pfq_tree &t) {
    if (t.kmer_size < 1 || t.kmer_size > pfq::KMAX)
        return fail(PFQ_ERR_UNSUPPORTED, "kmer_size " + std::to_string(t.kmer_size) + " outside the device path's 1.." +
                                              std::to_string(pfq::KMAX));
    if (t.nbits < 1 || t.nbits >= (1ull << 32))
        return fail(PFQ_ERR_UNSUPPORTED, "filter size " + std::to_string(t.nbits) + " bits outside 1..2^32-1");
    if (t.num_hashes < 1) return fail(PFQ_ERR_FORMAT, "num_hashes == 0");
    t.n_words = (t.nbits + 63) / 64;
    t.hp.k = (uint32_t)t.kmer_size;
    t.hp.num_hashes = t.num_hashes;
    t.hp.nbits = t.nbits;
    t.hp.bar_m = (~0ull) / t.nbits;
    t.hp.w64 = pow2_64_mod(t.nbits);
    // FxHasher after write_usize(seed) (hasher.rs:16-18) and the length prefix of <[u8] as Hash>::hash
    // (times K once more: the kernels finish with rotl(a + hash_bytes * K), see pfq_device.h)
    t.hp.a1 = (t.seed1 * pfq::FX_K + t.kmer_size) * pfq::FX_K * pfq::FX_K;
    t.hp.a2 = (t.seed2 * pfq::FX_K + t.kmer_size) * pfq::FX_K * pfq::FX_K;
    return PFQ_OK;
}

int use_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(PFQ_ERR_DEVICE, "no HIP device available (libpfq has no CPU fallback)");
    if (device < 0 || device >= n) return fail(PFQ_ERR_ARG, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    return PFQ_OK;
}

void relink(pfq_tree &t) {  // parent/depth after topology edits
    if (t.root < 0) return;
    std::vector<int32_t> st{t.root};
    t.nodes[t.root].parent = -1;
    t.nodes[t.root].depth = 0;
    while (!st.empty()) {
        int32_t v = st.back();
        st.pop_back();
        for (int32_t c : {t.nodes[v].left, t.nodes[v].right})
            if (c >= 0) {
                t.nodes[c].parent = v;
                t.nodes[c].depth = t.nodes[v].depth + 1;
                st.push_back(c);
            }
    }
}

std::vector<int32_t> leaves_dfs(const pfq_tree &t) {  // get_leaf_counts order, query.rs:197-218
    std::vector<int32_t> out;
    if (t.root < 0) return out;
    std::vector<int32_t> st{t.root};
    while (!st.empty()) {
        int32_t v = st.back();
        st.pop_back();
        const Node &nd = t.nodes[v];
        if (nd.is_leaf()) out.push_back(v);
        else {
            if (nd.right >= 0) st.push_back(nd.right);
            if (nd.left >= 0) st.push_back(nd.left);
        }
    }
    return out;
}

// Fold the device counters back into BloomNode::mapped_reads (before the leaf set changes / on read-out).
int sync_counts_to_nodes(pfq_tree &t) {
    if (!t.layout_valid || t.leaves.empty()) return PFQ_OK;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> h(t.leaves.size());
    HIP_TRY(hipMemcpy(h.data(), t.d_counts.p, h.size() * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i) t.nodes[t.leaves[i]].mapped_reads = h[i];
    HIP_TRY(hipMemcpy(h.data(), t.d_counts_base.p, h.size() * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i) t.nodes[t.leaves[i]].base_reads = h[i];
    return PFQ_OK;
}

// parent ⊇ child on every edge of the full tree, on the device.
int verify_supersets(pfq_tree &t) {
    t.edge_ok.assign(t.nodes.size(), 1);
    t.superset_all = true;
    std::vector<uint32_t> edges;
    std::vector<int32_t> edge_node;
    std::vector<uint8_t> reach(t.nodes.size(), 0);
    if (t.root >= 0) {
        std::vector<int32_t> st{t.root};
        while (!st.empty()) {
            int32_t v = st.back();
            st.pop_back();
            reach[v] = 1;
            if (t.nodes[v].left >= 0) st.push_back(t.nodes[v].left);
            if (t.nodes[v].right >= 0) st.push_back(t.nodes[v].right);
        }
    }
    for (size_t v = 0; v < t.nodes.size(); ++v)
        if (reach[v] && t.nodes[v].parent >= 0 && t.nodes[t.nodes[v].parent].filter != t.nodes[v].filter) {
            edges.push_back(t.nodes[t.nodes[v].parent].filter);
            edges.push_back(t.nodes[v].filter);
            edge_node.push_back((int32_t)v);
        }
    if (edge_node.empty()) return PFQ_OK;
    DevBuf<uint32_t> d_edges, d_fail;
    HIP_TRY(d_edges.ensure(edges.size()));
    HIP_TRY(d_fail.ensure(edge_node.size()));
    HIP_TRY(hipMemcpy(d_edges.p, edges.data(), edges.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_fail.p, 0, edge_node.size() * 4));
    // blockIdx.y is limited to 65535
    for (size_t e0 = 0; e0 < edge_node.size(); e0 += 32768) {
        uint32_t ne = (uint32_t)std::min<size_t>(32768, edge_node.size() - e0);
        pfq::launch_superset(t.d_bits.p, t.n_words, d_edges.p + 2 * e0, ne, d_fail.p + e0, nullptr);
    }
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> h(edge_node.size());
    HIP_TRY(hipMemcpy(h.data(), d_fail.p, h.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i)
        if (h[i]) {
            t.edge_ok[edge_node[i]] = 0;
            t.superset_all = false;
        }
    return PFQ_OK;
}

// Build the sliced matrix for the current leaf set.
uint64_t needed_bits_f32(float rate, uint32_t items) {  // bloom_filter.rs:354-357, f32 arithmetic
    const float ln2 = 0.693147180559945309417232121458176568f;
    const float ln22 = ln2 * ln2;
    const float v = roundf((float)items * (logf(1.0f / rate) / ln22));
    return v <= 0 ? 0 : (uint64_t)v;
}
uint32_t optimal_num_hashes_f32(uint64_t bits, uint32_t items) {  // bloom_filter.rs:342-350
    const float ln2 = 0.693147180559945309417232121458176568f;
    const float v = roundf((float)bits / (float)items * ln2);
    const uint32_t h = v <= 0 ? 0 : (uint32_t)v;
    return std::min<uint32_t>(std::max<uint32_t>(h, 2), 200);
}

// A failed insertion is sticky (include/pfq.h): the first one is recorded, and it is what every later call that needs the
// topology returns.
const char *const ONE_CHILD_MSG = "Node with only one child encountered - should not happen. (bloom_tree.rs:209)";
int insertion_failed(pfq_tree &t, int code, const std::string &msg) {
    if (t.insert_err == PFQ_OK) {
        t.insert_err = code;
        t.insert_err_msg = msg;
    }
    return fail(t.insert_err, t.insert_err_msg);
}
int insertion_error(const pfq_tree &t) { return t.insert_err == PFQ_OK ? PFQ_OK : fail(t.insert_err, t.insert_err_msg); }

// Nodes in pre-order again (root = 0) after pfq_tree_insert appended some; parents, depths and the ⊇ flags follow.
// The shape the insertions on the device left (k_greedy_insert): children of every node, the root.
int sync_topology(pfq_tree &t) {
    PFQ_TRY(insertion_error(t));
    if (!t.topo_pending) return PFQ_OK;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<pfq::TopoNode> h(t.nodes.size());
    int st[2] = {-1, 0};
    HIP_TRY(hipMemcpy(h.data(), t.d_topo.p, h.size() * sizeof(pfq::TopoNode), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, t.d_walk.p, sizeof st, hipMemcpyDeviceToHost));
    // (topo_pending stays set on failure: the shape on the device is never taken over)
    if (st[1] == 1) return insertion_failed(t, PFQ_ERR_FORMAT, ONE_CHILD_MSG);
    if (st[1] != 0) return insertion_failed(t, PFQ_ERR_DEVICE, "the insertion kernel's grid barrier timed out");
    t.topo_pending = false;
    for (size_t v = 0; v < h.size(); ++v) {
        t.nodes[v].left = h[v].left;
        t.nodes[v].right = h[v].right;
    }
    t.root = st[0];
    return PFQ_OK;
}

int finish_topology(pfq_tree &t) {
    PFQ_TRY(sync_topology(t));
    if (!t.topology_dirty) return PFQ_OK;
    std::vector<int32_t> order, new_of(t.nodes.size(), -1);
    if (t.root >= 0) {
        std::vector<int32_t> st{t.root};
        while (!st.empty()) {
            const int32_t v = st.back();
            st.pop_back();
            new_of[v] = (int32_t)order.size();
            order.push_back(v);
            if (t.nodes[v].right >= 0) st.push_back(t.nodes[v].right);
            if (t.nodes[v].left >= 0) st.push_back(t.nodes[v].left);
        }
    }
    std::vector<Node> nn;
    nn.reserve(order.size());
    for (int32_t v : order) {
        Node nd = std::move(t.nodes[v]);
        if (nd.left >= 0) nd.left = new_of[nd.left];
        if (nd.right >= 0) nd.right = new_of[nd.right];
        nn.push_back(std::move(nd));
    }
    t.nodes.swap(nn);
    t.root = t.nodes.empty() ? -1 : 0;
    relink(t);
    t.topology_dirty = false;
    t.topo_on_device = false;  // (the nodes were renumbered)
    PFQ_TRY(verify_supersets(t));
    return PFQ_OK;
}

// Room for `rows` filter rows in d_bits, keeping the rows in use.
int reserve_rows(pfq_tree &t, size_t rows) {
    if (rows <= t.row_capacity) return PFQ_OK;
    size_t cap = std::max<size_t>(rows, t.row_capacity + t.row_capacity / 2 + 2);
    HIP_TRY(hipDeviceSynchronize());  // (insertions in flight on the tree's own streams still write the old rows)
    uint64_t *p = nullptr;
    HIP_TRY(hipMalloc(&p, cap * t.n_words * 8));
    if (t.n_rows) HIP_TRY(hipMemcpy(p, t.d_bits.p, t.n_rows * t.n_words * 8, hipMemcpyDeviceToDevice));
    t.d_bits.release();
    t.d_bits.p = p;
    t.d_bits.n = cap * t.n_words;
    t.row_capacity = cap;
    return PFQ_OK;
}

// An allocation that may fail without failing the call: the caller then takes the next exact path.
template <typename T>
bool soft_ensure(DevBuf<T> &b, size_t want) {
    if (b.ensure(want) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

// The coarse level of the two-level frontier (pfq::CoarseArgs): an antichain of nodes that covers every leaf, as close to
// the leaves as `max_cols` columns allow (the node with the most leaves below it is split until the budget is spent), in
// left-to-right order; column c = the filter of node anti[c] — the filter the reference tests at that node (cache.rs:56-62
// keys filters by path, so nodes that share a file share the row).  Leaves: t.leaves must be current.
void pick_antichain(const pfq_tree &t, uint32_t max_cols, std::vector<int32_t> &anti, std::vector<uint32_t> &first, std::vector<uint32_t> &count) {
    const size_t nn = t.nodes.size();
    first.assign(nn, 0xffffffffu);
    count.assign(nn, 0);
    for (size_t i = 0; i < t.leaves.size(); ++i) {
        first[t.leaves[i]] = (uint32_t)i;
        count[t.leaves[i]] = 1;
    }
    {   // leaves below every node, first leaf (post-order without recursion)
        std::vector<std::pair<int32_t, int>> st{{t.root, 0}};
        while (!st.empty()) {
            auto &top = st.back();
            const Node &nd = t.nodes[top.first];
            if (top.second == 0) {
                top.second = 1;
                if (nd.left >= 0) st.push_back({nd.left, 0});
                continue;
            }
            if (top.second == 1) {
                top.second = 2;
                if (nd.right >= 0) st.push_back({nd.right, 0});
                continue;
            }
            const int32_t v = top.first;
            st.pop_back();
            for (int32_t c : {t.nodes[v].left, t.nodes[v].right})
                if (c >= 0) {
                    count[v] += count[c];
                    first[v] = std::min(first[v], first[c]);
                }
        }
    }
    auto less = [&](int32_t x, int32_t y) { return count[x] < count[y] || (count[x] == count[y] && x > y); };
    std::vector<int32_t> heap{t.root};
    while (true) {
        const int32_t v = heap.front();
        const Node &nd = t.nodes[v];
        if (nd.is_leaf()) break;  // the largest node is a leaf: every node of the antichain is
        const int kids = (nd.left >= 0) + (nd.right >= 0);
        if (heap.size() + kids - 1 > max_cols) break;
        std::pop_heap(heap.begin(), heap.end(), less);
        heap.pop_back();
        for (int32_t c : {nd.left, nd.right})
            if (c >= 0) {
                heap.push_back(c);
                std::push_heap(heap.begin(), heap.end(), less);
            }
    }
    std::sort(heap.begin(), heap.end(), [&](int32_t x, int32_t y) { return first[x] < first[y]; });
    anti.swap(heap);
}

// Plans the coarse level of the current leaf set: the antichain (1024 columns — one 128-byte line per row — when its filters
// are empty enough, else 2048) and how full its filters are.  n_cols == 0: no coarse level pays (the screens cannot drop a
// column whose filter has nearly every bit set); the frontier then runs flat, every leaf group on every read.
struct CoarsePlan {
    uint32_t n_cols = 0;
    std::vector<uint32_t> rows, cgrp;
    double fill = 0;
};
int plan_coarse(pfq_tree &t, CoarsePlan &plan) {
    plan.n_cols = 0;
    std::vector<uint32_t> budgets;
    if (t.knobs.coarse_cols > 0) budgets.push_back((uint32_t)std::min<long long>(2048, std::max<long long>(2, t.knobs.coarse_cols)));
    else budgets = {1024u, 2048u};
    for (size_t bi = 0; bi < budgets.size(); ++bi) {
        std::vector<int32_t> anti;
        std::vector<uint32_t> first, count;
        pick_antichain(t, budgets[bi], anti, first, count);
        const uint32_t C = (uint32_t)anti.size();
        if (C < 2) return PFQ_OK;
        std::vector<uint32_t> rows(C), cgrp(C);
        for (uint32_t c = 0; c < C; ++c) {
            rows[c] = t.nodes[anti[c]].filter;
            const uint32_t lo = first[anti[c]] >> t.group_log2, hi = (first[anti[c]] + count[anti[c]] - 1) >> t.group_log2;
            cgrp[c] = lo | (hi << 16);
        }
        DevBuf<uint32_t> d_rows;
        DevBuf<unsigned long long> d_pop;
        HIP_TRY(d_rows.ensure(C));
        HIP_TRY(d_pop.ensure(C));
        HIP_TRY(hipMemcpy(d_rows.p, rows.data(), C * 4, hipMemcpyHostToDevice));
        pfq::launch_row_popcount(t.d_bits.p, t.n_words, d_rows.p, C, d_pop.p, nullptr);
        HIP_TRY(hipGetLastError());
        std::vector<unsigned long long> pop(C);
        HIP_TRY(hipMemcpy(pop.data(), d_pop.p, C * 8, hipMemcpyDeviceToHost));
        double fill = 0;
        for (unsigned long long v : pop) fill += (double)v / (double)t.nbits;
        fill /= C;
        if (fill > 0.62 && bi + 1 < budgets.size()) continue;   // try the finer antichain
        if (fill > 0.80 && t.knobs.coarse <= 0) return PFQ_OK;  // too full to prune anything (PFQ_COARSE=1: build it anyway)
        plan.n_cols = C;
        plan.rows.swap(rows);
        plan.cgrp.swap(cgrp);
        plan.fill = fill;
        return PFQ_OK;
    }
    return PFQ_OK;
}
int build_coarse(pfq_tree &t, const CoarsePlan &plan) {
    const uint32_t C = plan.n_cols;
    uint32_t rwc = 16, rwc_log2 = 4;  // (the dense counting screen takes rows of 16, 32 or 64 words)
    while (rwc * 32 < C) {
        rwc <<= 1;
        ++rwc_log2;
    }
    const uint64_t sc_words = ((uint64_t)t.n_words * 64 + 1) * rwc;
    DevBuf<uint32_t> d_rows;
    if (!(soft_ensure(t.d_Sc, sc_words) && soft_ensure(t.d_cgrp, C) && soft_ensure(t.d_gcur, 2 * pfq::MAX_LEAF_GROUPS) && soft_ensure(d_rows, C)))
        return PFQ_OK;  // (no room: flat frontier)
    HIP_TRY(hipMemcpy(d_rows.p, plan.rows.data(), C * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.d_cgrp.p, plan.cgrp.data(), C * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(t.d_Sc.p, 0, sc_words * 4, nullptr));
    HIP_TRY(hipMemsetAsync(t.d_Sc.p + sc_words - rwc, 0xff, rwc * 4, nullptr));
    pfq::launch_transpose(t.d_bits.p, t.n_words, d_rows.p, C, t.d_Sc.p, rwc, sc_words, 11, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    t.coarse_cols = C;
    t.coarse_rw = rwc;
    t.coarse_rw_log2 = rwc_log2;
    t.coarse_fill = plan.fill;
    t.coarse_valid = true;
    return PFQ_OK;
}

// Position slots for k_tile_test<0>: every column whose filter has at most TILE_LIST_CAP set bits in each 2^TILE_LOG2-bit tile
// gets a row of slots.  Two launches and the read-back of one count per column; whatever goes wrong with memory here leaves
// the tree without slots (every tile is then loaded dense), never with an error.
int build_tile_lists(pfq_tree &t) {
    t.drop_tile_lists();
    const uint64_t n_tiles = (t.n_words * 64 + (1ull << pfq::TILE_LOG2) - 1) >> pfq::TILE_LOG2;
    if (t.knobs.tile_lists == 0 || t.n_cols == 0 || n_tiles == 0 || n_tiles >= 256) return PFQ_OK;  // (256 tiles and more: no tile mode)
    auto give_up = [&]() {
        (void)hipGetLastError();
        t.drop_tile_lists();
        return PFQ_OK;
    };
    DevBuf<uint32_t> d_max, d_cols;
    if (d_max.ensure(t.n_cols) != hipSuccess || t.d_tile_list_row.ensure(t.n_cols) != hipSuccess) return give_up();
    HIP_TRY(hipMemsetAsync(d_max.p, 0, (size_t)t.n_cols * 4, nullptr));
    pfq::launch_tile_list_count(t.d_bits.p, t.n_words, t.d_col_row.p, t.n_cols, (uint32_t)n_tiles, d_max.p, nullptr);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> col_max(t.n_cols), row(t.n_cols, pfq::TILE_LIST_NONE), cols;
    HIP_TRY(hipMemcpy(col_max.data(), d_max.p, (size_t)t.n_cols * 4, hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < t.n_cols; ++c)
        if (col_max[c] <= pfq::TILE_LIST_CAP) {
            row[c] = (uint32_t)cols.size();
            cols.push_back(c);
        }
    if (cols.empty()) return give_up();
    if (d_cols.ensure(cols.size()) != hipSuccess || t.d_tile_lists.ensure(cols.size() * n_tiles * pfq::TILE_LIST_CAP) != hipSuccess) return give_up();
    HIP_TRY(hipMemcpy(d_cols.p, cols.data(), cols.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.d_tile_list_row.p, row.data(), row.size() * 4, hipMemcpyHostToDevice));
    pfq::launch_tile_list_fill(t.d_bits.p, t.n_words, t.d_col_row.p, d_cols.p, (uint32_t)cols.size(), (uint32_t)n_tiles, t.d_tile_lists.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());  // (d_cols goes out of scope)
    t.tile_list_cols = (uint32_t)cols.size();
    return PFQ_OK;
}

int build_layout(pfq_tree &t) {
    PFQ_TRY(insertion_error(t));
    if (t.layout_valid) return PFQ_OK;
    t.drop_tile_lists();
    PFQ_TRY(finish_topology(t));
    t.leaves = leaves_dfs(t);
    const size_t nl = t.leaves.size();
    for (int32_t v : t.leaves)
        if (!t.nodes[v].has_tax)
            return fail(PFQ_ERR_FORMAT, "leaf node without tax_id (reference: unwrap panic, query.rs:146)");
    t.col_row.clear();
    t.guard_off.assign(nl + 1, 0);
    t.guard_col.clear();
    std::map<uint32_t, uint32_t> guard_column_of_row;  // filter row -> guard column
    std::vector<uint32_t> guard_rows;
    for (size_t i = 0; i < nl; ++i) {
        t.col_row.push_back(t.nodes[t.leaves[i]].filter);
        bool ok = true;
        for (int32_t v = t.leaves[i]; t.nodes[v].parent >= 0; v = t.nodes[v].parent) {
            ok = ok && t.edge_ok[v];
            if (!ok) {
                uint32_t row = t.nodes[t.nodes[v].parent].filter;
                if (row == t.nodes[t.leaves[i]].filter) continue;  // same filter as the leaf itself
                auto it = guard_column_of_row.find(row);
                uint32_t col;
                if (it == guard_column_of_row.end()) {
                    col = (uint32_t)(nl + guard_rows.size());
                    guard_column_of_row[row] = col;
                    guard_rows.push_back(row);
                } else col = it->second;
                if (std::find(t.guard_col.begin() + t.guard_off[i], t.guard_col.end(), col) == t.guard_col.end())
                    t.guard_col.push_back(col);
            }
        }
        t.guard_off[i + 1] = (uint32_t)t.guard_col.size();
    }
    for (uint32_t r : guard_rows) t.col_row.push_back(r);
    t.n_cols = (uint32_t)t.col_row.size();
    uint32_t need_words = std::max<uint32_t>(1, (t.n_cols + 31) / 32);
    // a wave holds one row of up to 64 dwords (2048 columns) across its lanes; wider trees are cut into column groups,
    // each with a sliced matrix of its own, and the frontier kernels run once per group — on the reads the coarse level
    // lists for the group when the tree has one (two-level frontier: groups of 1024 columns, one 128-byte line per row)
    t.coarse_valid = false;
    t.coarse_cols = 0;
    const size_t coarse_min = t.knobs.coarse_min_leaves >= 1024 ? (size_t)t.knobs.coarse_min_leaves : 2048;
    bool want_coarse = nl > coarse_min && t.knobs.coarse != 0;
    t.group_log2 = 11;
    CoarsePlan plan;
    if (want_coarse) {
        t.group_log2 = (t.knobs.group_log2 == 10 || t.knobs.group_log2 == 11) ? (uint32_t)t.knobs.group_log2 : 10u;
        if (((nl - 1) >> t.group_log2) + 1 > pfq::MAX_LEAF_GROUPS) t.group_log2 = 11;
        if (((nl - 1) >> t.group_log2) + 1 > pfq::MAX_LEAF_GROUPS) want_coarse = false;  // (flat frontier: every group sees every read)
        if (want_coarse) PFQ_TRY(plan_coarse(t, plan));
        if (plan.n_cols == 0) {
            want_coarse = false;
            t.group_log2 = 11;
        }
    }
    if (!want_coarse) t.d_Sc.release();
    const uint32_t group_cols = 1u << t.group_log2;
    t.rw = 4;  // at least 16-byte rows: the dense pre-screen gathers rows with dwordx4 loads
    t.rw_log2 = 2;
    while (t.rw < need_words && t.rw < group_cols / 32) {
        t.rw <<= 1;
        ++t.rw_log2;
    }
    t.n_groups = std::max<uint32_t>(1, (t.n_cols + group_cols - 1) / group_cols);
    t.group_stride = ((uint64_t)t.n_words * 64 + 1) * t.rw;  // + the all-ones row of the group
    if (nl == 0) {
        t.layout_valid = true;
        t.tables_valid = false;
        return PFQ_OK;
    }
    const size_t s_words = (size_t)t.group_stride * t.n_groups;
    if (t.d_S.ensure(s_words) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PFQ_ERR_DEVICE, "not enough device memory for the sliced matrix of " + std::to_string(t.n_cols) +
                                        " leaf+guard columns (" + std::to_string(s_words * 4 >> 20) + " MiB)");
    }
    HIP_TRY(t.d_col_row.ensure(t.col_row.size()));
    HIP_TRY(t.d_guard_off.ensure(t.guard_off.size() + t.n_cols));  // guard lists are indexed by column; pad for guard columns
    HIP_TRY(t.d_guard_col.ensure(std::max<size_t>(1, t.guard_col.size())));
    HIP_TRY(t.d_counts.ensure(nl));
    HIP_TRY(hipMemcpy(t.d_col_row.p, t.col_row.data(), t.col_row.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.d_guard_off.p, t.guard_off.data(), t.guard_off.size() * 4, hipMemcpyHostToDevice));
    if (!t.guard_col.empty())
        HIP_TRY(hipMemcpy(t.d_guard_col.p, t.guard_col.data(), t.guard_col.size() * 4, hipMemcpyHostToDevice));
    std::vector<unsigned long long> h(nl);
    for (size_t i = 0; i < nl; ++i) h[i] = t.nodes[t.leaves[i]].mapped_reads;
    HIP_TRY(hipMemcpy(t.d_counts.p, h.data(), nl * 8, hipMemcpyHostToDevice));
    HIP_TRY(t.d_counts_base.ensure(nl));
    HIP_TRY(t.d_counts_delta.ensure(nl));
    for (size_t i = 0; i < nl; ++i) h[i] = t.nodes[t.leaves[i]].base_reads;
    HIP_TRY(hipMemcpy(t.d_counts_base.p, h.data(), nl * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(t.d_S.p, 0, s_words * 4, nullptr));
    for (uint32_t g = 0; g < t.n_groups; ++g)
        HIP_TRY(hipMemsetAsync(t.d_S.p + (g + 1) * t.group_stride - t.rw, 0xff, t.rw * 4, nullptr));
    pfq::launch_transpose(t.d_bits.p, t.n_words, t.d_col_row.p, t.n_cols, t.d_S.p, t.rw, t.group_stride, t.group_log2, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (want_coarse) PFQ_TRY(build_coarse(t, plan));
    PFQ_TRY(build_tile_lists(t));
    t.have_cand_hint = false;
    t.tables_valid = false;
    t.layout_valid = true;
    return PFQ_OK;
}

// PFQ_WANT_LCA: the clade table of the tree as it is and the device tables over its leaf columns (pfq_kernels.h), built on
// first use and again after pfq_tree_insert / pfq_tree_prune; the clade counters start at zero with them.
int ensure_lca(pfq_tree &t) {
    if (t.is_shard)
        return fail(PFQ_ERR_UNSUPPORTED, "PFQ_WANT_LCA on a subtree shard: a shard holds only its own subtree and ancestor chain, not the "
                                         "other shards' topology, so its clades are not the whole tree's");
    PFQ_TRY(build_layout(t));
    if (t.lca_valid) return PFQ_OK;
    t.clades.clear();
    t.clade_names.clear();
    const size_t nl = t.leaves.size();
    std::vector<uint32_t> leaf_clade(nl, 0), gap(nl ? nl - 1 : 0, 0);
    if (t.root >= 0) {
        // pre-order, left before right; a two-child node is the LCA of the last leaf of its left subtree and the first leaf
        // of its right one, which are adjacent columns: it owns the gap before its right child's first leaf
        struct Frame { int32_t node; uint32_t clade; int stage; };
        std::vector<Frame> st;
        uint32_t next_leaf = 0;
        auto enter = [&](int32_t v, uint32_t parent, uint32_t depth) {
            const uint32_t c = (uint32_t)t.clades.size();
            t.clades.push_back(pfq_clade{parent, depth, next_leaf, 0, nullptr});
            const Node &nd = t.nodes[v];
            std::string name = nd.tax_id;
            if (!nd.has_tax) {
                const size_t slash = nd.bf_path.find_last_of('/');
                name = slash == std::string::npos ? nd.bf_path : nd.bf_path.substr(slash + 1);
                if (name.size() > 3 && name.compare(name.size() - 3, 3, ".bf") == 0) name.resize(name.size() - 3);
            }
            t.clade_names.push_back(std::move(name));
            if (nd.is_leaf()) leaf_clade[next_leaf++] = c;
            st.push_back(Frame{v, c, 0});
        };
        enter(t.root, PFQ_NO_CLADE, 0);
        while (!st.empty()) {
            Frame &f = st.back();
            const Node &nd = t.nodes[f.node];
            const uint32_t c = f.clade, depth = t.clades[c].depth;
            if (f.stage == 0) {
                f.stage = 1;
                if (nd.left >= 0) {
                    enter(nd.left, c, depth + 1);
                    continue;
                }
            }
            if (f.stage == 1) {
                f.stage = 2;
                if (nd.right >= 0) {
                    if (nd.left >= 0) gap[next_leaf - 1] = c;
                    enter(nd.right, c, depth + 1);
                    continue;
                }
            }
            t.clades[c].n_leaves = next_leaf - t.clades[c].first_leaf;
            st.pop_back();
        }
    }
    for (size_t c = 0; c < t.clades.size(); ++c) t.clades[c].name = t.clade_names[c].c_str();
    const size_t nc = t.clades.size();
    t.top_clade = 0;
    while (t.top_clade + 1 < nc && t.clades[t.top_clade + 1].n_leaves == nl) ++t.top_clade;  // (a chain of one-child nodes from the root)
    if (nl) {
        uint32_t levels = 1;
        while ((2ull << (levels - 1)) <= gap.size()) ++levels;
        std::vector<uint32_t> tab((size_t)levels * nl, PFQ_NO_CLADE);
        std::copy(gap.begin(), gap.end(), tab.begin());
        for (uint32_t j = 1; j < levels; ++j) {
            const size_t half = (size_t)1 << (j - 1);
            const uint32_t *prev = tab.data() + (size_t)(j - 1) * nl;
            uint32_t *cur = tab.data() + (size_t)j * nl;
            for (size_t i = 0; i + 2 * half <= gap.size(); ++i) cur[i] = std::min(prev[i], prev[i + half]);
        }
        HIP_TRY(t.d_leaf_clade.ensure(nl));
        HIP_TRY(t.d_gap_min.ensure(tab.size()));
        HIP_TRY(t.d_clade_here.ensure(nc));
        HIP_TRY(hipMemcpy(t.d_leaf_clade.p, leaf_clade.data(), nl * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t.d_gap_min.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(t.d_clade_here.p, 0, nc * 8));
    }
    t.lca_valid = true;
    return PFQ_OK;
}

// ---- PFQ_WANT_ABUNDANCE: the log of the calls' rows (pfq_tree::d_ab_*) ----
static_assert(pfq::ABUND_Q == PFQ_ABUND_Q, "pfq.h and pfq_kernels.h disagree about the mass unit");
constexpr uint64_t ABUND_MAX_UNITS = 0xffffffffull;  // a[l] < 2^48, so a[l] << 16 fits 64 bits
constexpr size_t ABUND_LOG_MIN = 1024;               // first allocation of a log buffer (elements); then it at least doubles

// Empties the log and gives its memory back (hipFree waits for the device).
void abund_clear(pfq_tree &t) {
    t.d_ab_start.release();
    t.d_ab_len.release();
    t.d_ab_entries.release();
    t.d_ab_unique.release();
    t.ab_rows = t.ab_entries = t.ab_units = t.ab_unhit = t.ab_unique = t.ab_all = 0;
    t.ab_incomplete = false;
}
// Room for `want` elements with the first `used` kept: max(want, twice the size, ABUND_LOG_MIN), or just `want` where
// that much memory is not to be had.  On failure the buffer is what it was.  The device is idle (the caller has waited).
template <typename T>
hipError_t grow_copy(DevBuf<T> &b, size_t used, size_t want) {
    if (want <= b.n) return hipSuccess;
    size_t cap = std::max(std::max(want, 2 * b.n), ABUND_LOG_MIN);
    T *p = nullptr;
    hipError_t e = hipMalloc(&p, cap * sizeof(T));
    if (e != hipSuccess && cap > want) {
        (void)hipGetLastError();
        cap = want;
        e = hipMalloc(&p, cap * sizeof(T));
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e;
    }
    if (used) e = hipMemcpy(p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return e;
    }
    if (b.p) (void)hipFree(b.p);
    b.p = p;
    b.n = cap;
    return hipSuccess;
}
// Why `units` more units with `entries` more leaf entries in ambiguous rows cannot be logged ("" = they can), before anything
// is changed: the 2^32 - 1 unit bound, the PFQ_ABUND_SLOTS cap.
std::string abund_refusal(const pfq_tree &t, uint64_t units, uint64_t entries) {
    if (t.ab_incomplete) return "an earlier call's rows did not fit, the log is incomplete";
    if (units > ABUND_MAX_UNITS - t.ab_units)
        return "more than 2^32 - 1 units (" + std::to_string(t.ab_units) + " logged, " + std::to_string(units) + " more)";
    if (t.knobs.abund_slots >= 0 && t.ab_entries + entries > (uint64_t)t.knobs.abund_slots)
        return std::to_string(t.ab_entries) + " leaf entries held and " + std::to_string(entries) + " more exceed PFQ_ABUND_SLOTS = " +
               std::to_string(t.knobs.abund_slots);
    return "";
}
// Device room for `rows` more ambiguous rows with `entries` more entries, and the unique counters.  false: out of memory.
int abund_room(pfq_tree &t, uint64_t rows, uint64_t entries, bool &ok) {
    ok = grow_copy(t.d_ab_start, t.ab_rows, t.ab_rows + rows) == hipSuccess && grow_copy(t.d_ab_len, t.ab_rows, t.ab_rows + rows) == hipSuccess &&
         grow_copy(t.d_ab_entries, t.ab_entries, t.ab_entries + entries) == hipSuccess;
    if (!ok) return PFQ_OK;
    if (!t.d_ab_unique.p && !t.leaves.empty()) {
        HIP_TRY(t.d_ab_unique.ensure(t.leaves.size()));
        HIP_TRY(hipMemset(t.d_ab_unique.p, 0, t.leaves.size() * 8));
    }
    HIP_TRY(t.d_ab_cur.ensure(2 + pfq::ABUND_CNT_N));
    return PFQ_OK;
}
int abund_shard_refused() {
    return fail(PFQ_ERR_UNSUPPORTED, "PFQ_WANT_ABUNDANCE on a subtree shard: a shard sees only its own leaves, so the rows it would log "
                                     "are partial");
}

// ---- PFQ_WANT_TAXA: the user's taxonomy (pfq_tree::tax, d_tax_*) ----
// Drops the taxonomy and gives its tables back (hipFree waits for the device): the leaves are no longer the ones it described.
void tax_clear(pfq_tree &t) {
    for (DevBuf<uint32_t> *b : {&t.d_tax_rank, &t.d_tax_leaf_node, &t.d_tax_parent, &t.d_tax_first, &t.d_tax_gap_min}) b->release();
    for (DevBuf<unsigned long long> *b : {&t.d_tax_here, &t.d_tax_any, &t.d_tax_misc}) b->release();
    t.tax = pfq_taxonomy::NodeTable();
    t.tax_set = false;
}
int tax_zero(pfq_tree &t) {
    if (!t.tax_set) return PFQ_OK;
    HIP_TRY(hipMemset(t.d_tax_here.p, 0, t.tax.nodes.size() * 8));
    HIP_TRY(hipMemset(t.d_tax_any.p, 0, t.tax.nodes.size() * 8));
    HIP_TRY(hipMemset(t.d_tax_misc.p, 0, pfq::TAX_MISC_N * 8));
    return PFQ_OK;
}
static_assert(pfq::TAX_NO_NODE == PFQ_NO_CLADE, "pfq.h and pfq_kernels.h disagree about \"no node\"");

// ---- PFQ_WANT_SWEEP: the counters of the threshold list (pfq_tree::d_sw_state) ----
static_assert(pfq::SWEEP_MAX == PFQ_SWEEP_MAX, "pfq.h and pfq_kernels.h disagree about the longest sweep list");
size_t sweep_words(size_t n_thr, size_t nl) { return (2 * n_thr + 1) * nl + n_thr + 1; }
// Gives the counters' memory back (hipFree waits for the device); the list stays.
void sweep_drop(pfq_tree &t) {
    t.d_sw_state.release();
    t.sw_nl = 0;
    t.sw_units = 0;
}
// The counters of the list over nl leaves, zeroed on `st` if they are made here.  No list: nothing.
int sweep_ensure(pfq_tree &t, size_t nl, hipStream_t st) {
    if (t.sw_thr.empty() || (t.d_sw_state.p && t.sw_nl == nl)) return PFQ_OK;
    sweep_drop(t);
    const size_t words = sweep_words(t.sw_thr.size(), nl);
    if ((t.sw_thr.size() + 1) * nl >= (1ull << 32) || t.d_sw_state.ensure(words) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PFQ_ERR_DEVICE, "no device memory for the threshold sweep's counters (" + std::to_string(words * 8) + " bytes: " + std::to_string(nl) +
                                    " leaves, " + std::to_string(t.sw_thr.size()) + " thresholds)");
    }
    t.sw_nl = nl;
    HIP_TRY(hipMemsetAsync(t.d_sw_state.p, 0, words * 8, st));
    return PFQ_OK;
}
// Zeroes the counters; the device is idle.
int sweep_zero(pfq_tree &t) {
    if (t.d_sw_state.p) HIP_TRY(hipMemset(t.d_sw_state.p, 0, sweep_words(t.sw_thr.size(), t.sw_nl) * 8));
    t.sw_units = 0;
    return PFQ_OK;
}
// Why a tree cannot be swept (pfq.h "threshold sweep"); PFQ_OK: it can.
int sweep_refused(const pfq_tree &t, const char *what) {
    if (t.is_shard)
        return fail(PFQ_ERR_UNSUPPORTED, std::string(what) + " on a subtree shard: a shard sees only its own leaves, so the units and the unique rows "
                                         "it would count are partial");
    if (!t.superset_all)
        return fail(PFQ_ERR_UNSUPPORTED, std::string(what) + " on a tree that is not superset-verified (pfq_info.superset_verified == 0): a read can "
                                         "fail a higher threshold at an ancestor whose score is not in its row, so the rows of the lowest "
                                         "threshold do not answer the others");
    return PFQ_OK;
}

// ---- PFQ_WANT_COVERAGE: the per-leaf sketches (pfq_tree::d_cov_*) ----
// The precision a new sketch gets: the option PFQ_COVER_P where it is in range (pfq_set_option refuses other values; one from
// the environment that is out of range counts as unset).
uint32_t cover_precision(const Knobs &k) {
    return k.cover_p >= (long long)pfq::COVER_P_MIN && k.cover_p <= (long long)pfq::COVER_P_MAX ? (uint32_t)k.cover_p : pfq::COVER_P_DEFAULT;
}
// Empties the sketch and gives its memory back (hipFree waits for the device).
void cover_clear(pfq_tree &t) {
    t.d_cov_regs.release();
    t.d_cov_cnt.release();
    t.cov_units = 0;
}
// The sketch of a tree of nl leaves, zeroed on `st` if it is made here.  Nothing of the call has run yet.
int cover_ensure(pfq_tree &t, size_t nl, hipStream_t st) {
    if (t.d_cov_regs.p || !nl) return PFQ_OK;
    const uint32_t p = cover_precision(t.knobs);
    if (t.d_cov_regs.ensure(nl << p) != hipSuccess || t.d_cov_cnt.ensure(2 * nl) != hipSuccess) {
        (void)hipGetLastError();
        cover_clear(t);
        return fail(PFQ_ERR_DEVICE, "no device memory for the coverage sketch (" + std::to_string((nl << p) + 16 * nl) + " bytes: " + std::to_string(nl) +
                                    " leaves, PFQ_COVER_P = " + std::to_string(p) + "); nothing of this call was sketched");
    }
    t.cov_p = p;
    HIP_TRY(hipMemsetAsync(t.d_cov_regs.p, 0, nl << p, st));
    HIP_TRY(hipMemsetAsync(t.d_cov_cnt.p, 0, 2 * nl * 8, st));
    return PFQ_OK;
}
// Set bits of every leaf's filter, once per topology.
int cover_filter_bits(pfq_tree &t) {
    const size_t nl = t.leaves.size();
    if (t.cov_bits_valid && t.cov_bits.size() == nl) return PFQ_OK;
    t.cov_bits.assign(nl, 0);
    if (nl) {
        DevBuf<unsigned long long> d_pop;
        HIP_TRY(d_pop.ensure(nl));
        pfq::launch_row_popcount(t.d_bits.p, t.n_words, t.d_col_row.p, (uint32_t)nl, d_pop.p, nullptr);  // (the first nl columns are the leaves)
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(t.cov_bits.data(), d_pop.p, nl * 8, hipMemcpyDeviceToHost));
    }
    t.screen_E = 0.0;
    for (size_t l = 0; l < nl; ++l) {
        const double f = (double)t.cov_bits[l] / (double)t.nbits;
        t.screen_E += f * f * f * f;
    }
    t.cov_bits_valid = true;
    return PFQ_OK;
}
// Classic HyperLogLog over the m = 2^p registers of one leaf (pfq.h "coverage").
double cover_estimate(const uint8_t *reg, uint32_t p) {
    const size_t m = (size_t)1 << p;
    double sum = 0.0;
    size_t zeros = 0;
    for (size_t j = 0; j < m; ++j) {
        sum += std::ldexp(1.0, -(int)reg[j]);
        zeros += reg[j] == 0;
    }
    if (zeros == m) return 0.0;
    const double dm = (double)m;
    const double alpha = p == 4 ? 0.673 : p == 5 ? 0.697 : p == 6 ? 0.709 : 0.7213 / (1.0 + 1.079 / dm);
    const double e = alpha * dm * dm / sum;
    return e <= 2.5 * dm && zeros > 0 ? dm * std::log(dm / (double)zeros) : e;
}

// The tree's own stream, for the uploads and stages that run beside the null stream's kernels; made by the first call that needs it.
int ensure_copy_stream(pfq_tree &t) {
    HIP_TRY(t.copy_stream.ensure(hipStreamNonBlocking));
    return PFQ_OK;
}

int ensure_scratch(pfq_tree &t, uint64_t n_reads, bool want_hits) {
    HIP_TRY(t.d_stats.ensure(pfq::ST_N));
    HIP_TRY(t.d_cursors.ensure(CUR_ALLOC));
    // two hits per read, or 1.3 x what recent blocks reported (a block that overflows is run again, see query_device)
    const uint64_t cap = (uint64_t)(std::max(2.0, 1.3 * t.hits_per_read) * (double)n_reads) + 1024;
    if (want_hits) {
        HIP_TRY(t.d_hit_pairs.ensure(cap));
        HIP_TRY(t.d_allhit.ensure(n_reads + 1));
        HIP_TRY(t.d_counts_snapshot.ensure(t.leaves.size() + 1));
    }
    return PFQ_OK;
}
constexpr uint64_t CLASSIFY_MAX_BLOCKS = 4096;  // blocks of 4 waves; every wave may leave one reservation partly used

// Scratch of the bucketed path.  false: not enough device memory, the caller stays on the direct kernel.
bool ensure_bucket_scratch(pfq_tree &t, uint64_t n_reads, bool with_guards, uint64_t launch_waves, uint32_t pair_ahead) {
    if (!t.h_pair_cursor.p) {  // (made last: where it exists, so does the event)
        if (t.hint_ev.ensure(hipEventDisableTiming) != hipSuccess || t.h_pair_cursor.ensure(HINT_N) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        for (int i = 0; i < HINT_N; ++i) t.h_pair_cursor.p[i] = 0;
    } else if (t.hint_reads && hipEventQuery(t.hint_ev) == hipSuccess) {
        t.pairs_per_read = std::max(t.pairs_per_read, (double)t.h_pair_cursor.p[HINT_PAIRS] / (double)t.hint_reads);
        if (t.hint_entry_cap) t.passes_hint = std::max<uint64_t>(1, (t.h_pair_cursor.p[HINT_TILE_ENTRIES] + t.hint_entry_cap - 1) / t.hint_entry_cap);
        if (t.hint_counts) t.dirty_frac = (double)t.h_pair_cursor.p[HINT_DIRTY] / (double)std::max<unsigned long long>(1, t.h_pair_cursor.p[HINT_SORTED] & 0xffffffffull);
        t.cand_per_read = (double)t.h_pair_cursor.p[HINT_CANDIDATES] / (double)t.hint_reads;
        t.have_cand_hint = true;
        t.hint_reads = 0;
    }
    (void)hipGetLastError();  // hipEventQuery reports "not ready" through the error state
    // room for two candidates per read, or for 1.3 x what recent calls deferred (at most 24 per read: 40 B per slot);
    // + one partially used reservation per wave and the pair_ahead it may hold beyond.  Pairs that do not fit are certified
    // inline (exact, slow).
    const double per_read = std::min(24.0, std::max(2.0, 1.3 * t.pairs_per_read));
    uint64_t cap = ((uint64_t)(per_read * (double)n_reads) + (1 + (uint64_t)pair_ahead) * pfq::PAIR_RESERVE * launch_waves + 1024 + 31) & ~31ull;
    // pairs deferred by k_classify: slots [0, leaf_cap); guard pairs (k_expand_guards): [leaf_cap, leaf_cap + guard_cap),
    // sized by the tree's guards per leaf (what does not fit is certified inline there)
    if (t.d_pairs.n && t.leaf_cap >= cap) cap = t.leaf_cap;  // (the buffers only grow)
    t.leaf_cap = cap;
    t.guard_cap = 0;
    if (with_guards) {
        const double per_leaf = (double)t.guard_col.size() / (double)std::max<size_t>(1, t.leaves.size());
        t.guard_cap = ((uint64_t)((double)cap * std::min(4.0, std::max(0.25, per_leaf))) + 32 * 4 * 2048 + 31) & ~31ull;
        cap += t.guard_cap;
    }
    bool ok = soft_ensure(t.d_pairs, cap) && soft_ensure(t.d_sorted, cap) && soft_ensure(t.d_fail, cap) &&
              soft_ensure(t.d_bucket, 3 * ((size_t)t.n_cols << 6) + 2) &&  // up to 64 sub-buckets per column
              soft_ensure(t.d_queue, 128);
    if (ok && with_guards)
        ok = soft_ensure(t.d_owner, t.d_pairs.n) && soft_ensure(t.d_owner_sorted, t.d_pairs.n) && soft_ensure(t.d_gfail, t.d_pairs.n);
    return ok;
}

constexpr int PROF_EV = 7;  // start, classify, bucket, plan+bin, test, verify, finalize
constexpr uint64_t BUCKET_MIN_READS = 1ull << 18;  // below this the bucketed pass cannot amortise warming the L2 slices
constexpr uint64_t SLICE_TARGET_BYTES = 2560ull << 10;

// One pfq_query_batch[_device] call.  plan() chooses the path and the modes from the tree, the threshold, the knobs, the room
// the device has left and — block mode, on a tree without history — a screened sample of the block's own reads; attempt() is
// one run of the kernels (a second one only when the hit buffer proved too small), stage by stage: frontier(), then on the
// bucketed path setup_pairs() -> frontier(true) -> expand guards / tail records -> bucket_sort() -> setup_verify() ->
// tile_stage() -> finish_blocks() or finish_pairs().  read_hits() then looks at the hit pairs: it asks for the second attempt,
// or builds the reads' CSR (fragments: pair_hits()), which deliver_rows() hands to the caller with the scores, the LCAs and
// the abundance log.  Everything is queued on `st`; results never depend on which modes were chosen.
struct QueryRun {
    pfq_tree &t;
    const uint8_t *d_seq;
    const uint64_t *d_off;
    uint64_t n_reads, total_bytes;
    float threshold;
    uint32_t flags;
    hipStream_t st;
    pfq_hits *hits;
    const Knobs &kn;
    // ---- the plan
    bool want_hits = false, want_scores = false, paired = false, pair_both = false, user_hits = false, want_lca = false, lca_best = false, want_abund = false, want_cover = false, want_taxa = false, rows_best = false, want_sweep = false, results_stand = false, with_guards = false, thr_one = false, thr_frac = false, counts_mode = false;
    bool pair_miss = false;    // counts_mode outside block mode: every deferred pair owns words of k-mer miss bits
    bool guard_pairs = false;  // guard columns outside block mode: the guards are pairs of their own, in a region of their own
    bool recs_possible = false, bucketed = false, block_mode = false, want_two_level = false, lean_screen = false;
    size_t nl = 0, nc = 0, guarded = 0, nb = 0, mem_free = 0, mem_total = 0;
    uint32_t group_cols = 0, leaf_groups = 1, n_tiles_block = 0, sub_log2 = 0, pair_ahead = 0;
    int blocks = 0, blocks_group = 0;
    uint64_t launch_waves = 0, n_blocks = 0, miss_cap = 0, hit_cap = 0;
    // ---- one attempt
    pfq::QueryArgs a{};
    Event *ev = nullptr;
    uint32_t *cnt = nullptr, *off = nullptr, *cur = nullptr, *cntw = nullptr, *offw = nullptr, *curw = nullptr;  // bucket histograms / offsets / cursors
    uint4 *recs = nullptr;
    uint32_t n_slices = 1;
    pfq::GuardArgs ga{};
    pfq::VerifyArgs v{};
    int vblocks = 512, vthreads = 512;
    // pfq_query_frames: the reads are a call's frames.  They count into the sink and their CSR stays on the device (d_hit_off /
    // d_hit_leaves, rows_total entries) for the segment stage; nothing is handed to a caller.
    bool frames = false;
    uint64_t rows_total = 0;
    // pfq_prep_deplete: the call is a screen's, on a block of another tree.  It builds the hit pairs (with their overflow retry)
    // like PFQ_WANT_LCA alone and hands nothing to a caller: reads leave a flag per read with a hit pair in deplete_hit (zeroed
    // by the caller), fragments their final CSR offsets in d_frag_off; the all-hit bytes stay in d_allhit.  Its small reads go
    // through `st`, not the null stream, so that nothing of the call waits for what another tree has queued there.
    bool deplete = false;
    uint32_t *deplete_hit = nullptr;

    QueryRun(pfq_tree &t_, const uint8_t *seq_, const uint64_t *off_, uint64_t n_, uint64_t bytes_, float thr_, uint32_t flags_, hipStream_t st_,
             pfq_hits *hits_)
        : t(t_), d_seq(seq_), d_off(off_), n_reads(n_), total_bytes(bytes_), threshold(thr_), flags(flags_), st(st_), hits(hits_), kn(t_.knobs) {}

    int plan() {
        if (t.root < 0) return fail(PFQ_ERR_STATE, "query on an empty tree");
        PFQ_TRY(build_layout(t));
        user_hits = (flags & PFQ_WANT_HITS) != 0;
        want_scores = (flags & PFQ_WANT_SCORES) != 0;
        paired = (flags & PFQ_PAIRED) != 0;
        pair_both = (flags & PFQ_PAIR_BOTH) != 0;
        if (user_hits && !hits) return fail(PFQ_ERR_ARG, "PFQ_WANT_HITS set but hits == NULL");
        want_lca = (flags & PFQ_WANT_LCA) != 0;
        lca_best = (flags & PFQ_LCA_BEST) != 0;
        want_abund = (flags & PFQ_WANT_ABUNDANCE) != 0;
        want_cover = (flags & PFQ_WANT_COVERAGE) != 0;
        want_taxa = (flags & PFQ_WANT_TAXA) != 0;
        rows_best = (flags & PFQ_ROWS_BEST) != 0;
        want_sweep = (flags & PFQ_WANT_SWEEP) != 0;
        if (want_sweep) PFQ_TRY(sweep_refused(t, "PFQ_WANT_SWEEP"));  // (the list was set on a tree that has changed since)
        if (want_taxa && (!t.tax_set || t.tax.rank.size() != t.leaves.size()))
            return fail(PFQ_ERR_STATE, "PFQ_WANT_TAXA without a taxonomy: pfq_tree_set_taxonomy first (pfq_tree_prune and pfq_tree_insert drop it)");
        if (want_lca) PFQ_TRY(ensure_lca(t));
        want_hits = user_hits || paired || want_lca || deplete;  // (fragments and LCAs are combined from the reads' hit lists)
        if (n_reads >= (1ull << 31) - 1024) return fail(PFQ_ERR_ARG, "more than 2^31 reads in one block");
        // the scratch buffers are reused call after call: calls on one stream are ordered by it, a change of stream waits
        HIP_TRY(t.last_done.ensure(hipEventDisableTiming));
        if (t.have_last_stream && t.last_stream != st) HIP_TRY(hipEventSynchronize(t.last_done));
        t.last_stream = st;
        t.have_last_stream = true;
        t.last_n_reads = n_reads;
        PFQ_TRY(ensure_scratch(t, n_reads, want_hits));
        nl = t.leaves.size();
        if (want_cover) PFQ_TRY(cover_ensure(t, nl, st));  // (before anything of the call runs: a failure sketches nothing)
        if (want_sweep) PFQ_TRY(sweep_ensure(t, nl, st));
        if (paired || frames) HIP_TRY(t.d_pair_sink.ensure(nl + 1));
        nc = t.n_cols;  // leaf + guard columns = buckets of the bucketed path (block mode: blocks of 8 leaf columns)
        with_guards = !t.guard_col.empty();
        // bucketed path: threshold 1 (any certificate kernel), or 0 < threshold < 1 with probe records (per-pair k-mer miss bits)
        thr_one = threshold == 1.0f;
        thr_frac = threshold > 0.0f && threshold < 1.0f;
        // budgets of the two large scratch buffers: what the device can still give (plus what the tree already holds of it),
        // at most 64 GB each, unless a knob says otherwise; a failed allocation degrades to the next exact path below
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = 0; }
        uint64_t rec_budget = std::min<uint64_t>(64ull << 30, (uint64_t)((double)(mem_free + t.d_recs.bytes()) * 0.45));
        if (kn.record_gb >= 0) rec_budget = (uint64_t)kn.record_gb << 30;
        recs_possible = total_bytes && t.nbits < (1ull << 30) && t.num_hashes <= 35 && total_bytes * 16 <= rec_budget;
        // (or as many bases as 2^18 reads of 150 bp: long reads bring the same certificate work with fewer reads)
        bucketed = (t.force_path == 1) || (t.force_path < 0 && (n_reads >= BUCKET_MIN_READS || total_bytes >= BUCKET_MIN_READS * 150));
        if (!(thr_one || thr_frac) || nl == 0 || n_reads == 0) bucketed = false;
        // probe records: hash survivors once instead of once per slice (needs d < 2^30, <= 35 hashes, room)
        if (bucketed && recs_possible && !soft_ensure(t.d_recs, total_bytes + 64)) recs_possible = false;
        if (bucketed && thr_frac && !recs_possible) bucketed = false;  // the miss bits of thresholds < 1 come from the records
        // the classify launches of this call: one per group of leaf columns (two for thresholds < 1: reads of >= 256 k-mers), on
        // all reads, or — two-level frontier — on the reads the coarse launch lists for the group
        group_cols = 1u << t.group_log2;
        leaf_groups = (uint32_t)std::max<size_t>(1, (nl + group_cols - 1) / group_cols);
        blocks = (int)std::min<uint64_t>((n_reads + 3) / 4, CLASSIFY_MAX_BLOCKS);  // (2048: 10.1 ms, 4096: 9.9 ms per step)
        if (kn.classify_blocks > 0) blocks = (int)std::min<long long>(blocks, kn.classify_blocks);
        // threshold 1: a wave's batched emission reserves pair slots for its next passes too (k_classify, emit_pass)
        pair_ahead = threshold >= 1.0f ? (uint32_t)(kn.pair_ahead >= 0 ? std::min<long long>(kn.pair_ahead, 16) : 8) : 0u;
        want_two_level = t.coarse_valid && leaf_groups > 1 && (kn.coarse > 0 || threshold >= 1.0f || t.coarse_fill <= 0.70);
        blocks_group = want_two_level ? std::min(blocks, 1024) : blocks;  // (a list holds a fraction of the reads)
        launch_waves = 4ull * (uint64_t)blocks_group * leaf_groups * (threshold >= 1.0f ? 1 : 2);
        if (bucketed && !ensure_bucket_scratch(t, n_reads, with_guards, launch_waves, pair_ahead)) bucketed = false;
        if (bucketed && recs_possible && !soft_ensure(t.d_meta, t.d_pairs.n)) recs_possible = false;
        if (bucketed && thr_frac && !recs_possible) bucketed = false;
        counts_mode = !(threshold >= 1.0f);  // theta >= 1: need >= n for every read with k-mers
        // Block mode (pfq::TILE_LOG2_BLOCK): reads that pass several leaves of a block of 8 (strains of one phage) are certified
        // once per block.  Threshold 1, no guard columns, records and room for the tables; chosen when recent calls saw more
        // than 1.5 candidate leaves per read (PFQ_BLOCK=1 / 0 forces / forbids it).  Results do not depend on the choice.
        n_blocks = (nl + 7) / 8;
        n_tiles_block = (uint32_t)((t.n_words * 64 + (1ull << pfq::TILE_LOG2_BLOCK) - 1) >> pfq::TILE_LOG2_BLOCK);
        // (Guard columns — reference-built trees whose internal names collide: the guards of a hit are certified against the
        // sliced matrix afterwards, 1300 line gathers each, which pays while few leaves have guards: <= 5 % of them.)
        guarded = 0;
        for (size_t c = 0; with_guards && c < nl; ++c) guarded += t.guard_off[c + 1] > t.guard_off[c];
        // Candidate leaves per read decide between the pair pipeline and block mode.  Later calls take the figure of the call
        // before; a call without that history (the first on a tree, the first after its layout changed) screens a sample of its
        // OWN reads first — the frontier only, nothing is certified or counted — so that a workload of related genomes does not
        // run its first block through the pair pipeline.  One small launch per column group and one read-back.
        const bool block_eligible = bucketed && (thr_one || (thr_frac && kn.tile_counts != 0)) && recs_possible && n_tiles_block <= 560 &&
                                    n_blocks < (1u << 16) && (kn.tile < 0 || kn.tile != 0);
        if (block_eligible && kn.block < 0 && !t.have_cand_hint && guarded * 20 <= nl) PFQ_TRY(sample_candidates());
        // At thresholds below 1 block mode keeps the k-mer entries: buckets by (block, candidate mask), 8 miss bytes per k-mer.
        block_mode = block_eligible && (kn.block >= 0 ? kn.block != 0 : (t.cand_per_read > 1.5 && guarded * 20 <= nl));
        if (block_mode && !soft_ensure(t.d_T, n_blocks * t.n_words * 64)) block_mode = false;
        if (block_mode && !soft_ensure(t.d_failb, t.d_pairs.n * 8)) block_mode = false;
        if (block_mode) nc = n_blocks * 256;  // buckets by (block, candidate mask)
        pair_miss = counts_mode && !block_mode;  // (block_mode is final here; neither flag depends on `bucketed`)
        guard_pairs = with_guards && !block_mode;
        t.last_block_mode = 0;
        miss_cap = 0;
        nb = 0;
        sub_log2 = 0;
        if (bucketed) {
            // sub-buckets (keyed by the read index) keep every histogram counter cold when columns are few
            while (sub_log2 < 6 && (nc << sub_log2) < 1024) ++sub_log2;
            nb = nc << sub_log2;
            if (block_mode && !soft_ensure(t.d_bucket, 3 * nb + 2)) bucketed = false;  // (buckets by (block, mask) outnumber the columns of small trees)
            if (pair_miss) {  // thresholds < 1: every deferred pair owns ceil(n/64) words of k-mer miss bits that the slices OR into
                const uint64_t avg_len = n_reads ? total_bytes / n_reads : 0;
                miss_cap = std::min<uint64_t>((t.leaf_cap + t.guard_cap) * ((avg_len >> 6) + 2) + (launch_waves + 4 * 2048) * (uint64_t)pfq::MISS_RESERVE, 0xfffffff0ull);
                if (!(soft_ensure(t.d_miss_words, miss_cap) && soft_ensure(t.d_miss_pos, t.d_pairs.n) && soft_ensure(t.d_bucket_w, 3 * nb + 2)))
                    bucketed = false;
            }
        }
        if (bucketed && kn.miss_words >= 0) miss_cap = std::min<uint64_t>(miss_cap, (uint64_t)kn.miss_words);
        // The lean dense screen: 2 k-mers of 32 reads a pass instead of 4 of 16 — half the row gathers, the passes and the
        // hashing of k_classify.  The screen is a necessary condition only (every pair it lets through is certified probe by
        // probe), so fewer rows change no result; they let more foreign reads through.  A random read keeps a leaf whose filter
        // has the fraction f of its bits set with probability f^4 after four rows, so E = sum over the leaves of
        // (popcount / nbits)^4 is the expected number of false pairs a read.  A false pair costs what a true one costs behind
        // the screen, about 3 ns of bin + test + records (13.4 ms for 4.2 M pairs); the lean screen saves about
        // 0.1 ns a read: break-even at E = 0.03.  The rule asks for E <= 2^-10, a factor of thirty below.  The popcounts are
        // the coverage report's (cover_filter_bits: once per topology).  Only the pair pipeline at threshold 1 on all reads
        // has the build: not block mode, not the leaf groups of a two-level frontier, and rows of at most 32 words (the
        // frontier words of 32 reads fill the wave's 1024 words of LDS).  PFQ_SCREEN_KMERS=2 / 4 forces / forbids it.
        lean_screen = false;
        if (bucketed && thr_one && !block_mode && leaf_groups == 1 && t.rw <= 32 && kn.screen_kmers != 4) {
            if (kn.screen_kmers == 2) lean_screen = true;
            else {
                PFQ_TRY(cover_filter_bits(t));
                lean_screen = t.screen_E <= 1.0 / 1024.0;
            }
        }
        t.last_screen_kmers = 0;
        t.last_pair_ahead = 0;
        t.last_path = bucketed ? 1 : 0;
        t.last_sort = 0;
        if (!bucketed) t.last_tile_mode = t.last_tile_bin = 0;  // (the direct path runs no tile pass)
        hit_cap = t.d_hit_pairs.n;
        if (kn.hit_slots >= 0) hit_cap = std::min<uint64_t>(hit_cap, (uint64_t)kn.hit_slots);  // (first attempt only, see read_hits)
        t.last_pair_cap = t.last_guard_cap = t.last_kmiss_cap = t.last_hit_cursor0 = t.last_attempts = 0;
        t.last_miss_cap = miss_cap;
        t.last_hit_cap0 = want_hits ? hit_cap : 0;
        t.last_nb = bucketed ? nb : 0;
        return PFQ_OK;
    }

    // what every classify launch of this call is told about the block, the threshold and the tree's layout; the callers add
    // the number of reads and where the launch counts and lists hits
    pfq::QueryArgs base_args() const {
        pfq::QueryArgs q{};
        q.hp = t.hp;
        q.seq = d_seq;
        q.off = d_off;
        q.threshold = threshold;
        q.S_all = t.d_S.p;
        q.group_stride = t.group_stride;
        q.group_log2 = t.group_log2;
        q.ones_row = (uint32_t)(t.n_words * 64);
        q.rw = t.rw;
        q.rw_log2 = t.rw_log2;
        q.n_cols = t.n_cols;
        q.guard_off = t.d_guard_off.p;
        q.guard_col = t.d_guard_col.p;
        q.hit_cursor = t.d_cursors.p + CUR_HIT;
        q.stats = t.d_stats.p;
        if (counts_mode) {  // thresholds < 1: the queue of reads of >= 256 k-mers (d_long holds n_reads + 1 by now)
            q.long_list = t.d_long.p;
            q.n_long = t.cur_lo(CUR_LONG);
        }
        return q;
    }

    // Candidates per read of the first reads of this block: the frontier only, nothing is certified or counted.
    int sample_candidates() {
        const uint64_t n_s = std::min<uint64_t>(n_reads, 16384);
        HIP_TRY(hipMemsetAsync(t.d_stats.p, 0, pfq::ST_N * 8, st));
        HIP_TRY(hipMemsetAsync(t.d_cursors.p, 0, CUR_ALLOC * 8, st));
        if (counts_mode) HIP_TRY(t.d_long.ensure(n_reads + 1));
        pfq::QueryArgs sa = base_args();
        sa.n_reads = n_s;
        sa.counts = t.d_counts.p;
        sa.screen_only = 1;
        PFQ_TRY(classify_groups(sa, false, (int)std::min<uint64_t>((n_s + 3) / 4, CLASSIFY_MAX_BLOCKS)));
        HIP_TRY(hipGetLastError());
        unsigned long long cand = 0;
        HIP_TRY(hipMemcpyAsync(&cand, t.d_stats.p + pfq::ST_CANDIDATES, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        t.cand_per_read = (double)cand / (double)n_s;
        t.have_cand_hint = true;
        return PFQ_OK;
    }

    // the frontier kernels, once per column group that holds leaves (a tree of up to 2048 columns has one group)
    int frontier(bool defer) {
        // Two-level frontier: the coarse launch screens every read against an antichain of internal nodes and lists
        // it for the leaf groups below its live columns; a group's launch then sees only its list.
        // (thresholds < 1: only while the coarse filters are empty enough for <= 4 probes per k-mer to tell a miss)
        bool two_level = want_two_level;
        uint32_t list_cap = 0;
        if (two_level) {
            // every read at most once per list + one partly used reservation of 32 per wave of the (two) coarse launches
            list_cap = (uint32_t)((n_reads + 2 * 32ull * 4 * (uint64_t)blocks + 63) & ~31ull);
            if (!soft_ensure(t.d_glists, (size_t)list_cap * leaf_groups)) two_level = false;
            if (two_level && counts_mode && !soft_ensure(t.d_glong, (size_t)list_cap * leaf_groups)) two_level = false;
        }
        t.last_leaf_groups = leaf_groups;
        t.last_coarse_cols = t.last_coarse_probes = 0;
        if (two_level) {
            pfq::QueryArgs ac = a;
            ac.S = ac.S_all = t.d_Sc.p;
            ac.group_stride = 0;
            ac.group_log2 = 11;
            ac.col0 = 0;
            ac.n_leaves = ac.n_cols = t.coarse_cols;
            ac.rw = t.coarse_rw;
            ac.rw_log2 = t.coarse_rw_log2;
            ac.first_group = 1;
            pfq::CoarseArgs ca{};
            ca.cgrp = t.d_cgrp.p;
            ca.n_groups = leaf_groups;
            ca.lists = t.d_glists.p;
            ca.cursors = t.d_gcur.p;
            ca.list_cap = list_cap;
            ca.total_leaves = (uint32_t)nl;
            // probes per k-mer: enough for a foreign read to lose every coarse column.  Threshold 1 (AND over 4 k-mers):
            // columns x fill^(4 p) <= 0.02; below 1: a k-mer must be a miss with probability >= 0.85, 1 - fill^p
            const double f = std::min(0.999, std::max(1e-6, t.coarse_fill));
            uint32_t np;
            if (!counts_mode) {
                np = (uint32_t)std::ceil(std::log(0.02 / t.coarse_cols) / (4.0 * std::log(f)));
                np = std::min<uint32_t>(std::max<uint32_t>(np, 2), pfq::COARSE_MAX_PROBES);
            } else {
                np = 1;
                while (np < 4 && 1.0 - std::pow(f, (double)np) < 0.85) ++np;
                // k-mers looked at beyond maxmiss + 1 + 8, per 256 of maxmiss + 1: what the k-mers that are no misses cost
                const double pm = 1.0 - std::pow(f, (double)np);
                ca.scr_extra = (uint32_t)std::min(256.0, std::ceil(256.0 * (1.0 / pm - 1.0)));
            }
            if (kn.coarse_probes > 0) np = (uint32_t)std::min<long long>(kn.coarse_probes, counts_mode ? 4 : pfq::COARSE_MAX_PROBES);
            np = std::max<uint32_t>(1, std::min<uint32_t>(np, t.num_hashes));
            ca.n_probes = np;
            t.last_coarse_cols = t.coarse_cols;
            t.last_coarse_probes = np;
            HIP_TRY(hipMemsetAsync(t.d_gcur.p, 0, 2 * pfq::MAX_LEAF_GROUPS * sizeof(unsigned int), st));  // lists' cursors, long reads' cursors
            // (1024 blocks: every wave of the coarse launch may leave a reservation of 32 slots partly used in every group's list —
            // with 4096 blocks and ten groups the lists were half unused slots, and the leaf groups' dense screens half idle)
            int coarse_blocks = std::min(blocks, 1024);
            pfq::launch_coarse(ac, ca, counts_mode, coarse_blocks, st);
        }
        if (two_level) {
            // ONE launch for all leaf groups (blockIdx.y = the group: its matrix, columns and list follow from it); the
            // queues of reads of >= 256 k-mers (thresholds < 1) are per group as well, behind the groups' cursors
            a.S = t.d_S.p;
            a.col0 = 0;
            a.n_leaves = (uint32_t)std::min<size_t>(group_cols, nl);
            a.first_group = 0;
            a.read_list = t.d_glists.p;
            a.n_list = t.d_gcur.p;
            a.grid_groups = leaf_groups;
            a.total_leaves = (uint32_t)nl;
            a.list_cap = list_cap;
            if (counts_mode) {
                a.long_list = t.d_glong.p;
                a.n_long = t.d_gcur.p + pfq::MAX_LEAF_GROUPS;
            }
            pfq::launch_classify(a, defer, counts_mode, blocks_group, st);
            a.read_list = nullptr;
            a.n_list = nullptr;
            a.grid_groups = 0;
            if (counts_mode) {
                a.long_list = t.d_long.p;
                a.n_long = t.cur_lo(CUR_LONG);
            }
            return PFQ_OK;
        }
        return classify_groups(a, defer, blocks);
    }
    // one classify launch per column group that holds leaves, on all reads
    int classify_groups(pfq::QueryArgs &q, bool defer, int n_blocks_launch) {
        for (uint32_t g = 0; g < leaf_groups; ++g) {
            q.S = t.d_S.p + (uint64_t)g * t.group_stride;
            q.col0 = g * group_cols;
            q.n_leaves = (uint32_t)std::min<size_t>(group_cols, nl - (size_t)g * group_cols);
            q.first_group = g == 0;
            if (g && counts_mode) HIP_TRY(hipMemsetAsync(t.d_cursors.p + CUR_LONG, 0, 8, st));  // the queue of long reads is per launch
            pfq::launch_classify(q, defer, counts_mode, n_blocks_launch, st);
        }
        return PFQ_OK;
    }

    int attempt(int attempt_no) {
        t.last_attempts = (uint32_t)attempt_no + 1;
        HIP_TRY(hipMemsetAsync(t.d_stats.p, 0, pfq::ST_N * 8, st));
        HIP_TRY(hipMemsetAsync(t.d_cursors.p, 0, CUR_ALLOC * 8, st));
        if (want_hits) {
            HIP_TRY(hipMemsetAsync(t.d_allhit.p, 0, n_reads + 1, st));
            if (attempt_no == 0 && nl)
                HIP_TRY(hipMemcpyAsync(t.d_counts_snapshot.p, t.d_counts.p, nl * 8, hipMemcpyDeviceToDevice, st));
        }
        if (n_reads && nl) {
            if (counts_mode) HIP_TRY(t.d_long.ensure(n_reads + 1));
            a = base_args();
            a.n_reads = n_reads;
            a.counts = count_dst();
            a.hit_pairs = want_hits ? t.d_hit_pairs.p : nullptr;
            a.hit_cap = hit_cap;
            a.allhit_flag = want_hits ? t.d_allhit.p : nullptr;
            ev = nullptr;
            if (t.prof_used < t.prof_cap) {
                ev = &t.prof_ev[PROF_EV * t.prof_used];
                t.prof_bucketed[t.prof_used] = bucketed;
                ++t.prof_used;
            }
            if (ev) HIP_TRY(hipEventRecord(ev[0], st));
            if (bucketed) {
                PFQ_TRY(setup_pairs());
                PFQ_TRY(frontier(true));
                PFQ_TRY(guards_and_tails());
                PFQ_TRY(bucket_sort());
                PFQ_TRY(setup_verify());
                PFQ_TRY(tile_stage());
                if (block_mode) PFQ_TRY(finish_blocks());
                else PFQ_TRY(finish_pairs());
            } else {
                PFQ_TRY(frontier(false));
                if (ev) HIP_TRY(hipEventRecord(ev[1], st));
            }
            HIP_TRY(hipGetLastError());
        }
        if (bucketed) {  // how many pair slots this call used, for the next call's sizing
            HIP_TRY(hipMemcpyAsync(t.h_pair_cursor.p + HINT_PAIRS, t.d_cursors.p + CUR_PAIR, 16, hipMemcpyDeviceToHost, st));  // and HINT_TILE_ENTRIES
            HIP_TRY(hipMemcpyAsync(t.h_pair_cursor.p + HINT_DIRTY, t.d_cursors.p + CUR_DIRTY, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(t.h_pair_cursor.p + HINT_CANDIDATES, t.d_stats.p + pfq::ST_CANDIDATES, 8, hipMemcpyDeviceToHost, st));
            if (n_reads && nl)  // ... of how many sorted pairs (the pair cursor also counts partly used reservations)
                HIP_TRY(hipMemcpyAsync(t.h_pair_cursor.p + HINT_SORTED, t.d_bucket.p + 2 * (nc << t.last_sub_log2), 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(t.hint_ev, st));
            t.hint_reads = n_reads;
        }
        return PFQ_OK;
    }

    // where the classify / finalize kernels count: the tree's counters, or with PFQ_PAIRED a sink (fragments count afterwards;
    // the frames of pfq_query_frames likewise: sequences count afterwards)
    unsigned long long *count_dst() const { return paired || frames ? t.d_pair_sink.p : t.d_counts.p; }

    // deferred-pair buffer, bucket histograms, probe records, miss words; block tables on first use
    int setup_pairs() {
        t.last_sub_log2 = sub_log2;
        cnt = t.d_bucket.p;
        off = cnt + nb;
        cur = off + nb + 1;
        a.pairs = t.d_pairs.p;
        a.pair_cap = t.leaf_cap;  // whole reservations only (PAIR_CHUNK = 32)
        if (kn.pair_slots >= 0) a.pair_cap = std::min<uint64_t>(a.pair_cap, (uint64_t)kn.pair_slots & ~(uint64_t)(pfq::PAIR_RESERVE - 1));
        t.last_pair_cap = a.pair_cap;
        a.pair_cursor = t.d_cursors.p + CUR_PAIR;
        a.bucket_cnt = cnt;
        a.sub_log2 = sub_log2;
        recs = recs_possible ? t.d_recs.p : nullptr;
        a.recs = recs;
        a.rec_cap = recs ? t.d_recs.n : 0;
        cntw = offw = curw = nullptr;
        if (pair_miss) {
            cntw = t.d_bucket_w.p;
            offw = cntw + nb;
            curw = offw + nb + 1;
            HIP_TRY(hipMemsetAsync(t.d_miss_words.p, 0, miss_cap * 8, st));
            HIP_TRY(hipMemsetAsync(cntw, 0, nb * 4, st));
            a.bucket_words = cntw;
            a.miss_cursor = t.d_cursors.p + CUR_MISS_WORDS;
            a.miss_cap = miss_cap;
        }
        n_slices = 1;
        uint64_t slice_target = SLICE_TARGET_BYTES;
        if (kn.slice_kb > 0) slice_target = (uint64_t)kn.slice_kb << 10;
        while (n_slices < 8 && (t.n_words * 8 + n_slices - 1) / n_slices > slice_target) n_slices <<= 1;
        t.last_slices = n_slices;
        HIP_TRY(hipMemsetAsync(cnt, 0, nb * 4, st));
        HIP_TRY(hipMemsetAsync(t.d_fail.p, 0, t.d_fail.n * 4, st));
        if (with_guards) HIP_TRY(hipMemsetAsync(t.d_gfail.p, 0, t.d_gfail.n * 4, st));
        HIP_TRY(hipMemsetAsync(t.d_queue.p, 0, 128 * 4, st));
        // last windows of few k-mers are hashed several reads per pass afterwards: of up to 16 k-mers, or of up to 32 when the
        // reads' (average) length makes such tails — 100 bp reads at k = 20 have 64 + 17 k-mers
        a.batch_tails = 0;
        if (recs && !counts_mode && kn.no_tail_batch <= 0) {
            const uint64_t avg_len = n_reads ? total_bytes / n_reads : 0;
            const uint64_t tl = avg_len >= t.kmer_size ? ((avg_len - t.kmer_size + 1) & 63u) : 0;
            a.batch_tails = (tl > 16 && tl <= 32) ? 32u : 16u;
        }
        // theta = 1: k_classify only defers its survivors; k_tail_records, leaner and with no frontier to walk, hashes them
        // (PFQ_SPLIT_RECORDS=0: k_classify hashes every window it does not leave to the batched tails)
        a.split_recs = (recs && !counts_mode && kn.split_records != 0) ? 1u : 0u;
        a.block_pairs = block_mode ? 1u : 0u;
        a.batch_emit = kn.batch_emit != 0 ? 1u : 0u;  // (PFQ_BATCH_EMIT=0: the per-read loop for every survivor)
        a.lean_screen = lean_screen ? 1u : 0u;
        a.pair_ahead = (!counts_mode && !block_mode && a.batch_emit) ? pair_ahead : 0u;  // (only the batched emission reserves ahead)
        t.last_pair_ahead = a.pair_ahead;
        t.last_screen_kmers = counts_mode ? 0u : (lean_screen ? 2u : 4u);  // (thresholds < 1 have the counting screen)
        a.screen_recs = kn.screen_recs >= 0 ? (uint32_t)(kn.screen_recs != 0) : 1u;
        if (block_mode) {
            if (!t.tables_valid) {  // (the leaf set changed, or first use)
                pfq::launch_block_tables(t.d_bits.p, t.n_words, t.d_col_row.p, (uint32_t)nl, t.d_T.p, st);
                t.tables_valid = true;
            }
            HIP_TRY(hipMemsetAsync(t.d_failb.p, 0, t.d_failb.n, st));
        }
        return PFQ_OK;
    }
    // guard columns of the deferred pairs (pairs of their own), the probe records of the deferred reads
    int guards_and_tails() {
        ga = pfq::GuardArgs{};
        if (guard_pairs) {  // every guard of a deferred pair's leaf becomes a pair of its own (second region of the buffer)
            ga.pairs = t.d_pairs.p + t.leaf_cap;
            ga.cap = t.guard_cap;
            if (kn.guard_slots >= 0) ga.cap = std::min<uint64_t>(ga.cap, (uint64_t)kn.guard_slots);
            t.last_guard_cap = ga.cap;
            ga.cursor = t.d_cursors.p + CUR_GUARD;
            ga.slot0 = (uint32_t)t.leaf_cap;
            ga.owner = t.d_owner.p;
            ga.gfail = t.d_gfail.p;
            pfq::launch_expand_guards(a, ga, 2048, st);
        }
        if (a.batch_tails || a.split_recs) pfq::launch_tail_records(a, t.cur_lo(CUR_TAIL_SHAPES), 2048, st);
        if (ev) HIP_TRY(hipEventRecord(ev[1], st));
        return PFQ_OK;
    }
    // counting sort of the pairs by column (block mode: by (block, candidate mask))
    int bucket_sort() {
        pfq::launch_bucket_scan(cnt, off, cur, (uint32_t)nb, st);
        if (pair_miss) pfq::launch_bucket_scan(cntw, offw, curw, (uint32_t)nb, st);
        t.last_sort = pfq::launch_bucket_scatter(t.d_pairs.p, t.d_cursors.p + CUR_PAIR, a.pair_cap, off, cur, (uint32_t)nb, sub_log2, t.d_sorted.p,
                                                 recs ? t.d_meta.p : nullptr, d_off, block_mode ? nullptr : t.d_col_row.p, offw, curw,
                                                 pair_miss ? t.d_miss_pos.p : nullptr, (uint32_t)t.kmer_size,
                                                 guard_pairs ? t.d_owner.p : nullptr, guard_pairs ? t.d_owner_sorted.p : nullptr,
                                                 block_mode ? 2u : 0u, st);
        if (guard_pairs)  // (the guard pairs reserve on the same cursors)
            pfq::launch_bucket_scatter(ga.pairs, ga.cursor, ga.cap, off, cur, (uint32_t)nb, sub_log2, t.d_sorted.p,
                                       recs ? t.d_meta.p : nullptr, d_off, t.d_col_row.p, offw, curw,
                                       counts_mode ? t.d_miss_pos.p : nullptr, (uint32_t)t.kmer_size,
                                       t.d_owner.p + t.leaf_cap, t.d_owner_sorted.p, 0u, st);
        if (ev) HIP_TRY(hipEventRecord(ev[2], st));
        return PFQ_OK;
    }
    int setup_verify() {
        v = pfq::VerifyArgs{};
        v.hp = t.hp;
        v.seq = d_seq;
        v.off = d_off;
        v.bits = t.d_bits.p;
        v.col_row = t.d_col_row.p;
        v.n_words = t.n_words;
        v.sorted = t.d_sorted.p;
        v.n_pairs_ptr = off + nb;
        v.fail = t.d_fail.p;
        v.recs = recs;
        v.miss_words = pair_miss ? t.d_miss_words.p : nullptr;
        v.miss_pos = pair_miss ? t.d_miss_pos.p : nullptr;
        v.meta = t.d_meta.p;
        v.n_slices = n_slices;
        uint64_t sb = (t.n_words * 64 + n_slices - 1) / n_slices;
        v.slice_bits = (uint32_t)((sb + 63) & ~63ull);
        v.queue = t.d_queue.p;
        // window of pairs in flight per slice = (blocks/8)*(8/n_slices)*4*chunk: about one leaf bucket
        vblocks = 512;
        v.chunk = 1;
        if (kn.verify_blocks >= 0) vblocks = std::max(8, (int)kn.verify_blocks & ~7);
        if (kn.verify_chunk >= 0) v.chunk = (uint32_t)std::max(1, (int)kn.verify_chunk);
        v.n_sub = 8;
        if (kn.verify_sub >= 0) v.n_sub = (uint32_t)std::min(16, std::max(1, (int)kn.verify_sub));
        vthreads = 512;
        if (kn.verify_threads >= 0) vthreads = std::min(1024, std::max(64, (int)kn.verify_threads & ~63));
        if (!recs) { vthreads = 256; vblocks = 1024; v.chunk = 4; }  // re-hash fallback kernel: 4-wave blocks
        return PFQ_OK;
    }
    int tile_stage() {
        // LDS-tile certificates: every probe binned by (leaf chunk, 128 KiB filter tile), tiles tested out of LDS;
        // k_verify_rec then only sees the pairs that could not be binned
        // (thresholds < 1: entries name k-mers, tiles are half the size — pfq::TILE_LOG2_COUNTS)
        const uint32_t tile_log2 = block_mode ? pfq::TILE_LOG2_BLOCK : (counts_mode ? pfq::TILE_LOG2_COUNTS : pfq::TILE_LOG2);
        const uint32_t n_tiles = (uint32_t)((t.n_words * 64 + (1ull << tile_log2) - 1) >> tile_log2);
        const uint32_t chunk_log2 = pfq::CHUNK_PAIRS_LOG2;
        // Thresholds < 1: the tile passes leave the k-mers that are not contained in per-chunk miss bitmaps; k_verify_rec
        // only sees what could not be binned.  (PFQ_TILE_COUNTS=0: record kernel only.)  Results do not depend on the choice.
        bool tile_counts = true;
        if (kn.tile_counts >= 0) tile_counts = kn.tile_counts != 0;
        bool tile_mode = recs && (!counts_mode || tile_counts) && (block_mode || n_tiles < 256);
        if (kn.tile >= 0) tile_mode = tile_mode && kn.tile != 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = 0; }
        uint64_t tile_budget = std::min<uint64_t>(64ull << 30, (uint64_t)((double)(mem_free + t.d_entries.bytes()) * 0.8));
        if (kn.tile_gb >= 0) tile_budget = (uint64_t)kn.tile_gb << 30;
        t.last_tile_mode = 0;
        t.last_tile_bin = 0;
        t.last_tile_stream = false;
        t.last_entry_pack = false;
        if (tile_mode) {
            // every read may survive with one candidate: (bases - (k-1) per read) * hashes * 1.125 + slack per bucket
            const uint64_t max_chunks = nc + ((t.leaf_cap + t.guard_cap) >> chunk_log2) + 2;
            uint64_t want = (uint64_t)((double)total_bytes * t.num_hashes * 1.13 * std::max(1.0, t.pairs_per_read)) +
                            max_chunks * n_tiles * 544ull;
            if (want * 4 > tile_budget) want = tile_budget / 4;
            if (kn.tile_entries >= 0) want = std::max<uint64_t>(1, (uint64_t)kn.tile_entries);  // tests: force passes
            // thresholds < 1: one miss byte per k-mer of every pair the recent calls make expect (chunks that find no room
            // take the fallback), the rounds' positions, the pairs' positions
            // (block mode: 8 bytes per k-mer, one per leaf of the block; chunk offsets are in 16-byte units)
            uint64_t kmiss_cap = counts_mode ? std::min<uint64_t>(((uint64_t)((double)total_bytes * std::max(1.0, 1.3 * t.pairs_per_read)) + 16 * max_chunks + 64) * (block_mode ? 8u : 1u),
                                                                      block_mode ? (48ull << 30) : 0xfffffff0ull) & ~15ull : 0;
            if (counts_mode && kn.kmiss_bytes >= 0) kmiss_cap = std::min<uint64_t>(kmiss_cap, (uint64_t)kn.kmiss_bytes & ~15ull);
            bool ok = soft_ensure(t.d_entries, want) && soft_ensure(t.d_pair_chunk, t.d_pairs.n) && soft_ensure(t.d_flag_list, t.d_pairs.n) &&
                      soft_ensure(t.d_leaf_chunk0, nc + 1) && soft_ensure(t.d_chunks, max_chunks) && soft_ensure(t.d_gfill, max_chunks * n_tiles) && soft_ensure(t.d_binq, 256);
            if (ok && counts_mode)
                ok = soft_ensure(t.d_kmiss, kmiss_cap) && soft_ensure(t.d_round_k0, max_chunks * pfq::MAX_ROUNDS) &&
                     soft_ensure(t.d_n_rounds, max_chunks) && soft_ensure(t.d_pair_kpos, t.d_pairs.n);
            if (ok && counts_mode && block_mode) ok = soft_ensure(t.d_kall, (kmiss_cap >> 3) + 64);
            // Threshold 1 outside block mode: packed entries (pfq::PACK_PAIRS) where the format's limits cost nothing.  A round
            // of k_tile_bin takes KB k-mers; 16 pairs a round are no cap when a read has at least KB / 16 of them, and a chunk
            // of 1024 pairs stays under 256 rounds — a round is more than half full where reads are shorter than KB / 2 — when
            // 2 * 1024 * mean / KB + 2 <= 256.  (Beyond either bound results stay exact: shorter rounds, or the fallback.)
            bool pack = false;
            const uint32_t bin_shape = kn.bin_narrow > 0 ? (uint32_t)kn.bin_narrow : (kn.bin_wide > 0 ? 2u : 0u);
            if (ok && !counts_mode && !block_mode && kn.entry_pack != 0) {
                pfq::TileArgs shape{};
                shape.n_tiles = n_tiles;
                shape.bin_shape = bin_shape;
                const uint32_t build = pfq::tile_bin_build(shape);
                const uint64_t KB = pfq::tile_bin_kmer_budget(build >> 16, build & 0xffffu, n_tiles, t.num_hashes, false);
                const uint64_t kmers = total_bytes > n_reads * (t.kmer_size - 1) ? total_bytes - n_reads * (t.kmer_size - 1) : 0;
                pack = kn.entry_pack == 2 || (n_reads && kmers * pfq::PACK_PAIRS >= KB * n_reads &&
                                              (2ull << chunk_log2) * kmers + 2 * KB * n_reads <= pfq::PACK_ROUNDS * KB * n_reads);
                if (pack)
                    pack = soft_ensure(t.d_round_p0, max_chunks * pfq::PACK_ROUNDS) && soft_ensure(t.d_n_rounds, max_chunks) &&
                           soft_ensure(t.d_round_fail, max_chunks * pfq::PACK_ROUNDS * pfq::PACK_PAIRS);
            }
            if (!ok) {
                tile_mode = false;  // not enough HBM for the probe buckets: stay with the record kernel
            } else {
                HIP_TRY(hipMemsetAsync(t.d_gfill.p, 0, max_chunks * n_tiles * 4, st));
                HIP_TRY(hipMemsetAsync(t.d_binq.p, 0, 256 * 4, st));
                pfq::TileArgs ta{};
                ta.hp = t.hp;
                ta.bits = t.d_bits.p;
                ta.n_words = t.n_words;
                ta.chunk_log2 = chunk_log2;
                if (block_mode) {  // the "filter" of a bucket is its block's table: n_words * 64 bytes
                    ta.blocks = 1;
                    if (counts_mode) ta.kall = t.d_kall.p;  // (buckets by (block, mask); the passes' columns are the blocks)
                    ta.bits = reinterpret_cast<const uint64_t *>(t.d_T.p);
                    ta.n_words = t.n_words * 8;
                    ta.failb = t.d_failb.p;
                }
                ta.recs = recs;
                ta.meta = t.d_meta.p;
                ta.col_row = t.d_col_row.p;
                ta.bucket_off = off;
                ta.sub_log2 = sub_log2;
                ta.n_leaves = (uint32_t)(block_mode ? n_blocks : nc);  // (columns of the passes: blocks, whatever the buckets)
                ta.n_tiles = n_tiles;
                ta.chunks = t.d_chunks.p;
                ta.max_chunks = (uint32_t)max_chunks;
                ta.leaf_chunk0 = t.d_leaf_chunk0.p;
                ta.pair_chunk = t.d_pair_chunk.p;
                ta.n_chunks = t.cur_lo(CUR_CHUNKS_FLAGGED);
                ta.n_flagged = t.cur_hi(CUR_CHUNKS_FLAGGED);
                ta.flag_list = t.d_flag_list.p;
                ta.flag_cap = (uint32_t)std::min<uint64_t>(t.d_flag_list.n, 0xffffffffu);
                ta.entry_cursor = t.d_cursors.p + CUR_TILE_ENTRIES;
                // (a multiple of 32 entries: buckets then start on 128-byte boundaries, k_tile_test reads them 16 bytes at a time)
                ta.entry_cap = std::min<uint64_t>(want, t.d_entries.n) & ~31ull;  // (the buffer only grows; the budget of this call is `want`)
                ta.entries = t.d_entries.p;
                ta.gfill = t.d_gfill.p;
                ta.fail = t.d_fail.p;
                ta.n_pairs_ptr = off + nb;
                if (!counts_mode && !block_mode) {  // k_tile_test<0>: sparse columns' tiles come from their position slots
                    ta.tile_list_stats = t.d_cursors.p + CUR_TILE_LIST;
                    if (t.tile_list_cols && kn.tile_lists != 0) {
                        ta.tile_list_row = t.d_tile_list_row.p;
                        ta.tile_lists = t.d_tile_lists.p;
                        // the tree decides the build, once, with its layout: slots-only where no column has a dense tile
                        ta.tile_stream = t.tile_list_cols == t.n_cols && kn.tile_stream != 0;
                    }
                    if (pack) {
                        ta.entry_pack = 1;
                        ta.round_p0 = t.d_round_p0.p;
                        ta.round_fail = t.d_round_fail.p;
                        ta.n_rounds = t.d_n_rounds.p;
                        // (k_pack_fail walks the rounds of every chunk: none for a chunk that no launched pass binned)
                        HIP_TRY(hipMemsetAsync(t.d_n_rounds.p, 0, max_chunks * 4, st));
                    }
                }
                if (counts_mode) {
                    ta.counts = 1;
                    ta.threshold = threshold;
                    ta.kmiss = t.d_kmiss.p;
                    ta.kmiss_cap = kmiss_cap;
                    t.last_kmiss_cap = kmiss_cap;
                    ta.kmiss_used = t.d_cursors.p + CUR_KMISS;
                    ta.round_k0 = t.d_round_k0.p;
                    ta.n_rounds = t.d_n_rounds.p;
                    ta.pair_kpos = t.d_pair_kpos.p;
                    HIP_TRY(hipMemsetAsync(t.d_n_rounds.p, 0, max_chunks * 4, st));
                }
                int bin_blocks = 512, test_blocks = 512;
                if (kn.bin_blocks >= 0) bin_blocks = std::max(1, (int)kn.bin_blocks);
                if (kn.test_blocks >= 0) test_blocks = std::max(1, (int)kn.test_blocks);
                ta.bin_shape = bin_shape;
                ta.debug = kn.bin_debug > 0 ? (uint32_t)kn.bin_debug : 0u;
                pfq::launch_tile_plan(ta, st);
                // The probe buckets of all pairs may exceed the buffer (reads that pass many leaves): the plan
                // spreads the chunks over passes that reuse it.  Their number is known on the device only; as
                // many passes as the previous call needed are launched without waiting, and chunks of later
                // passes (if any) are certified by the record kernel below — exact either way.
                uint64_t n_passes = std::min<uint64_t>(std::max<uint64_t>(1, t.passes_hint), 256);  // (more: the record kernel takes the rest)
                if (block_mode) {  // the fallback of block mode is slow: wait for the plan and launch every pass it needs
                    HIP_TRY(hipMemcpyAsync(t.h_pair_cursor.p + HINT_PLAN, t.d_cursors.p + CUR_TILE_ENTRIES, 8, hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipStreamSynchronize(st));
                    n_passes = ta.entry_cap ? std::min<uint64_t>(std::max<uint64_t>(1, (t.h_pair_cursor.p[HINT_PLAN] + ta.entry_cap - 1) / ta.entry_cap), 256) : 1;
                }
                for (uint64_t p = 0; p < n_passes; ++p) {
                    ta.pass = (uint32_t)p;
                    ta.bin_queue = t.d_binq.p + p;
                    t.last_tile_bin = pfq::launch_tile_bin(ta, bin_blocks, st);
                    if (p == 0 && ev) HIP_TRY(hipEventRecord(ev[3], st));
                    pfq::launch_tile_test(ta, test_blocks, st);
                    t.last_tile_stream = ta.tile_stream != 0;
                }
                pfq::launch_pack_fail(ta, st);  // (packed entries: the failures of all passes become fail words)
                t.last_entry_pack = ta.entry_pack != 0;
                t.last_n_tiles = n_tiles;
                v.pair_chunk = t.d_pair_chunk.p;
                v.chunks = t.d_chunks.p;
                v.entry_cursor = t.d_cursors.p + CUR_TILE_ENTRIES;
                v.entry_cap = ta.entry_cap;
                v.launched_passes = (uint32_t)n_passes;
                if (pair_miss) {  // binned pairs whose prefix of k-mers leaves them undecided go to the record kernel
                    pfq::FinalizeArgs pf{};
                    pf.hp = t.hp;
                    pf.threshold = threshold;
                    pf.fail = t.d_fail.p;
                    binned_miss(pf, (uint32_t)n_passes);
                    pfq::launch_prefix_open(pf, t.d_meta.p, off + nb, t.d_fail.p, st);
                }
                t.hint_entry_cap = ta.entry_cap;
                t.last_passes = (uint32_t)std::max<uint64_t>(n_passes, 1);
                if (ev) HIP_TRY(hipEventRecord(ev[4], st));
                v.only_flagged = 1;
                v.n_flagged = ta.n_flagged;
                v.flag_list = t.d_flag_list.p;
                v.flag_cap = ta.flag_cap;
                t.last_tile_mode = 1;
            }
        }
        if (ev && !t.last_tile_mode) {
            HIP_TRY(hipEventRecord(ev[3], st));
            HIP_TRY(hipEventRecord(ev[4], st));
        }
        return PFQ_OK;
    }
    // thresholds < 1 after tile passes: the miss bits of the binned pairs are in their chunks' bitmaps
    void binned_miss(pfq::FinalizeArgs &f, uint32_t launched_passes) const {
        f.kmiss = t.d_kmiss.p;
        f.pair_kpos = t.d_pair_kpos.p;
        f.pair_chunk = t.d_pair_chunk.p;
        f.chunks = t.d_chunks.p;
        f.launched_passes = launched_passes;
    }
    // what k_finalize needs on either side: the sorted pairs, where hits and counts go
    pfq::FinalizeArgs finalize_args() const {
        pfq::FinalizeArgs f{};
        f.hp = t.hp;
        f.off = d_off;
        f.sorted = t.d_sorted.p;
        f.bucket_off = off;
        f.sub_log2 = sub_log2;
        f.threshold = threshold;
        f.counts = count_dst();
        f.hit_pairs = a.hit_pairs;
        f.hit_cap = hit_cap;
        f.hit_cursor = t.d_cursors.p + CUR_HIT;
        f.stats = t.d_stats.p;
        return f;
    }
    int finish_blocks() {
        // what the passes did not bin (overflows, no room, or no passes at all) is certified leaf by leaf against S
        a.S = t.d_S.p;
        a.col0 = 0;
        a.n_leaves = (uint32_t)std::min<size_t>(2048, nl);
        if (counts_mode && t.last_tile_mode) {  // the miss bytes of the binned pairs decide their candidates
            pfq::FinalizeArgs cf{};
            cf.hp = t.hp;
            cf.off = d_off;
            cf.sorted = t.d_sorted.p;
            cf.threshold = threshold;
            cf.fail = t.d_fail.p;
            cf.kall = t.d_kall.p;
            binned_miss(cf, v.launched_passes);
            pfq::launch_block_count(cf, off + nb, t.d_failb.p, st);
        }
        pfq::launch_block_fallback(a, t.d_sorted.p, off + nb, t.d_fail.p, t.d_failb.p, t.d_pair_chunk.p,
                                   t.last_tile_mode ? t.d_chunks.p : nullptr, v.launched_passes,
                                   t.last_tile_mode ? v.n_flagged : nullptr, t.last_tile_mode ? v.flag_list : nullptr, v.flag_cap, st);
        // ancestors that are not provably supersets must pass too (query.rs:119-141): the guards of every candidate
        // that is still standing
        if (with_guards) pfq::launch_block_guards(a, t.d_sorted.p, off + nb, t.d_failb.p, st);
        if (ev) HIP_TRY(hipEventRecord(ev[5], st));
        pfq::FinalizeArgs f = finalize_args();
        f.failb = t.d_failb.p;
        f.c0 = 0;
        f.c1 = (uint32_t)nc;
        pfq::launch_finalize(f, st);
        if (ev) HIP_TRY(hipEventRecord(ev[6], st));
        t.last_block_mode = 1;
        if (t.last_tile_mode) t.last_tile_mode = 2;
        t.hint_counts = false;
        return PFQ_OK;
    }
    int finish_pairs() {
        if (v.only_flagged == 1 && counts_mode) {
            // thresholds < 1: the list becomes every pair the tile passes left open (a k-mer missing, or not binned)
            unsigned int *n_open = t.cur_lo(CUR_OPEN);
            pfq::launch_collect_open(t.d_fail.p, off + nb, t.d_flag_list.p, v.flag_cap, n_open, st);
            v.n_flagged = n_open;
        }
        pfq::launch_verify(v, vblocks, vthreads, st);
        if (v.only_flagged == 1) {  // many flagged pairs (no room for their probe buckets): walk all pairs in leaf order instead
            v.only_flagged = 2;
            if (counts_mode) v.chunk = 8;  // (the walk pulls an item per 64 pairs, not per 8)
            pfq::launch_verify(v, vblocks, vthreads, st);
        }
        if (ev) HIP_TRY(hipEventRecord(ev[5], st));
        pfq::FinalizeArgs f = finalize_args();
        f.fail = t.d_fail.p;
        f.miss_words = v.miss_words;
        f.miss_pos = v.miss_pos;
        f.n_dirty = t.d_cursors.p + CUR_DIRTY;
        if (counts_mode && t.last_tile_mode) binned_miss(f, v.launched_passes);
        f.owner_sorted = with_guards ? t.d_owner_sorted.p : nullptr;
        f.gfail = with_guards ? t.d_gfail.p : nullptr;
        t.hint_counts = counts_mode;
        if (with_guards) {  // the guard columns first: a guard that does not pass marks its leaf pair
            f.c0 = (uint32_t)nl;
            f.c1 = (uint32_t)nc;
            f.guards = 1;
            pfq::launch_finalize(f, st);
        }
        f.c0 = 0;
        f.c1 = (uint32_t)nl;
        f.guards = 0;
        pfq::launch_finalize(f, st);
        if (ev) HIP_TRY(hipEventRecord(ev[6], st));
        return PFQ_OK;
    }

    // The hit pairs of this attempt, once the stream has drained.  done = false: the hit buffer was too small, run again.
    // Otherwise the call's results: fragments (pair_hits), the LCAs alone, or the per-read CSR for deliver_rows().
    int read_hits(bool &done) {
        done = true;
        HIP_TRY(hipStreamSynchronize(st));
        unsigned long long cursors[2] = {0, 0};  // CUR_HIT, CUR_PAIR
        if (deplete) {
            HIP_TRY(hipMemcpyAsync(cursors, t.d_cursors.p, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        } else HIP_TRY(hipMemcpy(cursors, t.d_cursors.p, 16, hipMemcpyDeviceToHost));
        const uint64_t n_pairs = cursors[CUR_HIT];
        if (n_reads) t.hits_per_read = std::max(t.hits_per_read, (double)n_pairs / (double)n_reads);
        if (t.last_attempts == 1) t.last_hit_cursor0 = n_pairs;
        if (n_pairs > hit_cap) {
            // restore the counters and run the block again with room for every hit (whatever PFQ_HIT_SLOTS says)
            if (nl && deplete) {
                HIP_TRY(hipMemcpyAsync(t.d_counts.p, t.d_counts_snapshot.p, nl * 8, hipMemcpyDeviceToDevice, st));
                HIP_TRY(hipStreamSynchronize(st));
            } else if (nl) HIP_TRY(hipMemcpy(t.d_counts.p, t.d_counts_snapshot.p, nl * 8, hipMemcpyDeviceToDevice));
            HIP_TRY(t.d_hit_pairs.ensure(n_pairs + 1024));
            hit_cap = t.d_hit_pairs.n;
            done = false;
            return PFQ_OK;
        }
        if (paired) return pair_hits(n_pairs);
        if (deplete) {  // reads: the flags straight from the hit pairs, nothing waited for
            pfq::launch_deplete_pairs(t.d_hit_pairs.p, n_pairs, n_reads, deplete_hit, st);
            HIP_TRY(hipGetLastError());
            return PFQ_OK;
        }
        if (!user_hits) {  // PFQ_WANT_LCA alone: the reads' spans straight from the hit pairs, nothing waited for
            if (n_reads && nl) {
                HIP_TRY(t.d_lca_span.ensure(n_reads));
                HIP_TRY(hipMemsetAsync(t.d_lca_span.p, 0xff, n_reads * sizeof(uint2), st));
                pfq::launch_lca_pairs(t.d_hit_pairs.p, n_pairs, t.d_allhit.p, n_reads, t.d_lca_span.p, lca_tables(), t.d_lca.p, st);
                HIP_TRY(hipGetLastError());
            }
            return PFQ_OK;
        }
        if (!n_reads) return deliver_rows(nullptr, nullptr, 0, 0, 0);
        // CSR read -> leaves (ascending; reads that pass every node list every leaf), built on the device from the unordered
        // hit pairs.  All-hit reads list every leaf, so the total is only known from the offsets: they are read back first.
        unsigned long long n_allhit = 0;
        HIP_TRY(hipMemcpy(&n_allhit, t.d_stats.p + pfq::ST_ALLHIT, 8, hipMemcpyDeviceToHost));
        PFQ_TRY(mate_csr(n_pairs, n_allhit != 0));
        uint64_t total = 0;
        PFQ_TRY(fetch_offsets(t.d_hit_off.p, n_reads, total));
        if (total) {
            HIP_TRY(t.d_hit_leaves.ensure(total));
            pfq::launch_hits_fill(t.d_hit_pairs.p, n_pairs, t.d_allhit.p, n_reads, t.d_hit_off.p, t.d_hit_cnt.p, t.d_hit_leaves.p, st);
            HIP_TRY(hipGetLastError());
        }
        rows_total = total;
        if (frames) return PFQ_OK;
        return deliver_rows(t.d_hit_off.p, t.d_hit_leaves.p, n_reads, total, 0);
    }

    // Offsets of the mates' (reads') CSR from the hit pairs, into d_hit_off; launch_hits_fill then scatters the leaves with
    // d_hit_cnt and leaves it zero.  any_allhit: all-hit reads list every leaf (else they stay flags in d_allhit).
    int mate_csr(uint64_t n_pairs, bool any_allhit) {
        HIP_TRY(t.d_hit_cnt.ensure(n_reads + 1));
        HIP_TRY(t.d_hit_off.ensure(n_reads + 2));
        HIP_TRY(t.d_hit_sums.ensure((n_reads + 4095) / 4096 + 2));
        HIP_TRY(hipMemsetAsync(t.d_hit_cnt.p, 0, (n_reads + 1) * 4, st));
        if (paired) HIP_TRY(hipMemsetAsync(t.d_pair_misc.p, 0, 16, st));  // (pair_hits' two words, cleared where they always were)
        pfq::launch_hits_csr(t.d_hit_pairs.p, n_pairs, t.d_allhit.p, n_reads, (uint32_t)nl, any_allhit, t.d_hit_cnt.p, t.d_hit_sums.p, t.d_hit_off.p, st);
        HIP_TRY(hipGetLastError());
        return PFQ_OK;
    }
    // the offsets of a CSR into the caller's page-locked copy, waited for: total = its number of entries
    int fetch_offsets(const unsigned long long *off, uint64_t n_units, uint64_t &total) {
        HIP_TRY(t.h_hit_off.ensure(n_units + 1));
        HIP_TRY(hipMemcpyAsync(t.h_hit_off.p, off, (n_units + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        total = t.h_hit_off.p[n_units];
        return PFQ_OK;
    }

    // PFQ_PAIRED, after the mates' hit pairs are complete: the mate CSR (all-hit mates as flags only), the fragment CSR
    // (union / intersection per fragment) and its histogram into the tree's counters; PFQ_WANT_HITS: deliver_rows().
    // Without PFQ_WANT_HITS nothing more is waited for: every all-leaf fragment is a count, the lists hold at most the
    // mates' n_pairs entries (a union holds at most both mates' entries).
    int pair_hits(uint64_t n_pairs) {
        const uint64_t n_frag = n_reads / 2;
        const int pair_mode = pair_both ? 2 : 1;
        if (!n_frag || !nl) return user_hits ? deliver_rows(nullptr, nullptr, n_frag, 0, pair_mode) : PFQ_OK;
        HIP_TRY(t.d_hit_leaves.ensure(n_pairs + 1));
        HIP_TRY(t.d_frag_off.ensure(n_frag + 2));
        HIP_TRY(t.d_pair_long.ensure(n_frag + 1));
        HIP_TRY(t.d_pair_misc.ensure(2));
        PFQ_TRY(mate_csr(n_pairs, false));
        pfq::launch_hits_fill(t.d_hit_pairs.p, n_pairs, t.d_allhit.p, n_reads, t.d_hit_off.p, t.d_hit_cnt.p, t.d_hit_leaves.p, st);
        // (the scatter leaves d_hit_cnt zero: it holds the fragments' counts next)
        pfq::launch_pair_combine(t.d_hit_off.p, t.d_hit_leaves.p, t.d_allhit.p, n_frag, pair_both, (uint32_t)nl, user_hits, t.d_hit_cnt.p,
                                 t.d_pair_long.p, t.d_pair_misc.p, t.d_hit_sums.p, t.d_frag_off.p, st);
        HIP_TRY(hipGetLastError());
        uint64_t total = 0;
        if (user_hits) PFQ_TRY(fetch_offsets(t.d_frag_off.p, n_frag, total));
        const uint64_t room = user_hits ? total : n_pairs;
        HIP_TRY(t.d_frag_leaves.ensure(room + 1));
        pfq::launch_pair_fill(t.d_hit_off.p, t.d_hit_leaves.p, t.d_allhit.p, n_frag, pair_both, (uint32_t)nl, t.d_pair_long.p, t.d_pair_misc.p,
                              t.d_frag_off.p, t.d_frag_leaves.p, st);
        pfq::launch_pair_leaf_counts(t.d_frag_leaves.p, t.d_frag_off.p + n_frag, t.d_pair_misc.p, (uint32_t)nl, room, t.d_counts.p, st);
        HIP_TRY(hipGetLastError());
        if (user_hits) return deliver_rows(t.d_frag_off.p, t.d_frag_leaves.p, n_frag, total, pair_mode);
        if (want_lca) PFQ_TRY(lca_rows(t.d_frag_off.p, t.d_frag_leaves.p, n_frag, pair_mode));
        return PFQ_OK;
    }

    // PFQ_WANT_HITS: the call's final CSR (off / leaves in device memory, `total` entries over n_units rows, the offsets
    // already in h_hit_off; off == nullptr: no row was built, every list is empty) goes to the caller, with everything that
    // is derived from it: scores (reads: pair_mode 0, fragments: 1 either / 2 both), LCAs, the abundance log.  The scores
    // are queued before the LCAs (PFQ_LCA_BEST reads d_hit_scores), the LCAs run beside the copies, and the log is appended
    // once the copies have been waited for.  Host waits of a call that builds hit pairs (PFQ_PAIRED, PFQ_WANT_LCA alone included):
    //   every such call             1 wait and the 16-byte cursor read (read_hits)
    //   reads, PFQ_WANT_HITS        + the 8-byte read of ST_ALLHIT, 1 wait for the offsets (fetch_offsets), 1 for the lists (here)
    //   fragments, PFQ_WANT_HITS    + 1 wait for the fragment offsets (fetch_offsets), 1 for the lists (here)
    //   fragments without it, PFQ_WANT_LCA alone: nothing more;  PFQ_WANT_ABUNDANCE: + 1, in abund_append
    int deliver_rows(const unsigned long long *off, const uint32_t *leaves, uint64_t n_units, uint64_t total, int pair_mode) {
        if (!off) {  // offsets[0 .. n_units] are always written
            HIP_TRY(t.h_hit_off.ensure(n_units + 1));
            std::fill_n(t.h_hit_off.p, n_units + 1, 0);
        }
        HIP_TRY(t.h_hit_leaves.ensure(total + 1));  // (empty lists still get a buffer)
        if (want_scores) HIP_TRY(t.h_hit_scores.ensure(total + 1));
        if (total) {
            HIP_TRY(hipMemcpyAsync(t.h_hit_leaves.p, leaves, total * 4, hipMemcpyDeviceToHost, st));
            if (want_scores) {  // the hit set is final: score every (unit, listed leaf) pair of the CSR
                HIP_TRY(t.d_hit_scores.ensure(total));
                if (pair_mode) pfq::launch_pair_scores(t.hp, d_seq, d_off, n_units, threshold, pair_both, off, leaves, t.d_col_row.p, t.d_bits.p, t.n_words, t.d_hit_scores.p, st);
                else pfq::launch_hit_scores(t.hp, d_seq, d_off, n_units, threshold, off, leaves, t.d_col_row.p, t.d_bits.p, t.n_words, t.d_hit_scores.p, st);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(t.h_hit_scores.p, t.d_hit_scores.p, total * 4, hipMemcpyDeviceToHost, st));
            }
        }
        if (want_lca && off) PFQ_TRY(lca_rows(off, leaves, n_units, pair_mode));
        // PFQ_ROWS_BEST: the three consumers below read the best rows; everything above and the caller's copies keep the call's own
        const unsigned long long *use_off = off;
        const uint32_t *use_leaves = leaves;
        if (rows_best) {
            PFQ_TRY(best_rows(off, leaves, n_units, total));
            if (off) {
                use_off = t.d_best_off.p;
                use_leaves = t.d_best_leaves.p;
            }
        }
        if (want_sweep) PFQ_TRY(sweep_rows(off, leaves, n_units));  // (the whole rows, whatever PFQ_ROWS_BEST says)
        if (want_cover) PFQ_TRY(cover_sketch(use_off, use_leaves, n_units, total, pair_mode));
        if (want_taxa && off) PFQ_TRY(tax_rows(use_off, use_leaves, n_units));
        if (total) HIP_TRY(hipStreamSynchronize(st));
        if (want_scores) {
            t.scores_valid = true;
            t.scores_n = total;
        }
        hits->n_reads = n_units;
        hits->offsets = t.h_hit_off.p;
        hits->leaves = t.h_hit_leaves.p;
        return want_abund ? abund_append(use_off, use_leaves, n_units) : PFQ_OK;
    }

    // PFQ_ROWS_BEST: the rows of the call's final CSR reduced to their best-scoring entries (pfq.h "best rows"), once:
    // deliver_rows() runs for the attempt that stands.  Queued behind the score kernel (check_flags has made sure of the scores;
    // fragments: launch_pair_scores' sums); `total` bounds what the reduction can keep, so nothing is read back.  No row built:
    // every best row is empty and nothing runs.
    int best_rows(const unsigned long long *off, const uint32_t *leaves, uint64_t n_units, uint64_t total) {
        t.best_units = n_units;
        t.best_built = off != nullptr && n_units != 0;
        if (!t.best_built) return PFQ_OK;
        HIP_TRY(t.d_best_cnt.ensure(n_units));
        HIP_TRY(t.d_best_sums.ensure((n_units + 4095) / 4096 + 2));
        HIP_TRY(t.d_best_long.ensure(n_units));
        HIP_TRY(t.d_best_cur.ensure(1));
        HIP_TRY(t.d_best_off.ensure(n_units + 1));
        HIP_TRY(t.d_best_leaves.ensure(total + 1));
        HIP_TRY(hipMemsetAsync(t.d_best_cur.p, 0, 8, st));
        pfq::launch_best_rows(off, leaves, t.d_hit_scores.p, n_units, t.d_best_cnt.p, t.d_best_sums.p, t.d_best_long.p, t.d_best_cur.p,
                              t.d_best_off.p, t.d_best_leaves.p, st);
        HIP_TRY(hipGetLastError());
        return PFQ_OK;
    }

    // PFQ_WANT_SWEEP: the rows of the call's final CSR and their scores are counted against the tree's threshold list (pfq.h
    // "threshold sweep"), once: deliver_rows() runs for the attempt that stands.  Queued behind the score kernel (check_flags has
    // made sure of the scores and of reads, not fragments) and before deliver_rows' wait, which so covers the kernels' reads of
    // d_off.  No row built: the units have empty rows and are counted in sw_units alone.
    int sweep_rows(const unsigned long long *off, const uint32_t *leaves, uint64_t n_units) {
        t.sw_units += n_units;
        if (!off || !n_units) return PFQ_OK;
        HIP_TRY(t.d_sw_long.ensure(n_units));
        HIP_TRY(t.d_sw_cur.ensure(1));
        HIP_TRY(hipMemsetAsync(t.d_sw_cur.p, 0, 8, st));
        const size_t n_thr = t.sw_thr.size();
        pfq::SweepArgs a{};
        a.off = off;
        a.leaves = leaves;
        a.scores = t.d_hit_scores.p;
        a.read_off = d_off;
        a.n_units = n_units;
        a.k = t.hp.k;
        a.n_thr = (uint32_t)n_thr;
        a.n_leaves = (uint32_t)nl;
        std::copy(t.sw_thr.begin(), t.sw_thr.end(), a.thr);
        a.pass = t.d_sw_state.p;
        a.uniq = a.pass + (n_thr + 1) * nl;
        a.tops = a.uniq + n_thr * nl;
        a.long_list = t.d_sw_long.p;
        a.n_long = t.d_sw_cur.p;
        pfq::launch_sweep(a, kn.sweep_lds != 0, st);
        HIP_TRY(hipGetLastError());
        return PFQ_OK;
    }

    // PFQ_WANT_COVERAGE: the rows of the call's final CSR are sketched, once: deliver_rows() runs for the attempt that stands.
    // Queued behind the scores and before deliver_rows' wait, which so covers the kernel's reads of d_seq (the caller's own
    // buffer in pfq_query_batch_device).  Rows without entries add nothing to any leaf.
    int cover_sketch(const unsigned long long *off, const uint32_t *leaves, uint64_t n_units, uint64_t total, int pair_mode) {
        t.cov_units += n_units;
        if (!off || !total || !t.d_cov_regs.p) return PFQ_OK;
        const pfq::CoverArgs cv{t.d_cov_regs.p, t.d_cov_cnt.p, t.d_cov_cnt.p + nl, (uint32_t)nl, t.cov_p};
        const uint32_t blocks = kn.cover_blocks > 0 ? (uint32_t)std::min<long long>(kn.cover_blocks, 65535) : 0;
        pfq::launch_cover_sketch(t.hp, d_seq, d_off, n_units, threshold, pair_mode, off, leaves, t.d_col_row.p, t.d_bits.p, t.n_words, cv, blocks, st);
        HIP_TRY(hipGetLastError());
        return PFQ_OK;
    }

    // PFQ_WANT_TAXA: the rows of the call's final CSR are counted on the taxonomy's nodes, once: deliver_rows() runs for the attempt
    // that stands.  Queued before deliver_rows' wait; rows without entries count nowhere (d_tax_node keeps PFQ_NO_CLADE).
    int tax_rows(const unsigned long long *off, const uint32_t *leaves, uint64_t n_units) {
        if (!n_units) return PFQ_OK;
        HIP_TRY(t.d_tax_long.ensure(n_units));
        HIP_TRY(t.d_tax_cur.ensure(1));
        HIP_TRY(hipMemsetAsync(t.d_tax_cur.p, 0, 8, st));
        pfq::TaxTables tb{};
        tb.n_leaves = (uint32_t)nl;
        tb.n_nodes = (uint32_t)t.tax.nodes.size();
        tb.top_node = t.tax.top;
        for (uint32_t k = 0; k < pfq::TAX_HOT; ++k) tb.hot[k] = t.tax_hot[k];
        tb.rank = t.d_tax_rank.p;
        tb.leaf_node = t.d_tax_leaf_node.p;
        tb.parent = t.d_tax_parent.p;
        tb.first_rank = t.d_tax_first.p;
        tb.gap_min = t.d_tax_gap_min.p;
        tb.here = t.d_tax_here.p;
        tb.any = t.d_tax_any.p;
        tb.misc = t.d_tax_misc.p;
        pfq::launch_tax_rows(off, leaves, n_units, tb, t.d_tax_node.p, t.d_tax_long.p, t.d_tax_cur.p, st);
        HIP_TRY(hipGetLastError());
        return PFQ_OK;
    }

    // PFQ_WANT_ABUNDANCE: the rows of the call's final CSR (off / leaves, in device memory) go into the log, device to device.
    // k_abund_count first says what they add; the host reads those five words (the one wait the flag costs), makes exactly
    // that much room and appends.  The stream is otherwise idle here: PFQ_WANT_HITS has waited for the copies.  Rows that do
    // not fit: PFQ_ERR_UNSUPPORTED, the call's other results stand (they are complete by now) and the log keeps what it held.
    int abund_append(const unsigned long long *off, const uint32_t *leaves, uint64_t n_units) {
        if (!n_units) return PFQ_OK;
        HIP_TRY(t.d_ab_cur.ensure(2 + pfq::ABUND_CNT_N));
        unsigned long long *d_cnt = t.d_ab_cur.p + 2, c[pfq::ABUND_CNT_N];
        HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof c, st));
        pfq::launch_abund_count(off, n_units, (uint32_t)nl, d_cnt, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c, d_cnt, sizeof c, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint64_t unhit = c[pfq::ABUND_CNT_UNHIT], uniq = c[pfq::ABUND_CNT_UNIQUE], all = c[pfq::ABUND_CNT_ALL], rows = c[pfq::ABUND_CNT_ROWS],
                       entries = c[pfq::ABUND_CNT_ENTRIES];
        std::string why = abund_refusal(t, n_units, entries);
        bool ok = true;
        if (why.empty()) {
            PFQ_TRY(abund_room(t, rows, entries, ok));
            if (!ok) why = "no device memory for " + std::to_string(rows) + " more rows with " + std::to_string(entries) + " leaf entries";
        }
        if (!why.empty()) {
            t.ab_incomplete = true;
            results_stand = true;
            return fail(PFQ_ERR_UNSUPPORTED, "abundance log: " + why + ": this call's units were not logged (its other results stand); "
                                             "pfq_abundance_reset starts a new log");
        }
        const unsigned long long cur[2] = {t.ab_rows, t.ab_entries};
        HIP_TRY(hipMemcpy(t.d_ab_cur.p, cur, sizeof cur, hipMemcpyHostToDevice));
        pfq::AbundLog g{t.d_ab_start.p, t.d_ab_len.p, t.d_ab_entries.p, t.d_ab_cur.p, t.d_ab_unique.p, t.ab_rows + rows, t.ab_entries + entries};
        pfq::launch_abund_append(off, leaves, n_units, (uint32_t)nl, g, st);
        HIP_TRY(hipGetLastError());
        t.ab_rows += rows;
        t.ab_entries += entries;
        t.ab_units += n_units;
        t.ab_unhit += unhit;
        t.ab_unique += uniq;
        t.ab_all += all;
        return PFQ_OK;
    }

    pfq::LcaTables lca_tables() const {
        return pfq::LcaTables{(uint32_t)nl, (uint32_t)t.clades.size(), t.top_clade, t.d_leaf_clade.p, t.d_gap_min.p, t.d_clade_here.p};
    }
    // PFQ_WANT_LCA over the rows of the CSR the call has built (reads, or fragments: pair_mode 1 either / 2 both, whose all-leaf
    // fragments may be unlisted); PFQ_LCA_BEST: over the entries with the row's highest score (the scores are queued before)
    int lca_rows(const unsigned long long *off, const uint32_t *leaves, uint64_t n_units, int pair_mode) {
        if (lca_best) {
            HIP_TRY(t.d_lca_span.ensure(n_units));
            HIP_TRY(t.d_lca_long.ensure(n_units));
            HIP_TRY(t.d_lca_misc.ensure(1));
            HIP_TRY(hipMemsetAsync(t.d_lca_misc.p, 0, 8, st));
            pfq::launch_lca_best(off, leaves, t.d_hit_scores.p, n_units, t.d_lca_span.p, t.d_lca_long.p, t.d_lca_misc.p, lca_tables(), t.d_lca.p, st);
        } else pfq::launch_lca_rows(off, leaves, n_units, t.d_allhit.p, pair_mode, lca_tables(), t.d_lca.p, st);
        HIP_TRY(hipGetLastError());
        return PFQ_OK;
    }

    int run() {
        if (want_lca) {
            t.lca_units = paired ? n_reads / 2 : n_reads;
            HIP_TRY(t.d_lca.ensure(t.lca_units + 1));
            HIP_TRY(hipMemsetAsync(t.d_lca.p, 0xff, t.lca_units * 4, st));  // (an empty tree or call: no unit has a clade)
        }
        if (want_taxa) {
            t.taxa_units = paired ? n_reads / 2 : n_reads;
            HIP_TRY(t.d_tax_node.ensure(t.taxa_units + 1));
            HIP_TRY(hipMemsetAsync(t.d_tax_node.p, 0xff, t.taxa_units * 4, st));  // (a unit without a hit has no node)
        }
        for (int attempt_no = 0; attempt_no < 2; ++attempt_no) {
            PFQ_TRY(attempt(attempt_no));
            if (!want_hits) return PFQ_OK;  // (PFQ_PAIRED always builds the mates' hit lists)
            bool done = false;
            PFQ_TRY(read_hits(done));
            if (done) return PFQ_OK;
        }
        return fail(PFQ_ERR_DEVICE, "hit buffer overflow persisted");
    }
};

int query_device(pfq_tree &t, const uint8_t *d_seq, const uint64_t *d_off, uint64_t n_reads, uint64_t total_bytes,
                 float threshold, uint32_t flags, hipStream_t st, pfq_hits *hits, bool deplete = false, uint32_t *deplete_hit = nullptr) {
    t.fm_rows = false;
    t.scores_valid = false;
    t.lca_last = false;
    t.taxa_last = false;
    t.best_last = false;
    QueryRun q(t, d_seq, d_off, n_reads, total_bytes, threshold, flags, st, hits);
    q.deplete = deplete;
    q.deplete_hit = deplete_hit;
    int rc = q.plan();
    if (rc == PFQ_OK) rc = q.run();
    t.lca_last = (rc == PFQ_OK || q.results_stand) && (flags & PFQ_WANT_LCA);
    t.taxa_last = (rc == PFQ_OK || q.results_stand) && (flags & PFQ_WANT_TAXA);
    t.best_last = (rc == PFQ_OK || q.results_stand) && (flags & PFQ_ROWS_BEST);
    if (t.last_done && t.have_last_stream && t.last_stream == st) HIP_TRY(hipEventRecord(t.last_done, st));  // (what waits for this call)
    return rc;
}
// What every pfq_debug_last_*_ms does: the intervals between a timer's events, where the call that recorded them has stood
// (`also`: what else the getter asks of the tree); else PFQ_ERR_STATE with `refusal`.
template <int N>
int last_stage_ms(pfq_tree *tree, double *ms, StageTimes<N> pfq_tree::*timer, bool also, const char *refusal) {
    if (!tree || !ms) return fail(PFQ_ERR_ARG, "null argument");
    if (!also || !(tree->*timer).valid) return fail(PFQ_ERR_STATE, refusal);
    PFQ_TRY(use_device(tree->device));
    HIP_TRY((tree->*timer).read(ms));
    return PFQ_OK;
}

// Waits for the last query call's work (its stream may since have been destroyed by the caller).
int wait_last_call(pfq_tree &t) {
    if (t.last_done) HIP_TRY(hipEventSynchronize(t.last_done));
    return PFQ_OK;
}

// ---- pfq_query_frames (pfq.h "frames and segments") ----
static_assert(sizeof(pfq::Segment) == sizeof(pfq_segment) && sizeof(pfq_segment) == 40, "the kernels write pfq_segment");
uint32_t frame_piece(const Knobs &k) {
    return k.frame_piece > 0 && k.frame_piece % 64 == 0 && k.frame_piece <= (1ll << 30) ? (uint32_t)k.frame_piece : pfq::FRAME_PIECE_DEFAULT;
}
// a few words of the device read on the host, waited for
int fetch_words(unsigned long long *dst, const unsigned long long *d_src, size_t n, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(dst, d_src, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PFQ_OK;
}
// One pfq_query_frames[_device] call, everything queued on `st` and waited for: the frame table and the frames' bytes; the
// frames classified as a block of reads by QueryRun (hit lists, overflow retry) into the count sink; then, from the rows it
// leaves on the device, the segments, the sequences' leaf counts — the only writes to the tree's counters — and the
// refinement.  Host waits beyond QueryRun's: the number of frames, of segments, of pieces (they size buffers), the results.
int query_frames_device(pfq_tree &t, const uint8_t *d_seq, const uint64_t *d_off, uint64_t n_seqs, uint32_t F, uint32_t S, float threshold,
                        hipStream_t st, pfq_segments *out) {
    if (F < t.kmer_size || S < 1 || S > F)
        return fail(PFQ_ERR_ARG, "pfq_query_frames: frame = " + std::to_string(F) + ", step = " + std::to_string(S) + " (need k = " +
                                     std::to_string(t.kmer_size) + " <= frame and 1 <= step <= frame)");
    if (t.root < 0) return fail(PFQ_ERR_STATE, "query on an empty tree");
    PFQ_TRY(build_layout(t));
    HIP_TRY(t.h_fr_off.ensure(n_seqs + 1));
    HIP_TRY(t.h_fr_segs.ensure(1));
    out->n_seqs = n_seqs;
    out->n_frames = 0;
    out->offsets = t.h_fr_off.p;
    out->seg = t.h_fr_segs.p;
    t.h_fr_off.p[0] = 0;
    if (!n_seqs) return PFQ_OK;
    // (the scratch is reused call after call: as in QueryRun::plan, a call on another stream waits for the last one)
    HIP_TRY(t.last_done.ensure(hipEventDisableTiming));
    if (t.have_last_stream && t.last_stream != st) HIP_TRY(hipEventSynchronize(t.last_done));
    t.last_stream = st;
    t.have_last_stream = true;
    if (n_seqs >= 0xffffffffull) return fail(PFQ_ERR_UNSUPPORTED, "pfq_query_frames: 2^32 - 1 frames or more in one call (every sequence has a frame)");
    const size_t nl = t.leaves.size();
    // ---- frames per sequence, their scan, the table and the cut
    HIP_TRY(t.d_fr_cnt.ensure(n_seqs + 1));
    HIP_TRY(t.d_fr_def.ensure(n_seqs + 1));
    HIP_TRY(t.d_fr_seq0.ensure(n_seqs + 2));
    HIP_TRY(t.d_fr_defoff.ensure(n_seqs + 2));
    HIP_TRY(t.d_fr_seqseg.ensure(n_seqs + 2));
    HIP_TRY(t.d_fr_sums.ensure((n_seqs + 4095) / 4096 + 2));
    HIP_TRY(t.d_fr_misc.ensure(4));  // [0] a sequence is too long, [1] segments queued for k_seg_walk, [2..3] totals on their way to the host
    HIP_TRY(hipMemsetAsync(t.d_fr_misc.p, 0, 4 * 8, st));
    pfq::launch_frame_count(d_off, n_seqs, F, S, t.d_fr_cnt.p, t.d_fr_def.p, t.d_fr_misc.p, st);
    pfq::launch_scan_u32(t.d_fr_cnt.p, n_seqs, t.d_fr_sums.p, t.d_fr_seq0.p, st);
    pfq::launch_scan_u32(t.d_fr_def.p, n_seqs, t.d_fr_sums.p, t.d_fr_defoff.p, st);
    HIP_TRY(hipGetLastError());
    unsigned long long w[2] = {0, 0}, too_long = 0;
    HIP_TRY(hipMemcpyAsync(&w[0], t.d_fr_seq0.p + n_seqs, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&w[1], t.d_fr_defoff.p + n_seqs, 8, hipMemcpyDeviceToHost, st));
    PFQ_TRY(fetch_words(&too_long, t.d_fr_misc.p, 1, st));
    if (too_long) return fail(PFQ_ERR_UNSUPPORTED, "pfq_query_frames: a sequence of 2^32 bases or more (or offsets that do not ascend); nothing was counted");
    const uint64_t n_frames = w[0], bytes = (uint64_t)F * n_frames - w[1];
    // (QueryRun takes fewer than 2^31 - 1024 reads a block: that is the limit in force, below the 2^32 - 1 of the frame table)
    if (n_frames >= (1ull << 31) - 1024)
        return fail(PFQ_ERR_UNSUPPORTED, "pfq_query_frames: " + std::to_string(n_frames) + " frames in one call (the limit is 2^31 - 1024: a smaller step "
                                         "or longer sequences need several calls); nothing was counted");
    if (!(soft_ensure(t.d_fr_bytes, bytes + 64) && soft_ensure(t.d_fr_foff, n_frames + 2) && soft_ensure(t.d_fr_seq, n_frames + 1) &&
          soft_ensure(t.d_fr_start, n_frames + 1) && soft_ensure(t.d_fr_segpos, n_frames + 2) && soft_ensure(t.d_fr_cnt, n_frames + 1) &&
          soft_ensure(t.d_fr_sums, (n_frames + 4095) / 4096 + 2)))
        return fail(PFQ_ERR_UNSUPPORTED, "pfq_query_frames: no device memory for the frame bytes (" + std::to_string(bytes) + " bytes in " +
                                         std::to_string(n_frames) + " frames: the input times frame / step); nothing was counted");
    out->n_frames = n_frames;
    pfq::FrameArgs fa{d_off, n_seqs, n_frames, F, S, t.d_fr_seq0.p, t.d_fr_defoff.p, t.d_fr_seq.p, t.d_fr_start.p, t.d_fr_foff.p};
    pfq::launch_frame_cut(fa, d_seq, t.d_fr_bytes.p, st);
    HIP_TRY(hipGetLastError());
    // ---- the frames, classified like reads
    pfq_hits unused{};
    QueryRun q(t, t.d_fr_bytes.p, t.d_fr_foff.p, n_frames, bytes, threshold, PFQ_WANT_HITS, st, &unused);
    q.frames = true;
    PFQ_TRY(q.plan());
    PFQ_TRY(q.run());
    // ---- segments from the ascending rows (t.d_hit_off / t.d_hit_leaves)
    pfq::SegArgs sa{};
    sa.row_off = t.d_hit_off.p;
    sa.row_leaves = t.d_hit_leaves.p;
    sa.n_frames = n_frames;
    sa.n_leaves = (uint32_t)nl;
    sa.frame_seq = t.d_fr_seq.p;
    sa.frame_start = t.d_fr_start.p;
    sa.frame_off = t.d_fr_foff.p;
    sa.seq_frame0 = t.d_fr_seq0.p;
    sa.open_cnt = t.d_fr_cnt.p;
    sa.seg_pos = t.d_fr_segpos.p;
    sa.n_queued = t.d_fr_misc.p + 1;
    sa.counts = t.d_counts.p;
    uint64_t n_segs = 0;
    if (q.rows_total) {
        pfq::launch_seg_count(sa, st);
        pfq::launch_scan_u32(t.d_fr_cnt.p, n_frames, t.d_fr_sums.p, t.d_fr_segpos.p, st);
        pfq::launch_seq_seg_off(t.d_fr_seq0.p, t.d_fr_segpos.p, n_seqs, t.d_fr_seqseg.p, st);
        HIP_TRY(hipGetLastError());
        unsigned long long ns = 0;
        PFQ_TRY(fetch_words(&ns, t.d_fr_segpos.p + n_frames, 1, st));
        n_segs = ns;
    }
    if (!n_segs) {
        std::fill_n(t.h_fr_off.p, n_seqs + 1, 0);
        return PFQ_OK;
    }
    if (n_segs >= 0xffffffffull) return fail(PFQ_ERR_UNSUPPORTED, "pfq_query_frames: 2^32 - 1 segments or more in one call; nothing was counted");
    HIP_TRY(t.d_fr_segs.ensure(n_segs + 1));
    HIP_TRY(t.d_fr_segseq.ensure(n_segs + 1));
    HIP_TRY(t.d_fr_queue.ensure(n_segs + 1));
    HIP_TRY(t.d_fr_cnt.ensure(std::max<uint64_t>(n_segs, n_frames) + 1));  // (may drop the open counts: they are scanned by now)
    HIP_TRY(t.d_fr_pieceoff.ensure(n_segs + 2));
    HIP_TRY(t.d_fr_sums.ensure((n_segs + 4095) / 4096 + 2));
    HIP_TRY(t.h_fr_segs.ensure(n_segs));
    sa.open_cnt = t.d_fr_cnt.p;
    sa.seg = t.d_fr_segs.p;
    sa.seg_seq = t.d_fr_segseq.p;
    sa.queue = t.d_fr_queue.p;
    pfq::launch_seg_fill(sa, t.d_fr_seqseg.p, n_seqs, n_segs, st);
    // ---- refinement: pieces of the segments' k-mer positions, probed on the sequences themselves
    const uint32_t piece = frame_piece(t.knobs);
    pfq::launch_piece_count(t.d_fr_segs.p, n_segs, t.hp.k, piece, t.d_fr_cnt.p, st);
    pfq::launch_scan_u32(t.d_fr_cnt.p, n_segs, t.d_fr_sums.p, t.d_fr_pieceoff.p, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(t.h_fr_off.p, t.d_fr_seqseg.p, (n_seqs + 1) * 8, hipMemcpyDeviceToHost, st));
    unsigned long long n_pieces = 0;
    PFQ_TRY(fetch_words(&n_pieces, t.d_fr_pieceoff.p + n_segs, 1, st));
    HIP_TRY(t.d_fr_parts.ensure(n_pieces + 1));
    pfq::launch_seg_refine(t.hp, d_seq, d_off, t.d_fr_segs.p, t.d_fr_segseq.p, t.d_fr_pieceoff.p, n_segs, n_pieces, piece, t.d_col_row.p, t.d_bits.p,
                           t.n_words, t.d_fr_parts.p, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(t.h_fr_segs.p, t.d_fr_segs.p, n_segs * sizeof(pfq_segment), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->offsets = t.h_fr_off.p;
    out->seg = t.h_fr_segs.p;
    return PFQ_OK;
}

// The subtree shards of a tree: its depth-`depth` frontier, left to right — nodes at that depth and leaves above it
// (pfq_tree_open_subtree, pfq_db_shard_count).  Needs depth of every node.
std::vector<int32_t> shard_frontier(const pfq_tree &t, uint64_t depth) {
    std::vector<int32_t> frontier;
    if (t.root < 0) return frontier;
    std::vector<int32_t> st{t.root};
    while (!st.empty()) {
        int32_t v = st.back();
        st.pop_back();
        const Node &nd = t.nodes[v];
        if (nd.depth == depth || nd.is_leaf()) { frontier.push_back(v); continue; }
        if (nd.right >= 0) st.push_back(nd.right);
        if (nd.left >= 0) st.push_back(nd.left);
    }
    return frontier;
}

// Reduce a whole tree to subtree shard `index` of the depth-`depth` frontier (pfq_tree_open_subtree): the shard's node,
// everything below it and the chain of its ancestors, each reduced to the child on the path.  `reachable` marks the nodes
// that stay; `chain` lists the ancestors, root first.  Needs parent / depth of every node (relink).
int apply_shard(pfq_tree &t, uint64_t depth, uint64_t index, std::vector<uint8_t> &reachable, std::vector<int32_t> &chain) {
    if (t.root < 0) return fail(PFQ_ERR_STATE, "subtree shard of an empty tree");
    const std::vector<int32_t> frontier = shard_frontier(t, depth);
    if (index >= frontier.size())
        return fail(PFQ_ERR_ARG, "subtree index " + std::to_string(index) + " out of range: the depth-" +
                                     std::to_string(depth) + " frontier has " + std::to_string(frontier.size()) + " nodes");
    const int32_t target = frontier[index];
    // leaves before the shard in the whole tree's order
    auto count_leaves = [&](int32_t root) {
        uint64_t n = 0;
        std::vector<int32_t> s2{root};
        while (!s2.empty()) {
            int32_t v = s2.back();
            s2.pop_back();
            const Node &nd = t.nodes[v];
            if (nd.is_leaf()) ++n;
            if (nd.left >= 0) s2.push_back(nd.left);
            if (nd.right >= 0) s2.push_back(nd.right);
        }
        return n;
    };
    t.shard_first_leaf = 0;
    for (uint64_t i = 0; i < index; ++i) t.shard_first_leaf += count_leaves(frontier[i]);
    // reduce every ancestor to the child on the path
    chain.clear();
    for (int32_t c = target, v = t.nodes[target].parent; v >= 0; c = v, v = t.nodes[v].parent) {
        if (t.nodes[v].left != c) t.nodes[v].left = -1;
        if (t.nodes[v].right != c) t.nodes[v].right = -1;
        chain.insert(chain.begin(), v);
    }
    reachable.assign(t.nodes.size(), 0);
    std::vector<int32_t> s3{t.root};
    while (!s3.empty()) {
        int32_t v = s3.back();
        s3.pop_back();
        reachable[v] = 1;
        if (t.nodes[v].left >= 0) s3.push_back(t.nodes[v].left);
        if (t.nodes[v].right >= 0) s3.push_back(t.nodes[v].right);
    }
    t.is_shard = true;
    return PFQ_OK;
}

// Balanced synthetic tree topology; same numbering as oracle/pfq_oracle.py:build_balanced_tree.
int32_t build_balanced_rec(pfq_tree &t, const char *const *tax_ids, uint64_t lo, uint64_t hi, int32_t parent,
                           uint32_t depth, uint64_t &internal_counter, std::vector<std::pair<uint64_t, uint64_t>> &range) {
    int32_t v = (int32_t)t.nodes.size();
    t.nodes.emplace_back();
    range.emplace_back(lo, hi);  // genomes below node v
    t.nodes[v].parent = parent;
    t.nodes[v].depth = depth;
    t.nodes[v].filter = (uint32_t)v;
    t.nodes[v].has_tax = true;
    if (hi - lo == 1) {
        t.nodes[v].tax_id = tax_ids[lo];
        t.nodes[v].bf_path = t.nodes[v].tax_id + ".bf";
        return v;
    }
    t.nodes[v].tax_id = "Internal_Node_" + std::to_string(internal_counter++);
    t.nodes[v].bf_path = t.nodes[v].tax_id + ".bf";
    uint64_t mid = lo + (hi - lo + 1) / 2;
    int32_t l = build_balanced_rec(t, tax_ids, lo, mid, v, depth + 1, internal_counter, range);
    int32_t r = build_balanced_rec(t, tax_ids, mid, hi, v, depth + 1, internal_counter, range);
    t.nodes[v].left = l;
    t.nodes[v].right = r;
    return v;
}

// shard: only subtree shard `shard_index` of the depth-`shard_depth` frontier is materialised (its subtree bottom-up from
// its own genomes; every ancestor on the chain = the union of ALL genomes below it in the whole tree, inserted directly).
int build_balanced_common(const uint8_t *d_genomes, const uint64_t *d_goff, uint64_t n_genomes, const char *const *tax_ids,
                          uint64_t kmer_size, uint64_t nbits, uint32_t num_hashes, uint64_t seed1, uint64_t seed2,
                          float fpr, uint32_t largest, int device, bool shard, uint64_t shard_depth, uint64_t shard_index,
                          pfq_tree **out) {
    std::unique_ptr<pfq_tree> t(new pfq_tree());
    t->device = device;
    t->kmer_size = kmer_size;
    t->nbits = nbits;
    t->num_hashes = num_hashes;
    t->seed1 = seed1;
    t->seed2 = seed2;
    t->false_pos_rate = fpr;
    t->largest_expected_genome = largest;
    PFQ_TRY(setup_hash_params(*t));
    if (n_genomes > (1u << 24)) return fail(PFQ_ERR_UNSUPPORTED, "more than 2^24 genomes in one balanced build");
    std::vector<std::pair<uint64_t, uint64_t>> range;
    if (n_genomes) {
        uint64_t counter = 0;
        t->root = build_balanced_rec(*t, tax_ids, 0, n_genomes, -1, 0, counter, range);
    }
    t->tree_leaves = n_genomes;
    std::vector<uint8_t> reachable(t->nodes.size(), 1);
    std::vector<int32_t> chain;
    if (shard) PFQ_TRY(apply_shard(*t, shard_depth, shard_index, reachable, chain));
    std::vector<uint8_t> on_chain(t->nodes.size(), 0);
    for (int32_t v : chain) on_chain[v] = 1;
    // filter rows: one per node that stays (a whole tree: row == node index)
    for (size_t v = 0; v < t->nodes.size(); ++v) {
        if (!reachable[v]) continue;
        t->nodes[v].filter = (uint32_t)t->filter_paths.size();
        t->filter_paths.push_back(t->nodes[v].bf_path);
    }
    const size_t nn = t->nodes.size(), nrows = t->filter_paths.size();
    if (nrows) {
        if (t->d_bits.ensure(nrows * t->n_words) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PFQ_ERR_DEVICE, "not enough device memory for " + std::to_string(nrows) + " filters of " +
                                            std::to_string(t->n_words * 8) + " bytes");
        }
        t->n_rows = t->row_capacity = nrows;
        HIP_TRY(hipMemset(t->d_bits.p, 0, nrows * t->n_words * 8));
        // genome -> filter rows it is inserted into: its leaf (when the leaf stays) and every ancestor on the shard's chain
        // (k_insert takes one row per genome and launch; the chain is a handful of nodes)
        DevBuf<uint32_t> d_leaf_row, d_triples;
        HIP_TRY(d_leaf_row.ensure(n_genomes + 1));
        std::vector<uint32_t> leaf_row(n_genomes, 0xffffffffu);
        for (size_t v = 0; v < nn; ++v)
            if (reachable[v] && range[v].second - range[v].first == 1 && t->nodes[v].is_leaf() && !on_chain[v])
                leaf_row[range[v].first] = t->nodes[v].filter;
        auto insert_range = [&](uint64_t lo, uint64_t hi) -> int {  // genomes [lo, hi) with rows leaf_row[lo..hi)
            // runs of genomes that have a row; blockIdx.y is limited to 65535 genomes per launch
            for (uint64_t g = lo; g < hi;) {
                if (leaf_row[g] == 0xffffffffu) { ++g; continue; }
                uint64_t e = g;
                while (e < hi && e - g < 32768 && leaf_row[e] != 0xffffffffu) ++e;
                HIP_TRY(hipMemcpy(d_leaf_row.p, leaf_row.data() + g, (e - g) * 4, hipMemcpyHostToDevice));
                pfq::launch_insert(t->hp, d_genomes, d_goff + g, (uint32_t)(e - g), d_leaf_row.p, t->d_bits.p, t->n_words, nullptr);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipDeviceSynchronize());
                g = e;
            }
            return PFQ_OK;
        };
        PFQ_TRY(insert_range(0, n_genomes));
        for (int32_t v : chain) {  // ancestors of the shard: every genome below them, straight into their row
            std::fill(leaf_row.begin(), leaf_row.end(), 0xffffffffu);
            for (uint64_t g = range[v].first; g < range[v].second; ++g) leaf_row[g] = t->nodes[v].filter;
            PFQ_TRY(insert_range(range[v].first, range[v].second));
        }
        // internal nodes of the (sub)tree bottom-up, one launch per depth
        uint32_t max_depth = 0;
        for (auto &nd : t->nodes) max_depth = std::max(max_depth, nd.depth);
        for (int d = (int)max_depth; d >= 0; --d) {
            std::vector<uint32_t> triples;
            for (size_t v = 0; v < nn; ++v) {
                const Node &nd = t->nodes[v];
                if ((int)nd.depth != d || nd.is_leaf() || !reachable[v] || on_chain[v]) continue;
                triples.push_back(nd.filter);
                triples.push_back(t->nodes[nd.left].filter);
                triples.push_back(t->nodes[nd.right].filter);
            }
            if (triples.empty()) continue;
            HIP_TRY(d_triples.ensure(triples.size()));
            HIP_TRY(hipMemcpy(d_triples.p, triples.data(), triples.size() * 4, hipMemcpyHostToDevice));
            for (size_t t0 = 0; t0 < triples.size() / 3; t0 += 32768) {
                uint32_t nt = (uint32_t)std::min<size_t>(32768, triples.size() / 3 - t0);
                pfq::launch_union(t->d_bits.p, t->n_words, d_triples.p + 3 * t0, nt, nullptr);
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipDeviceSynchronize());
        }
        HIP_TRY(hipDeviceSynchronize());
        PFQ_TRY(verify_supersets(*t));
    }
    *out = t.release();
    return PFQ_OK;
}

void put_u64(std::vector<uint8_t> &o, uint64_t v) { o.insert(o.end(), (uint8_t *)&v, (uint8_t *)&v + 8); }
void put_u32(std::vector<uint8_t> &o, uint32_t v) { o.insert(o.end(), (uint8_t *)&v, (uint8_t *)&v + 4); }
void put_str(std::vector<uint8_t> &o, const std::string &s) {
    put_u64(o, s.size());
    o.insert(o.end(), s.begin(), s.end());
}
void encode_node(const pfq_tree &t, int32_t v, std::vector<uint8_t> &o) {
    const Node &nd = t.nodes[v];
    for (int32_t c : {nd.left, nd.right}) {
        o.push_back(c >= 0 ? 1 : 0);
        if (c >= 0) encode_node(t, c, o);
    }
    put_str(o, nd.bf_path);
    o.push_back(nd.has_tax ? 1 : 0);
    if (nd.has_tax) put_str(o, nd.tax_id);
    put_u64(o, nd.mapped_reads);
}

const char ORDER_NAME[] = "bitvec::order::Lsb0";

}  // namespace

// =================================================================================================================
// C ABI
// =================================================================================================================
extern "C" {

int pfq_host_alloc(uint64_t bytes, void **out) {
    if (!out) return fail(PFQ_ERR_ARG, "null argument");
    *out = nullptr;
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return PFQ_OK;
}
int pfq_host_free(void *p) {
    if (p) HIP_TRY(hipHostFree(p));
    return PFQ_OK;
}

const char *pfq_last_error(void) { return g_err.c_str(); }
const char *pfq_version(void) { return "libpfq 0.1 (gfx950)"; }

// <dir>/tree.bin (BloomTree::load, bloom_tree.rs:364-386) into the model of `t`: topology, names, counts, parameters.
// Reads no .bf file and uses no device.
static int read_tree_bin(const std::string &dir, pfq_tree &t) {
    std::vector<uint8_t> buf;
    if (!read_file(dir + "/tree.bin", buf))
        return fail(PFQ_ERR_IO, "cannot read " + dir + "/tree.bin (reference: panic at bloom_tree.rs:375)");
    Cur c{buf.data(), buf.size()};
    uint8_t tag = c.u8();
    if (!c.ok || tag > 1) return fail(PFQ_ERR_FORMAT, "tree.bin: bad Option tag for root");
    if (tag == 1) PFQ_TRY(parse_node(c, t, -1, 0, t.root));
    t.false_pos_rate = c.f32();
    t.largest_expected_genome = c.u32();
    t.kmer_size = c.u64();
    t.seed1 = c.u64();
    t.seed2 = c.u64();
    if (!c.ok || c.p != c.n) return fail(PFQ_ERR_FORMAT, "tree.bin: truncated or trailing bytes");
    return PFQ_OK;
}

static int open_impl(const char *db_dir, int device, bool shard, uint64_t shard_depth, uint64_t shard_index, pfq_tree **out) {
    if (!db_dir || !out) return fail(PFQ_ERR_ARG, "null argument");
    *out = nullptr;
    PFQ_TRY(use_device(device));
    std::unique_ptr<pfq_tree> t(new pfq_tree());
    t->device = device;
    std::string dir(db_dir);
    PFQ_TRY(read_tree_bin(dir, *t));
    t->tree_leaves = leaves_dfs(*t).size();
    std::vector<uint8_t> reachable(t->nodes.size(), 1);
    std::vector<int32_t> chain;
    if (shard) PFQ_TRY(apply_shard(*t, shard_depth, shard_index, reachable, chain));
    // filters keyed by relative path, exactly like the LRU cache key (cache.rs:56-62)
    std::map<std::string, uint32_t> row_of;
    for (size_t vi = 0; vi < t->nodes.size(); ++vi) {
        auto &nd = t->nodes[vi];
        if (!reachable[vi]) continue;  // outside this shard: its .bf is never read
        auto it = row_of.find(nd.bf_path);
        if (it == row_of.end()) {
            nd.filter = (uint32_t)t->filter_paths.size();
            row_of[nd.bf_path] = nd.filter;
            t->filter_paths.push_back(nd.bf_path);
        } else nd.filter = it->second;
    }
    // One .bf per filter: read, check, upload.  The first one fixes the geometry; the others are loaded by a few
    // threads side by side (a 1024-leaf database is 2047 files of 9 MB: reading them one after the other takes longer
    // than classifying a hundred million reads).  Returns a status and leaves the message in `msg`.
    pfq_tree *tp = t.get();
    auto load_one = [&](size_t f, std::vector<uint8_t> &fb, bool first, std::string &msg) -> int {
        const std::string path = dir + "/" + tp->filter_paths[f];
        if (!read_file(path, fb)) {
            msg = "cannot read Bloom filter file " + path + " (reference: panic at bloom_filter.rs:155)";
            return PFQ_ERR_IO;
        }
        Cur b{fb.data(), fb.size()};
        std::string order = b.str();
        uint8_t width = b.u8(), index = b.u8();
        uint64_t nbits = b.u64(), nwords = b.u64();
        if (!b.ok || order != ORDER_NAME || width != 64 || index != 0 || nwords != (nbits + 63) / 64) {
            msg = path + ": not a BitVec<usize, Lsb0> BloomFilter (order/head/length mismatch)";
            return PFQ_ERR_FORMAT;
        }
        const uint8_t *words = b.take((size_t)nwords * 8);
        uint32_t nh = b.u32();
        uint64_t s1 = b.u64(), s2 = b.u64();
        uint8_t ptag = b.u8();
        if (b.ok && ptag == 1) (void)b.str();
        if (!b.ok || ptag > 1 || b.p != b.n) {
            msg = path + ": truncated or trailing bytes";
            return PFQ_ERR_FORMAT;
        }
        if (first) {
            tp->nbits = nbits;
            tp->num_hashes = nh;
            int rc = setup_hash_params(*tp);
            if (rc != PFQ_OK) {
                msg = g_err;
                return rc;
            }
            if (tp->d_bits.ensure(tp->filter_paths.size() * tp->n_words) != hipSuccess) {
                (void)hipGetLastError();
                msg = "not enough device memory for " + std::to_string(tp->filter_paths.size()) + " filters";
                return PFQ_ERR_DEVICE;
            }
            tp->n_rows = tp->row_capacity = tp->filter_paths.size();
        }
        if (nbits != tp->nbits || nh != tp->num_hashes) {
            msg = path + ": filter size / num_hashes differ from the other nodes";
            return PFQ_ERR_UNSUPPORTED;
        }
        if (s1 != tp->seed1 || s2 != tp->seed2) {
            msg = path + ": hash seeds differ from tree.bin's (node-independent indices need one seed pair)";
            return PFQ_ERR_UNSUPPORTED;
        }
        if (hipMemcpy(tp->d_bits.p + f * tp->n_words, words, (size_t)nwords * 8, hipMemcpyHostToDevice) != hipSuccess) {
            msg = std::string("hipMemcpy of ") + path + ": " + hipGetErrorString(hipGetLastError());
            return PFQ_ERR_DEVICE;
        }
        return PFQ_OK;
    };
    const size_t n_files = t->filter_paths.size();
    if (n_files) {
        std::vector<uint8_t> fb;
        std::string msg;
        int rc = load_one(0, fb, true, msg);
        if (rc != PFQ_OK) return fail(rc, msg);
    }
    if (n_files > 1) {
        unsigned n_threads = (unsigned)std::min<size_t>(8, n_files - 1);
        if (const char *e = getenv("PFQ_LOAD_THREADS")) n_threads = (unsigned)std::min<size_t>(std::max(1, atoi(e)), n_files - 1);
        std::atomic<size_t> next{1};
        std::mutex err_mu;
        int err_rc = PFQ_OK;
        size_t err_file = ~(size_t)0;  // the lowest-numbered failing file is reported, like a sequential reader would
        std::string err_msg;
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < n_threads; ++w)
            pool.emplace_back([&] {
                (void)hipSetDevice(device);
                std::vector<uint8_t> fb;
                std::string msg;
                for (size_t f; (f = next.fetch_add(1)) < n_files;) {
                    int rc = load_one(f, fb, false, msg);
                    if (rc != PFQ_OK) {
                        std::lock_guard<std::mutex> lk(err_mu);
                        if (f < err_file) {
                            err_file = f;
                            err_rc = rc;
                            err_msg = msg;
                        }
                    }
                }
            });
        for (auto &th : pool) th.join();
        if (err_rc != PFQ_OK) return fail(err_rc, err_msg);
    }
    if (t->root >= 0) PFQ_TRY(verify_supersets(*t));
    *out = t.release();
    return PFQ_OK;
}

int pfq_tree_open(const char *db_dir, int device, pfq_tree **out) { return open_impl(db_dir, device, false, 0, 0, out); }

int pfq_tree_open_subtree(const char *db_dir, int device, uint64_t depth, uint64_t index, pfq_tree **out) {
    return open_impl(db_dir, device, true, depth, index, out);
}

int pfq_db_shard_count(const char *db_dir, uint64_t depth, uint64_t *n_shards) {
    if (!db_dir || !n_shards) return fail(PFQ_ERR_ARG, "null argument");
    *n_shards = 0;
    pfq_tree t;  // the model only: no filter is read, no device is touched
    PFQ_TRY(read_tree_bin(db_dir, t));
    if (t.root < 0) return fail(PFQ_ERR_STATE, "subtree shards of an empty tree");
    *n_shards = shard_frontier(t, depth).size();
    return PFQ_OK;
}

// BloomTree::new (bloom_tree.rs:100-118) with explicit hash seeds: an empty tree whose filters are sized like
// create_bloom_filter / with_rate (bloom_filter.rs:55-70,:229-240).
int pfq_tree_create(uint64_t kmer_size, float false_pos_rate, uint32_t largest_expected_genome, uint64_t seed1, uint64_t seed2,
                    uint64_t expected_genomes, int device, pfq_tree **out) {
    if (!out) return fail(PFQ_ERR_ARG, "null argument");
    *out = nullptr;
    PFQ_TRY(use_device(device));
    std::unique_ptr<pfq_tree> t(new pfq_tree());
    t->device = device;
    t->kmer_size = kmer_size;
    t->false_pos_rate = false_pos_rate;
    t->largest_expected_genome = largest_expected_genome;
    t->seed1 = seed1;
    t->seed2 = seed2;
    if (!(false_pos_rate > 0.0f) || largest_expected_genome == 0)
        return fail(PFQ_ERR_ARG, "false_pos_rate must be > 0 and largest_expected_genome > 0");
    t->nbits = needed_bits_f32(false_pos_rate, largest_expected_genome);
    t->num_hashes = optimal_num_hashes_f32(t->nbits, largest_expected_genome);
    PFQ_TRY(setup_hash_params(*t));
    if (expected_genomes) PFQ_TRY(reserve_rows(*t, 2 * expected_genomes - 1));
    *out = t.release();
    return PFQ_OK;
}

// BloomTree::insert (bloom_tree.rs:128-143): init_leaf_node (:154-168) + add_to_tree (:187-214) + init_internal_node
// (:226-245).  Internal nodes are named `internal_name` or "Internal_Node_<n>" with a running n that is unique in the
// tree (the reference draws a random u16, :231-233, which can collide and then shares a .bf file between two nodes).
int pfq_tree_insert(pfq_tree *tree, const uint8_t *seq, uint64_t len, const char *tax_id, const char *internal_name) {
    if (!tree || !tax_id || (len && !seq)) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(insertion_error(t));
    if (t.is_shard) return fail(PFQ_ERR_STATE, "a subtree shard cannot be extended");
    if (t.n_words == 0) return fail(PFQ_ERR_STATE, "tree has no filter geometry");
    // One .bf per node here.  (The reference keys filters by file name: a second node called <tax_id> gets a fresh empty
    // filter under the first one's key, bloom_tree.rs:294 / cache.rs:83-87, and the two then share one file on disk —
    // SURVEY H4.  Such databases can be OPENED; building one is refused.)
    if (t.path_set.size() != t.filter_paths.size()) {
        t.path_set.clear();
        t.path_set.insert(t.filter_paths.begin(), t.filter_paths.end());
    }
    auto path_taken = [&](const std::string &pth) { return t.path_set.count(pth) != 0; };
    if (path_taken(std::string(tax_id) + ".bf"))
        return fail(PFQ_ERR_ARG, std::string("a node named ") + tax_id + " exists already: two nodes would share " + tax_id + ".bf");
    if (internal_name && (path_taken(std::string(internal_name) + ".bf") || !strcmp(internal_name, tax_id)))
        return fail(PFQ_ERR_ARG, std::string("a node named ") + internal_name + " exists already: two nodes would share " + internal_name + ".bf");
    PFQ_TRY(sync_counts_to_nodes(t));
    t.layout_valid = false;
    t.fm_rows = false;    // (the rows of the last pfq_text_query name the leaves as they were)
    t.drop_tile_lists();  // (made again with the layout)
    t.lca_valid = false;  // (the clade numbering changes: tables and counters start again)
    abund_clear(t);       // (the leaf columns change meaning)
    cover_clear(t);
    sweep_drop(t);        // (the list stays: the counters are made anew for the new leaves)
    tax_clear(t);         // (the taxonomy described the leaves as they were)
    t.cov_bits_valid = false;
    t.merges.clear();     // (a re-clustered tree's merge log describes the shape it was given)
    t.merge_rounds = 0;
    PFQ_TRY(reserve_rows(t, t.n_rows + 2));
    if (!t.greedy_blocks) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, t.device));
        // every block must be resident (one per CU at most); blocks of 1024 threads, half as many as CUs: they stream the filters
        // as fast as all would (measured: 128 blocks 5300, 192 5270, 256 4790 genomes/s)
        int want = prop.multiProcessorCount / 2;
        if (const char *e = getenv("PFQ_GREEDY_BLOCKS")) want = atoi(e);
        t.greedy_blocks = std::max(1, std::min(std::min(pfq::GREEDY_MAX_BLOCKS, prop.multiProcessorCount), want));
    }
    // the device's copy of the shape (all of it once; afterwards the kernel keeps it current)
    const size_t n_after = t.nodes.size() + 2;
    if (t.knobs.greedy_host > 0) {
        // the host walk takes the shape over from the device walk's insertions (before the new leaf is appended: the
        // device's copy has no entry for it yet)
        PFQ_TRY(sync_topology(t));
        t.topo_on_device = false;
        HIP_TRY(t.d_dist.ensure(2 * (size_t)pfq::INSERT_STEP_BLOCKS));
    } else if (!t.topo_on_device || t.d_topo.n < n_after) {
        PFQ_TRY(sync_topology(t));
        HIP_TRY(hipDeviceSynchronize());
        const size_t cap = std::max<size_t>(n_after, 2 * t.d_topo.n + 1024);
        HIP_TRY(t.d_topo.ensure(cap));
        HIP_TRY(t.d_walk.ensure(4));
        const size_t sync_words = (size_t)pfq::GREEDY_SYNC_LINES * pfq::GREEDY_SYNC_STRIDE / 8;
        HIP_TRY(t.d_dist.ensure(std::max<size_t>(sync_words, 2 * (size_t)pfq::INSERT_STEP_BLOCKS)));
        HIP_TRY(hipMemset(t.d_dist.p, 0, sync_words * 8));  // the walk's counters, generation words and accumulators start clear
        std::vector<pfq::TopoNode> h(t.nodes.size());
        for (size_t v = 0; v < h.size(); ++v) h[v] = pfq::TopoNode{t.nodes[v].left, t.nodes[v].right, t.nodes[v].filter, 0u};
        if (!h.empty()) HIP_TRY(hipMemcpy(t.d_topo.p, h.data(), h.size() * sizeof(pfq::TopoNode), hipMemcpyHostToDevice));
        const int st[4] = {t.root, 0, t.root, t.root};
        t.walk_seq = 0;
        HIP_TRY(hipMemcpy(t.d_walk.p, st, sizeof st, hipMemcpyHostToDevice));
        t.topo_on_device = true;
    }
    // the new leaf's filter: the genome goes to one of four staging buffers (the copy of genome i + 1 does not wait for the
    // kernels of genome i), its k-mers are inserted into a cleared row
    const uint32_t new_row = (uint32_t)t.n_rows++, int_row = (uint32_t)t.n_rows++;  // (the internal node's row stays unused by the first leaf of a tree)
    const uint32_t slot = t.gseq_next++ & 3u;
    PFQ_TRY(ensure_copy_stream(t));
    HIP_TRY(t.gseq_copied[slot].ensure(hipEventDisableTiming));
    if (t.gseq_free[slot]) HIP_TRY(hipEventSynchronize(t.gseq_free[slot]));  // the insertion that used these buffers four calls ago has read them
    HIP_TRY(t.gseq_free[slot].ensure(hipEventDisableTiming));
    if (t.d_gseq[slot].n < len + 16) {
        HIP_TRY(t.d_gseq[slot].ensure(std::max<size_t>(len + 16, 2 * t.d_gseq[slot].n)));
    }
    HIP_TRY(t.h_gseq[slot].ensure(len + 16));
    // (through page-locked staging on a stream of its own: the copy neither waits for the kernels of the insertions before
    // nor holds the caller — the kernels wait for it by event)
    if (len) {
        memcpy(t.h_gseq[slot].p, seq, len);
        HIP_TRY(hipMemcpyAsync(t.d_gseq[slot].p, t.h_gseq[slot].p, len, hipMemcpyHostToDevice, t.copy_stream));
    }
    HIP_TRY(hipEventRecord(t.gseq_copied[slot], t.copy_stream));
    HIP_TRY(hipStreamWaitEvent(nullptr, t.gseq_copied[slot], 0));
    HIP_TRY(hipMemsetAsync(t.d_bits.p + (uint64_t)new_row * t.n_words, 0, t.n_words * 8, nullptr));
    pfq::launch_insert_one(t.hp, t.d_gseq[slot].p, len, new_row, t.d_bits.p, t.n_words, nullptr);
    HIP_TRY(hipEventRecord(t.gseq_free[slot], nullptr));
    Node leaf;
    leaf.has_tax = true;
    leaf.tax_id = tax_id;
    leaf.bf_path = std::string(tax_id) + ".bf";
    leaf.filter = new_row;
    t.filter_paths.push_back(leaf.bf_path);
    t.path_set.insert(leaf.bf_path);
    const int32_t nv = (int32_t)t.nodes.size();
    t.nodes.push_back(leaf);
    t.topology_dirty = true;
    // PFQ_GREEDY_HOST=1: the descent level by level from the host (one launch and one read-back per level; no kernel with a
    // grid barrier) — for devices that are shared with other work, where not every block of such a kernel stays resident
    if (t.knobs.greedy_host > 0) {
        if (t.root < 0 || nv == 0) {
            t.root = nv;
            --t.n_rows;  // (no internal node: its row is not used)
            HIP_TRY(hipDeviceSynchronize());
            return PFQ_OK;
        }
        std::vector<unsigned long long> part(2 * pfq::INSERT_STEP_BLOCKS);
        int32_t cur = t.root, parent = -1;
        bool went_right = false;
        while (true) {
            const Node &c = t.nodes[cur];
            if (c.left >= 0 && c.right >= 0) {
                pfq::launch_insert_step(t.d_bits.p, t.n_words, c.filter, new_row, t.nodes[c.left].filter, t.nodes[c.right].filter, t.d_dist.p, nullptr);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpy(part.data(), t.d_dist.p, part.size() * 8, hipMemcpyDeviceToHost));
                unsigned long long d[2] = {0, 0};
                for (uint32_t b = 0; b < pfq::INSERT_STEP_BLOCKS; ++b) {
                    d[0] += part[2 * b];
                    d[1] += part[2 * b + 1];
                }
                parent = cur;
                went_right = d[1] < d[0];  // `if right_distance < left_distance` (bloom_tree.rs:201): ties go left
                cur = went_right ? c.right : c.left;
            } else if (c.is_leaf()) {
                std::string name;
                if (internal_name) name = internal_name;
                else {
                    do name = "Internal_Node_" + std::to_string(t.internal_counter++);
                    while (path_taken(name + ".bf"));
                }
                HIP_TRY(t.d_build.ensure(8));
                const uint32_t triple[3] = {int_row, c.filter, new_row};
                HIP_TRY(hipMemcpy(t.d_build.p + 4, triple, 12, hipMemcpyHostToDevice));
                pfq::launch_union(t.d_bits.p, t.n_words, t.d_build.p + 4, 1, nullptr);
                HIP_TRY(hipGetLastError());
                Node in;
                in.has_tax = true;
                in.tax_id = name;
                in.bf_path = name + ".bf";
                in.filter = int_row;
                in.left = cur;   // the node already in the tree (bloom_tree.rs:241)
                in.right = nv;   // the new leaf (:242)
                t.filter_paths.push_back(in.bf_path);
                t.path_set.insert(in.bf_path);
                const int32_t ni_h = (int32_t)t.nodes.size();
                t.nodes.push_back(in);
                if (parent < 0) t.root = ni_h;
                else (went_right ? t.nodes[parent].right : t.nodes[parent].left) = ni_h;
                break;
            } else {
                return insertion_failed(t, PFQ_ERR_FORMAT, ONE_CHILD_MSG);
            }
        }
        HIP_TRY(hipDeviceSynchronize());
        return PFQ_OK;
    }
    // BloomTree::insert (bloom_tree.rs:128-143): the first leaf is the root; every later one is placed by the greedy descent,
    // which ends in a new internal node (left = the leaf it reached, right = the new leaf, filter = their union)
    int32_t ni = -1;
    if (nv > 0 || t.root >= 0) {
        std::string name;
        if (internal_name) name = internal_name;
        else {
            do name = "Internal_Node_" + std::to_string(t.internal_counter++);
            while (path_taken(name + ".bf"));
        }
        Node in;
        in.has_tax = true;
        in.tax_id = name;
        in.bf_path = name + ".bf";
        in.filter = int_row;
        in.right = nv;   // the new leaf (:242); `left` = the leaf the walk reaches, known on the device (sync_topology)
        t.filter_paths.push_back(in.bf_path);
        t.path_set.insert(in.bf_path);
        ni = (int32_t)t.nodes.size();
        t.nodes.push_back(in);
    } else {
        --t.n_rows;  // (no internal node: its row is not used)
    }
    if (ni < 0) t.root = nv;  // (the host's root is only a hint while insertions are pending; empty vs. not is what counts)
    pfq::launch_greedy_insert(t.d_bits.p, t.n_words, t.d_topo.p, t.d_walk.p, t.d_dist.p, nv, ni < 0 ? nv : ni, new_row, int_row, t.walk_seq++, t.greedy_blocks, nullptr);
    HIP_TRY(hipGetLastError());
    t.topo_pending = true;
    return PFQ_OK;
}

int pfq_tree_build_balanced(const uint8_t *genomes, const uint64_t *offsets, uint64_t n_genomes, const char *const *tax_ids,
                            uint64_t kmer_size, uint64_t nbits, uint32_t num_hashes, uint64_t seed1, uint64_t seed2,
                            float false_pos_rate, uint32_t largest_expected_genome, int device, pfq_tree **out) {
    if (!out || (n_genomes && (!genomes || !offsets || !tax_ids))) return fail(PFQ_ERR_ARG, "null argument");
    *out = nullptr;
    PFQ_TRY(use_device(device));
    DevBuf<uint8_t> d_g;
    DevBuf<uint64_t> d_o;
    uint64_t total = n_genomes ? offsets[n_genomes] : 0;
    HIP_TRY(d_g.ensure(total + 1));
    HIP_TRY(d_o.ensure(n_genomes + 1));
    if (total) HIP_TRY(hipMemcpy(d_g.p, genomes, total, hipMemcpyHostToDevice));
    if (n_genomes) HIP_TRY(hipMemcpy(d_o.p, offsets, (n_genomes + 1) * 8, hipMemcpyHostToDevice));
    return build_balanced_common(d_g.p, d_o.p, n_genomes, tax_ids, kmer_size, nbits, num_hashes, seed1, seed2,
                                 false_pos_rate, largest_expected_genome, device, false, 0, 0, out);
}

int pfq_tree_build_balanced_device(const uint8_t *d_genomes, uint64_t genome_len, uint64_t n_genomes,
                                   const char *const *tax_ids, uint64_t kmer_size, uint64_t nbits, uint32_t num_hashes,
                                   uint64_t seed1, uint64_t seed2, float false_pos_rate, uint32_t largest_expected_genome,
                                   int device, pfq_tree **out) {
    if (!out || (n_genomes && (!d_genomes || !tax_ids))) return fail(PFQ_ERR_ARG, "null argument");
    *out = nullptr;
    PFQ_TRY(use_device(device));
    std::vector<uint64_t> off(n_genomes + 1);
    for (uint64_t i = 0; i <= n_genomes; ++i) off[i] = i * genome_len;
    DevBuf<uint64_t> d_o;
    HIP_TRY(d_o.ensure(n_genomes + 1));
    HIP_TRY(hipMemcpy(d_o.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    return build_balanced_common(d_genomes, d_o.p, n_genomes, tax_ids, kmer_size, nbits, num_hashes, seed1, seed2,
                                 false_pos_rate, largest_expected_genome, device, false, 0, 0, out);
}

int pfq_tree_build_balanced_subtree_device(const uint8_t *d_genomes, uint64_t genome_len, uint64_t n_genomes,
                                           const char *const *tax_ids, uint64_t kmer_size, uint64_t nbits, uint32_t num_hashes,
                                           uint64_t seed1, uint64_t seed2, float false_pos_rate, uint32_t largest_expected_genome,
                                           uint64_t depth, uint64_t index, int device, pfq_tree **out) {
    if (!out || (n_genomes && (!d_genomes || !tax_ids))) return fail(PFQ_ERR_ARG, "null argument");
    *out = nullptr;
    PFQ_TRY(use_device(device));
    std::vector<uint64_t> off(n_genomes + 1);
    for (uint64_t i = 0; i <= n_genomes; ++i) off[i] = i * genome_len;
    DevBuf<uint64_t> d_o;
    HIP_TRY(d_o.ensure(n_genomes + 1));
    HIP_TRY(hipMemcpy(d_o.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    return build_balanced_common(d_genomes, d_o.p, n_genomes, tax_ids, kmer_size, nbits, num_hashes, seed1, seed2,
                                 false_pos_rate, largest_expected_genome, device, true, depth, index, out);
}

int pfq_tree_save(const pfq_tree *tree, const char *db_dir) {
    if (!tree || !db_dir) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    PFQ_TRY(finish_topology(*const_cast<pfq_tree *>(tree)));
    // BloomTree::save writes the live mapped_reads (bloom_tree.rs:339-355): fold the device counters back first
    PFQ_TRY(sync_counts_to_nodes(*const_cast<pfq_tree *>(tree)));
    const pfq_tree &t = *tree;
    if (t.is_shard) return fail(PFQ_ERR_STATE, "a subtree shard is not a whole database and cannot be saved");
    std::string dir(db_dir);
    std::vector<uint8_t> o;
    o.push_back(t.root >= 0 ? 1 : 0);
    if (t.root >= 0) encode_node(t, t.root, o);
    o.insert(o.end(), (const uint8_t *)&t.false_pos_rate, (const uint8_t *)&t.false_pos_rate + 4);
    put_u32(o, t.largest_expected_genome);
    put_u64(o, t.kmer_size);
    put_u64(o, t.seed1);
    put_u64(o, t.seed2);
    {
        FILE *f = fopen((dir + "/tree.bin").c_str(), "wb");
        if (!f) return fail(PFQ_ERR_IO, "cannot create " + dir + "/tree.bin: " + strerror(errno));
        bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
        ok = (fclose(f) == 0) && ok;
        if (!ok) return fail(PFQ_ERR_IO, "short write to tree.bin");
    }
    std::vector<uint64_t> words((size_t)t.n_words);
    for (size_t fi = 0; fi < t.filter_paths.size(); ++fi) {
        HIP_TRY(hipMemcpy(words.data(), t.d_bits.p + fi * t.n_words, (size_t)t.n_words * 8, hipMemcpyDeviceToHost));
        std::vector<uint8_t> h;
        put_str(h, ORDER_NAME);
        h.push_back(64);
        h.push_back(0);
        put_u64(h, t.nbits);
        put_u64(h, t.n_words);
        std::vector<uint8_t> tail;
        put_u32(tail, t.num_hashes);
        put_u64(tail, t.seed1);
        put_u64(tail, t.seed2);
        const std::string path = dir + "/" + t.filter_paths[fi];
        tail.push_back(1);
        put_str(tail, path);
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) return fail(PFQ_ERR_IO, "cannot create " + path + ": " + strerror(errno));
        bool ok = fwrite(h.data(), 1, h.size(), f) == h.size();
        ok = ok && fwrite(words.data(), 8, words.size(), f) == words.size();
        ok = ok && fwrite(tail.data(), 1, tail.size(), f) == tail.size();
        ok = (fclose(f) == 0) && ok;
        if (!ok) return fail(PFQ_ERR_IO, "short write to " + path);
    }
    return PFQ_OK;
}

int pfq_tree_info(const pfq_tree *tree, pfq_info *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    if (tree->topology_dirty && tree->insert_err == PFQ_OK) {
        PFQ_TRY(use_device(tree->device));
        // (an insertion that failed is learnt here without failing the call: the parameters stay readable)
        const int rc = finish_topology(*const_cast<pfq_tree *>(tree));
        if (rc != PFQ_OK && tree->insert_err == PFQ_OK) return rc;
    }
    const pfq_tree &t = *tree;
    out->kmer_size = t.kmer_size;
    out->nbits = t.nbits;
    out->num_hashes = t.num_hashes;
    out->largest_expected_genome = t.largest_expected_genome;
    out->false_pos_rate = t.false_pos_rate;
    out->superset_verified = t.superset_all ? 1 : 0;
    out->seed1 = t.seed1;
    out->seed2 = t.seed2;
    out->n_nodes = t.nodes.size();
    out->n_leaves = leaves_dfs(t).size();
    out->n_filters = t.filter_paths.size();
    out->shard_first_leaf = t.shard_first_leaf;
    out->tree_leaves = t.is_shard ? t.tree_leaves : out->n_leaves;
    out->device_bytes = t.d_bits.bytes() + t.d_S.bytes() + t.d_pairs.bytes() + t.d_sorted.bytes() + t.d_fail.bytes() +
                        t.d_hit_pairs.bytes() + t.d_seq.bytes() + t.d_off.bytes() + t.d_recs.bytes() + t.d_entries.bytes() +
                        t.d_ab_start.bytes() + t.d_ab_len.bytes() + t.d_ab_entries.bytes() + t.d_ab_unique.bytes() +  // (the abundance log)
                        t.d_cov_regs.bytes() + t.d_cov_cnt.bytes() +                                                  // (the coverage sketch)
                        t.d_sw_state.bytes() +                                                                        // (the threshold sweep)
                        t.d_tax_rank.bytes() + t.d_tax_leaf_node.bytes() + t.d_tax_parent.bytes() + t.d_tax_first.bytes() +   // (the taxonomy)
                        t.d_tax_gap_min.bytes() + t.d_tax_here.bytes() + t.d_tax_any.bytes() + t.d_tax_misc.bytes() +
                        t.d_fr_bytes.bytes() + t.d_fr_foff.bytes() + t.d_fr_seq.bytes() + t.d_fr_start.bytes() + t.d_fr_segpos.bytes() +  // (pfq_query_frames)
                        t.d_fr_cnt.bytes() + t.d_fr_def.bytes() + t.d_fr_seq0.bytes() + t.d_fr_defoff.bytes() + t.d_fr_seqseg.bytes() + t.d_fr_sums.bytes() +
                        t.d_fr_segs.bytes() + t.d_fr_segseq.bytes() + t.d_fr_queue.bytes() + t.d_fr_pieceoff.bytes() + t.d_fr_parts.bytes() + t.d_fr_misc.bytes() +
                        t.d_tx_text.bytes() + t.d_tx_seq[0].bytes() + t.d_tx_seq[1].bytes() + t.d_tx_off[0].bytes() + t.d_tx_off[1].bytes() +  // (pfq_text_parse)
                        t.d_tx_rec_begin.bytes() + t.d_tx_blk.bytes() + t.d_tx_line.bytes() + t.d_tx_len.bytes() + t.d_tx_hdr.bytes() + t.d_tx_rec_line.bytes() +
                        t.d_tx_bad.bytes() + t.d_tx_blk_off.bytes() + t.d_tx_sums.bytes() + t.d_tx_dst.bytes() + t.d_tx_rec_idx.bytes() + t.d_tx_res.bytes() +
                        t.d_gz.bytes() + t.d_gz_text.bytes() + t.d_gz_mem.bytes() + t.d_gz_res.bytes() +  // (pfq_text_inflate)
                        t.d_df_text.bytes() + t.d_df_slots.bytes() + t.d_df_gz[0].bytes() + t.d_df_gz[1].bytes() + t.d_df_mem.bytes() +  // (pfq_bgzf_deflate)
                        t.d_df_tokens.bytes() + t.d_df_sizes.bytes() + t.d_df_off.bytes() + t.d_df_sums.bytes() +
                        t.d_pp_in.bytes() + t.d_pp_qual.bytes() + t.d_pp_hq.bytes() + t.d_pp_seq[0].bytes() + t.d_pp_seq[1].bytes() + t.d_pp_inoff.bytes() +  // (pfq_prep_reads)
                        t.d_pp_off[0].bytes() + t.d_pp_off[1].bytes() + t.d_pp_begin.bytes() + t.d_pp_len.bytes() + t.d_pp_reason.bytes() + t.d_pp_keep.bytes() +
                        t.d_pp_klen.bytes() + t.d_pp_kept.bytes() + t.d_pp_kpos.bytes() + t.d_pp_koff.bytes() + t.d_pp_sums.bytes() + t.d_pp_tot.bytes() +
                        t.d_pp_cut.bytes() + t.d_pp_which.bytes() + t.d_pp_atot.bytes() +  // (the adapter step)
                        t.d_pp_oins.bytes() + t.d_pp_omm.bytes() + t.d_pp_ecut.bytes() + t.d_pp_otot.bytes() +  // (the mate overlap step)
                        t.d_pp_ctot.bytes() + t.d_pp_cat.bytes() + t.d_pp_ccnt.bytes() + t.d_pp_patch.bytes() +  // (the mate correction)
                        t.d_dp_hit.bytes() + t.d_dp_tot.bytes() +  // (pfq_prep_deplete)
                        t.d_fm_idb.bytes() + t.d_fm_idl.bytes() + t.d_fm_len[0].bytes() + t.d_fm_len[1].bytes() + t.d_fm_long.bytes() +  // (pfq_text_format)
                        t.d_fm_name_off.bytes() + t.d_fm_hash.bytes() + t.d_fm_dst[0].bytes() + t.d_fm_dst[1].bytes() + t.d_fm_sums.bytes() +
                        t.d_fm_small.bytes() + t.d_fm_names.bytes() + t.d_fm_out[0].bytes() + t.d_fm_out[1].bytes();
    return PFQ_OK;
}

int pfq_tree_prune(pfq_tree *tree, uint64_t search_depth) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(finish_topology(t));
    if (t.root < 0) return fail(PFQ_ERR_STATE, "prune_tree on an empty tree (reference: unwrap panic, bloom_tree.rs:310)");
    PFQ_TRY(sync_counts_to_nodes(t));
    relink(t);
    for (auto &nd : t.nodes)
        if (nd.depth >= search_depth) nd.left = nd.right = -1;  // bloom_tree.rs:322-325
    // nodes below the cut are unreachable now; they keep their slots (and filters) but never appear as leaves
    t.layout_valid = false;
    t.fm_rows = false;    // (the rows of the last pfq_text_query name the leaves as they were)
    t.drop_tile_lists();  // (made again with the layout)
    t.lca_valid = false;  // (the clade numbering changes: tables and counters start again)
    abund_clear(t);       // (the leaf columns change meaning)
    cover_clear(t);
    sweep_drop(t);        // (the list stays: the counters are made anew for the new leaves)
    tax_clear(t);         // (the taxonomy described the leaves as they were)
    t.cov_bits_valid = false;
    t.merges.clear();     // (a re-clustered tree's merge log describes the shape it was given)
    t.merge_rounds = 0;
    return PFQ_OK;
}

void pfq_tree_close(pfq_tree *tree) {
    if (!tree) return;
    (void)hipSetDevice(tree->device);
    (void)hipDeviceSynchronize();
    delete tree;
}

// The host block of pfq_query_batch / pfq_query_frames into device memory.  Two input buffers and a copy stream of its own: the
// copy of this block runs while the kernels of the previous block (which read the other buffer) are still at work.  A call
// that wants no hits returns once its kernels are queued; counts are read by calls that synchronise (pfq_leaf_counts,
// pfq_last_stats, pfq_tree_close).  slot: which pair (d_seq / d_off or d_seq2 / d_off2) holds the block; the caller records
// the set as read (in_sets.read_by) behind the kernels that read it.
static int stage_input(pfq_tree &t, const uint8_t *seq, const uint64_t *offsets, uint64_t n_reads, uint64_t total, int &slot) {
    PFQ_TRY(ensure_copy_stream(t));
    HIP_TRY(t.in_sets.ensure());
    slot = t.in_sets.cur = t.in_sets.other();
    HIP_TRY(t.in_sets.wait(slot));  // the kernels that read this buffer are done
    DevBuf<uint8_t> &ds = slot ? t.d_seq2 : t.d_seq;
    DevBuf<uint64_t> &dof = slot ? t.d_off2 : t.d_off;
    HIP_TRY(ds.ensure(total + 16));
    HIP_TRY(dof.ensure(n_reads + 1));
    if (total) HIP_TRY(hipMemcpyAsync(ds.p, seq, total, hipMemcpyHostToDevice, t.copy_stream));
    if (n_reads) HIP_TRY(hipMemcpyAsync(dof.p, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, t.copy_stream));
    HIP_TRY(hipStreamSynchronize(t.copy_stream));
    return PFQ_OK;
}

// Flags of a query call; every query call ends the validity of the previous call's scores, a refused one included.
static int check_flags(pfq_tree &t, uint32_t flags, uint64_t n_reads, float threshold) {
    t.fm_rows = false;
    t.scores_valid = false;
    t.lca_last = false;
    t.taxa_last = false;
    t.best_last = false;
    if ((flags & PFQ_ROWS_BEST) && (~flags & (PFQ_WANT_HITS | PFQ_WANT_SCORES)))
        return fail(PFQ_ERR_ARG, "PFQ_ROWS_BEST needs PFQ_WANT_HITS | PFQ_WANT_SCORES");
    if ((flags & PFQ_ROWS_BEST) && t.is_shard)
        return fail(PFQ_ERR_UNSUPPORTED, "PFQ_ROWS_BEST on a subtree shard: a shard sees only its own leaves, and the best of a partial row "
                                         "is not the row's best");
    if (flags & PFQ_WANT_SWEEP) {
        if (~flags & (PFQ_WANT_HITS | PFQ_WANT_SCORES)) return fail(PFQ_ERR_ARG, "PFQ_WANT_SWEEP needs PFQ_WANT_HITS | PFQ_WANT_SCORES");
        if (flags & PFQ_PAIRED)
            return fail(PFQ_ERR_ARG, "PFQ_WANT_SWEEP with PFQ_PAIRED: a fragment's score is its mates' sum and its row a union or an intersection "
                                     "of per-mate decisions, so its rows at other thresholds do not follow from them");
        if (t.sw_thr.empty()) return fail(PFQ_ERR_STATE, "PFQ_WANT_SWEEP without a threshold list: pfq_tree_set_sweep first");
        if (!(threshold <= t.sw_thr[0]))
            return fail(PFQ_ERR_ARG, "PFQ_WANT_SWEEP: the call's threshold (" + std::to_string(threshold) + ") must not be above the list's lowest (" +
                                     std::to_string(t.sw_thr[0]) + "): the rows of a higher threshold lack entries the lower ones have");
    }
    if ((flags & PFQ_WANT_TAXA) && !(flags & PFQ_WANT_HITS)) return fail(PFQ_ERR_ARG, "PFQ_WANT_TAXA needs PFQ_WANT_HITS");
    if ((flags & PFQ_WANT_TAXA) && t.is_shard)
        return fail(PFQ_ERR_UNSUPPORTED, "PFQ_WANT_TAXA on a subtree shard: a shard sees only its own leaves, so its rows are partial");
    if ((flags & PFQ_LCA_BEST) && (~flags & (PFQ_WANT_LCA | PFQ_WANT_HITS | PFQ_WANT_SCORES)))
        return fail(PFQ_ERR_ARG, "PFQ_LCA_BEST needs PFQ_WANT_LCA | PFQ_WANT_HITS | PFQ_WANT_SCORES");
    if ((flags & PFQ_WANT_LCA) && t.is_shard)
        return fail(PFQ_ERR_UNSUPPORTED, "PFQ_WANT_LCA on a subtree shard: a shard holds only its own subtree and ancestor chain, not the "
                                         "other shards' topology, so its clades are not the whole tree's");
    if ((flags & PFQ_WANT_SCORES) && !(flags & PFQ_WANT_HITS)) return fail(PFQ_ERR_ARG, "PFQ_WANT_SCORES needs PFQ_WANT_HITS");
    if ((flags & PFQ_WANT_ABUNDANCE) && !(flags & PFQ_WANT_HITS)) return fail(PFQ_ERR_ARG, "PFQ_WANT_ABUNDANCE needs PFQ_WANT_HITS");
    if ((flags & PFQ_WANT_ABUNDANCE) && t.is_shard) return abund_shard_refused();
    if ((flags & PFQ_WANT_COVERAGE) && !(flags & PFQ_WANT_HITS)) return fail(PFQ_ERR_ARG, "PFQ_WANT_COVERAGE needs PFQ_WANT_HITS");
    if ((flags & PFQ_PAIRED) && (n_reads & 1)) return fail(PFQ_ERR_ARG, "PFQ_PAIRED needs an even number of reads (mates 2i, 2i + 1)");
    if ((flags & PFQ_PAIR_BOTH) && !(flags & PFQ_PAIRED)) return fail(PFQ_ERR_ARG, "PFQ_PAIR_BOTH needs PFQ_PAIRED");
    return PFQ_OK;
}

int pfq_query_batch_device(pfq_tree *tree, const uint8_t *d_seq, const uint64_t *d_offsets, uint64_t n_reads,
                           uint64_t total_bytes, float threshold, uint32_t flags, void *stream, pfq_hits *hits) {
    if (!tree || (n_reads && (!d_seq || !d_offsets))) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(check_flags(*tree, flags, n_reads, threshold));
    PFQ_TRY(use_device(tree->device));
    return query_device(*tree, d_seq, d_offsets, n_reads, total_bytes, threshold, flags, (hipStream_t)stream, hits);
}

int pfq_query_batch(pfq_tree *tree, const uint8_t *seq, const uint64_t *offsets, uint64_t n_reads, float threshold,
                    uint32_t flags, pfq_hits *hits) {
    if (!tree || (n_reads && (!seq || !offsets))) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(check_flags(*tree, flags, n_reads, threshold));
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    uint64_t total = n_reads ? offsets[n_reads] : 0;
    int slot = 0;
    PFQ_TRY(stage_input(t, seq, offsets, n_reads, total, slot));
    PFQ_TRY(query_device(t, (slot ? t.d_seq2 : t.d_seq).p, (slot ? t.d_off2 : t.d_off).p, n_reads, total, threshold, flags, nullptr, hits));
    HIP_TRY(t.in_sets.read_by(slot, nullptr));
    if (flags & PFQ_WANT_HITS) HIP_TRY(hipStreamSynchronize(nullptr));
    return PFQ_OK;
}

// Flags and arguments of a frames call; like every query call it ends the validity of the previous call's scores and LCAs.
static int check_frames(pfq_tree *tree, const void *seq, const void *offsets, uint64_t n_seqs, uint32_t flags, pfq_segments *out) {
    if (!tree || !out || (n_seqs && (!seq || !offsets))) return fail(PFQ_ERR_ARG, "null argument");
    tree->fm_rows = false;
    tree->scores_valid = false;
    tree->lca_last = false;
    tree->taxa_last = false;
    tree->best_last = false;
    if (flags) return fail(PFQ_ERR_ARG, "pfq_query_frames: flags must be 0 (frames do not combine with pairs, LCA, abundance or coverage)");
    return PFQ_OK;
}
static int frames_call(pfq_tree &t, const uint8_t *d_seq, const uint64_t *d_off, uint64_t n_seqs, uint32_t frame, uint32_t step, float threshold,
                       hipStream_t st, pfq_segments *out) {
    const int rc = query_frames_device(t, d_seq, d_off, n_seqs, frame, step, threshold, st, out);
    if (t.last_done && t.have_last_stream && t.last_stream == st) HIP_TRY(hipEventRecord(t.last_done, st));  // (what waits for this call)
    return rc;
}

int pfq_query_frames_device(pfq_tree *tree, const uint8_t *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t total_bytes, uint32_t frame,
                            uint32_t step, float threshold, uint32_t flags, void *stream, pfq_segments *out) {
    (void)total_bytes;  // (the frames' own buffer is what the classification reads: its size is known)
    PFQ_TRY(check_frames(tree, d_seq, d_offsets, n_seqs, flags, out));
    PFQ_TRY(use_device(tree->device));
    return frames_call(*tree, d_seq, d_offsets, n_seqs, frame, step, threshold, (hipStream_t)stream, out);
}

int pfq_query_frames(pfq_tree *tree, const uint8_t *seq, const uint64_t *offsets, uint64_t n_seqs, uint32_t frame, uint32_t step, float threshold,
                     uint32_t flags, pfq_segments *out) {
    PFQ_TRY(check_frames(tree, seq, offsets, n_seqs, flags, out));
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    int slot = 0;
    PFQ_TRY(stage_input(t, seq, offsets, n_seqs, n_seqs ? offsets[n_seqs] : 0, slot));
    PFQ_TRY(frames_call(t, (slot ? t.d_seq2 : t.d_seq).p, (slot ? t.d_off2 : t.d_off).p, n_seqs, frame, step, threshold, nullptr, out));
    HIP_TRY(t.in_sets.read_by(slot, nullptr));
    return PFQ_OK;
}

// ---- text ---------------------------------------------------------------------------------------------------------------

static uint32_t text_tile(const Knobs &k) {
    const long long v = k.text_tile;  // (the environment is not checked when it is read: anything but a power of two in range is the built-in)
    return (v >= (long long)pfq::TEXT_TILE_MIN && v <= (long long)pfq::TEXT_TILE_DEFAULT && !(v & (v - 1))) ? (uint32_t)v : pfq::TEXT_TILE_DEFAULT;
}

// What both parse calls do first: the copy stream and the events, the CSR set the coming parse fills (waiting for the
// classification that read it), room for n bytes of text in d_tx_text.  From here there is no block to query until the parse
// has succeeded.
static int text_parse_begin(pfq_tree &t, uint32_t n, int *slot_out) {
    PFQ_TRY(ensure_copy_stream(t));
    HIP_TRY(t.tx_parsed.ensure(hipEventDisableTiming));
    HIP_TRY(t.tx_sets.ensure());
    HIP_TRY(t.h_tx_res.ensure(pfq::TEXT_RES_N));
    HIP_TRY(t.d_tx_res.ensure(pfq::TEXT_RES_N));
    HIP_TRY(t.d_tx_bad.ensure(1));
    const int slot = t.tx_sets.other();
    HIP_TRY(t.tx_sets.wait(slot));  // the classification that read this set is done
    t.tx_have = false;  // (until this parse has succeeded there is no block to query)
    t.fm_rows = false;
    HIP_TRY(t.d_tx_seq[slot].ensure((size_t)n + 16));
    if (n) HIP_TRY(t.d_tx_text.ensure(((size_t)n + 15) / 16 * 16 + 16));
    *slot_out = slot;
    return PFQ_OK;
}

// The parse of d_tx_text[0, n), which the caller has queued on the copy stream; first and last: text[0] and text[n - 1].
static int text_parse_staged(pfq_tree &t, int slot, uint32_t n, uint8_t first, uint8_t last, uint64_t limit, bool fastq, bool final, bool want_rec,
                             pfq_text *out) {
    hipStream_t st = t.copy_stream;
    out->n_records = out->consumed = out->n_bases = 0;
    out->stop = PFQ_TEXT_END;
    out->rec_begin = nullptr;
    uint32_t n_lines = 0;
    bool unterminated = false;
    if (n) {
        const uint32_t tile = text_tile(t.knobs), n_tiles = (n + tile - 1) / tile;
        HIP_TRY(t.d_tx_blk.ensure(n_tiles));
        HIP_TRY(t.d_tx_blk_off.ensure((size_t)n_tiles + 1));
        HIP_TRY(t.d_tx_sums.ensure((size_t)n_tiles / 4096 + 2));
        pfq::launch_text_count(t.d_tx_text.p, n, tile, t.d_tx_blk.p, st);
        pfq::launch_scan_u32(t.d_tx_blk.p, n_tiles, t.d_tx_sums.p, t.d_tx_blk_off.p, st);
        HIP_TRY(hipMemcpyAsync(t.h_tx_res.p, t.d_tx_blk_off.p + n_tiles, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));  // (the caller's buffer is free from here; the line count sizes what follows)
        unterminated = final && last != '\n';
        n_lines = (uint32_t)t.h_tx_res.p[0] + (unterminated ? 1u : 0u);
    }
    // what needs no kernel: empty text; text without a considered line; FASTA that does not begin with a header
    bool trivial = true;
    if (!n) out->stop = PFQ_TEXT_END;
    else if (!fastq && first != '>') out->stop = PFQ_TEXT_SLOW;
    else if (!n_lines) out->stop = (fastq || limit) ? PFQ_TEXT_MORE : PFQ_TEXT_LIMIT;
    else trivial = false;
    const uint64_t max_records = fastq ? n_lines / 4 : n_lines;
    HIP_TRY(t.d_tx_off[slot].ensure(max_records + 1));
    if (want_rec) HIP_TRY(t.d_tx_rec_begin.ensure(max_records + 1));
    if (trivial) {
        HIP_TRY(hipMemsetAsync(t.d_tx_off[slot].p, 0, 8, st));
        if (want_rec) t.out_rec_begin.assign(1, 0);
    } else {
        HIP_TRY(t.d_tx_line.ensure((size_t)n_lines + 1));
        HIP_TRY(t.d_tx_len.ensure(n_lines));
        HIP_TRY(t.d_tx_dst.ensure((size_t)n_lines + 1));
        HIP_TRY(t.d_tx_sums.ensure((size_t)n_lines / 4096 + 2));
        pfq::TextArgs a{};
        a.text = t.d_tx_text.p;
        a.len = n;
        a.n_lines = n_lines;
        a.limit = limit;
        a.fastq = fastq ? 1 : 0;
        a.final = final ? 1 : 0;
        a.line_start = t.d_tx_line.p;
        a.line_len = t.d_tx_len.p;
        a.dst = t.d_tx_dst.p;
        a.first_bad = t.d_tx_bad.p;
        a.result = t.d_tx_res.p;
        const uint32_t tile = text_tile(t.knobs);
        pfq::launch_text_lines(t.d_tx_text.p, n, tile, t.d_tx_blk_off.p, t.d_tx_line.p, n_lines, unterminated, st);
        if (fastq) {
            const uint32_t n_full = n_lines / 4;
            t.h_tx_res.p[1] = n_full;  // (little-endian: its low word is what is copied; the result lands here only behind this copy)
            HIP_TRY(hipMemcpyAsync(t.d_tx_bad.p, t.h_tx_res.p + 1, 4, hipMemcpyHostToDevice, st));
        } else {
            HIP_TRY(t.d_tx_hdr.ensure(n_lines));
            HIP_TRY(t.d_tx_rec_idx.ensure((size_t)n_lines + 1));
            HIP_TRY(t.d_tx_rec_line.ensure(n_lines));
            a.rec_idx = t.d_tx_rec_idx.p;
            a.rec_line = t.d_tx_rec_line.p;
        }
        pfq::launch_text_roles(a, t.d_tx_hdr.p, st);
        pfq::launch_scan_u32(t.d_tx_len.p, n_lines, t.d_tx_sums.p, t.d_tx_dst.p, st);
        if (!fastq) {
            pfq::launch_scan_u32(t.d_tx_hdr.p, n_lines, t.d_tx_sums.p, t.d_tx_rec_idx.p, st);
            pfq::launch_text_rec_lines(t.d_tx_hdr.p, t.d_tx_rec_idx.p, n_lines, t.d_tx_rec_line.p, st);
        }
        pfq::launch_text_finish(a, t.d_tx_seq[slot].p, t.d_tx_off[slot].p, want_rec ? t.d_tx_rec_begin.p : nullptr, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(t.h_tx_res.p, t.d_tx_res.p, pfq::TEXT_RES_N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        out->n_records = t.h_tx_res.p[pfq::TEXT_RES_RECORDS];
        out->consumed = t.h_tx_res.p[pfq::TEXT_RES_CONSUMED];
        out->n_bases = t.h_tx_res.p[pfq::TEXT_RES_BASES];
        out->stop = (uint32_t)t.h_tx_res.p[pfq::TEXT_RES_STOP];
        if (want_rec) {
            t.out_rec_begin.resize(out->n_records + 1);
            HIP_TRY(hipMemcpyAsync(t.out_rec_begin.data(), t.d_tx_rec_begin.p, (out->n_records + 1) * 8, hipMemcpyDeviceToHost, st));
        }
    }
    HIP_TRY(hipEventRecord(t.tx_parsed, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (want_rec) out->rec_begin = t.out_rec_begin.data();
    t.tx_sets.cur = slot;
    t.tx_records = out->n_records;
    t.tx_bases = out->n_bases;
    t.tx_fastq = fastq ? 1 : 0;
    t.tx_len = n;
    t.tx_have = true;
    return PFQ_OK;
}

int pfq_text_parse(pfq_tree *tree, const uint8_t *text, uint64_t len, uint64_t limit, int format, uint32_t flags, pfq_text *out) {
    if (!tree || !out || (len && !text)) return fail(PFQ_ERR_ARG, "null argument");
    if (format != PFQ_TEXT_FASTA && format != PFQ_TEXT_FASTQ) return fail(PFQ_ERR_ARG, "pfq_text_parse: format must be PFQ_TEXT_FASTA or PFQ_TEXT_FASTQ");
    if (flags & ~(PFQ_TEXT_FINAL | PFQ_TEXT_WANT_RECORDS)) return fail(PFQ_ERR_ARG, "pfq_text_parse: unknown flag bits");
    if (len >> 31) return fail(PFQ_ERR_UNSUPPORTED, "pfq_text_parse: 2^31 bytes of text or more in one call: ask in pieces");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    const uint32_t n = (uint32_t)len;
    int slot = 0;
    PFQ_TRY(text_parse_begin(t, n, &slot));
    if (n) HIP_TRY(hipMemcpyAsync(t.d_tx_text.p, text, n, hipMemcpyHostToDevice, t.copy_stream));
    return text_parse_staged(t, slot, n, n ? text[0] : 0, n ? text[n - 1] : 0, limit, format == PFQ_TEXT_FASTQ, (flags & PFQ_TEXT_FINAL) != 0,
                             (flags & PFQ_TEXT_WANT_RECORDS) != 0, out);
}


int pfq_text_query(pfq_tree *tree, float threshold, uint32_t flags, pfq_hits *hits) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(check_flags(*tree, flags, tree->tx_records, threshold));
    if (!tree->tx_have) return fail(PFQ_ERR_STATE, "pfq_text_query before a pfq_text_parse on this tree");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    const int slot = t.tx_sets.cur;
    HIP_TRY(hipStreamWaitEvent(nullptr, t.tx_parsed, 0));  // (the classification is ordered behind the parse on the device)
    const int rc = query_device(t, t.d_tx_seq[slot].p, t.d_tx_off[slot].p, t.tx_records, t.tx_bases, threshold, flags, nullptr, hits);
    HIP_TRY(t.tx_sets.read_by(slot, nullptr));  // (also behind a call that failed half-way: what it queued may read the set)
    PFQ_TRY(rc);
    if (flags & PFQ_WANT_HITS) HIP_TRY(hipStreamSynchronize(nullptr));
    t.fm_rows = (flags & PFQ_WANT_HITS) && !(flags & PFQ_PAIRED);  // (pfq_text_format reads these rows)
    t.fm_rows_leaves = t.leaves.size();
    return PFQ_OK;
}

int pfq_debug_text_csr(pfq_tree *tree, uint8_t *seq_out, uint64_t *off_out) {
    if (!tree || !off_out || (tree->tx_bases && !seq_out)) return fail(PFQ_ERR_ARG, "null argument");
    if (!tree->tx_have) return fail(PFQ_ERR_STATE, "pfq_debug_text_csr before a pfq_text_parse on this tree");
    PFQ_TRY(use_device(tree->device));
    const pfq_tree &t = *tree;
    if (t.tx_bases) HIP_TRY(hipMemcpy(seq_out, t.d_tx_seq[t.tx_sets.cur].p, t.tx_bases, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(off_out, t.d_tx_off[t.tx_sets.cur].p, (t.tx_records + 1) * 8, hipMemcpyDeviceToHost));
    return PFQ_OK;
}

// ---- blocked gzip ---------------------------------------------------------------------------------------------------------

// The header walk of pfq_gz_scan: begin and text_begin [n + 1]; for pfq_text_inflate also what the kernel needs per member and
// the trailers' CRCs.
static int gz_walk(const char *who, const uint8_t *gz, uint64_t len, uint64_t max_text, uint32_t flags, std::vector<uint64_t> &begin,
                   std::vector<uint64_t> &text_begin, std::vector<pfq::GzMember> *mem, std::vector<uint32_t> *crc, pfq_gz_members *out) {
    if (!out || (len && !gz)) return fail(PFQ_ERR_ARG, "null argument");
    if (flags & ~PFQ_TEXT_FINAL) return fail(PFQ_ERR_ARG, std::string(who) + ": unknown flag bits");
    if (max_text && max_text < PFQ_GZ_MEMBER_TEXT_MAX)
        return fail(PFQ_ERR_ARG, std::string(who) + ": max_text must be 0 or at least " + std::to_string(PFQ_GZ_MEMBER_TEXT_MAX) + ", not " + std::to_string(max_text));
    begin.assign(1, 0);
    text_begin.assign(1, 0);
    if (mem) mem->clear();
    if (crc) crc->clear();
    uint64_t p = 0, text = 0;
    uint32_t stop = PFQ_GZ_END;
    while (p < len) {
        pfq_inflate::Member m{};
        const pfq_inflate::Walk w = pfq_inflate::walk_member(gz + p, len - p, &m);
        if (w == pfq_inflate::WALK_SHORT) {
            stop = (flags & PFQ_TEXT_FINAL) ? PFQ_GZ_FOREIGN : PFQ_GZ_MORE;
            break;
        }
        if (w == pfq_inflate::WALK_FOREIGN) {
            stop = PFQ_GZ_FOREIGN;
            break;
        }
        if ((max_text && text + m.isize > max_text) || text + m.isize > 0x7fffffffull) {
            stop = PFQ_GZ_LIMIT;
            break;
        }
        if (mem) mem->push_back(pfq::GzMember{p + m.header, text, m.size - 8 - m.header, m.isize});
        if (crc) crc->push_back(m.crc);
        p += m.size;
        text += m.isize;
        begin.push_back(p);
        text_begin.push_back(text);
    }
    out->n_members = begin.size() - 1;
    out->consumed = p;
    out->text_bytes = text;
    out->stop = stop;
    out->begin = begin.data();
    out->text_begin = text_begin.data();
    return PFQ_OK;
}

thread_local std::vector<uint64_t> g_gz_begin, g_gz_text_begin;

int pfq_gz_scan(const uint8_t *gz, uint64_t len, uint64_t max_text, uint32_t flags, pfq_gz_members *out) {
    return gz_walk("pfq_gz_scan", gz, len, max_text, flags, g_gz_begin, g_gz_text_begin, nullptr, nullptr, out);
}

int pfq_text_inflate(pfq_tree *tree, const uint8_t *gz, uint64_t len, uint64_t max_text, uint32_t flags, pfq_text_inflated *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    pfq_tree &t = *tree;
    t.gz_have = false;
    std::vector<uint32_t> trailer_crc;
    PFQ_TRY(gz_walk("pfq_text_inflate", gz, len, max_text, flags, t.gz_begin, t.gz_text_begin, &t.gz_mem, &trailer_crc, &out->members));
    PFQ_TRY(use_device(t.device));
    PFQ_TRY(ensure_copy_stream(t));
    HIP_TRY(t.gz_time.ensure());
    hipStream_t st = t.copy_stream;
    const uint64_t n = out->members.n_members, consumed = out->members.consumed;
    t.gz_res.assign(2 * n, 0);
    t.gz_time.valid = false;
    if (n) {
        // (the kernel stages whole pieces of GZ_STAGE bytes: the allocation reaches beyond the last one it can touch)
        HIP_TRY(t.d_gz.ensure((consumed + pfq::GZ_STAGE - 1) / pfq::GZ_STAGE * pfq::GZ_STAGE + pfq::GZ_STAGE));
        HIP_TRY(t.d_gz_text.ensure(out->members.text_bytes + 16));
        HIP_TRY(t.d_gz_mem.ensure(n));
        HIP_TRY(t.d_gz_res.ensure(2 * n));
        long long blocks = t.knobs.inflate_blocks;
        if (blocks < 1 || blocks > 65535) {
            int cus = 0;
            HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t.device));
            blocks = 2 * std::max(cus, 1);
        }
        HIP_TRY(t.gz_time.mark(0, st));
        HIP_TRY(hipMemcpyAsync(t.d_gz.p, gz, consumed, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t.d_gz_mem.p, t.gz_mem.data(), n * sizeof(pfq::GzMember), hipMemcpyHostToDevice, st));
        HIP_TRY(t.gz_time.mark(1, st));
        pfq::launch_gz_inflate(t.d_gz.p, t.d_gz_mem.p, n, t.d_gz_text.p, t.d_gz_res.p, (uint32_t)blocks, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(t.gz_time.mark(2, st));
        HIP_TRY(hipMemcpyAsync(t.gz_res.data(), t.d_gz_res.p, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        t.gz_time.valid = true;
    }
    t.gz_status.resize(n);
    uint64_t good = n;
    for (uint64_t m = 0; m < n; m++) {
        uint32_t s = t.gz_res[2 * m];
        if (s > PFQ_GZ_LENGTH) s = PFQ_GZ_MALFORMED;  // (not a word the kernel writes)
        if (s == PFQ_GZ_OK && t.gz_res[2 * m + 1] != trailer_crc[m]) s = PFQ_GZ_CRC;
        t.gz_status[m] = (uint8_t)s;
        if (s != PFQ_GZ_OK && m < good) good = m;
    }
    out->n_good = good;
    out->good_text = t.gz_text_begin[good];
    out->status = t.gz_status.data();
    t.gz_good_text = out->good_text;
    t.gz_have = true;
    return PFQ_OK;
}

int pfq_text_parse_inflated(pfq_tree *tree, const uint8_t *carry, uint64_t carry_len, uint64_t limit, int format, uint32_t flags, pfq_text *out) {
    if (!tree || !out || (carry_len && !carry)) return fail(PFQ_ERR_ARG, "null argument");
    if (format != PFQ_TEXT_FASTA && format != PFQ_TEXT_FASTQ)
        return fail(PFQ_ERR_ARG, "pfq_text_parse_inflated: format must be PFQ_TEXT_FASTA or PFQ_TEXT_FASTQ");
    if (flags & ~(PFQ_TEXT_FINAL | PFQ_TEXT_WANT_RECORDS)) return fail(PFQ_ERR_ARG, "pfq_text_parse_inflated: unknown flag bits");
    if (!tree->gz_have) return fail(PFQ_ERR_STATE, "pfq_text_parse_inflated before a pfq_text_inflate on this tree");
    pfq_tree &t = *tree;
    if ((carry_len >> 31) || ((carry_len + t.gz_good_text) >> 31))
        return fail(PFQ_ERR_UNSUPPORTED, "pfq_text_parse_inflated: 2^31 bytes of text or more in one call (carry " + std::to_string(carry_len) +
                                             " + inflated " + std::to_string(t.gz_good_text) + "): inflate smaller chunks");
    PFQ_TRY(use_device(t.device));
    const uint32_t n = (uint32_t)(carry_len + t.gz_good_text), n_carry = (uint32_t)carry_len;
    int slot = 0;
    PFQ_TRY(text_parse_begin(t, n, &slot));
    hipStream_t st = t.copy_stream;
    uint8_t ends[2] = {0, 0};  // the text's first and last byte
    if (n) {
        if (n_carry) HIP_TRY(hipMemcpyAsync(t.d_tx_text.p, carry, n_carry, hipMemcpyHostToDevice, st));
        if (t.gz_good_text) HIP_TRY(hipMemcpyAsync(t.d_tx_text.p + n_carry, t.d_gz_text.p, t.gz_good_text, hipMemcpyDeviceToDevice, st));
        if (n_carry) {
            ends[0] = carry[0];
        } else {
            HIP_TRY(hipMemcpyAsync(&ends[0], t.d_gz_text.p, 1, hipMemcpyDeviceToHost, st));
        }
        if (t.gz_good_text) {
            HIP_TRY(hipMemcpyAsync(&ends[1], t.d_gz_text.p + t.gz_good_text - 1, 1, hipMemcpyDeviceToHost, st));
        } else {
            ends[1] = carry[n_carry - 1];
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    return text_parse_staged(t, slot, n, ends[0], ends[1], limit, format == PFQ_TEXT_FASTQ, (flags & PFQ_TEXT_FINAL) != 0,
                             (flags & PFQ_TEXT_WANT_RECORDS) != 0, out);
}

int pfq_text_read(pfq_tree *tree, uint64_t from, uint64_t n, uint8_t *dst) {
    if (!tree || (n && !dst)) return fail(PFQ_ERR_ARG, "null argument");
    if (!tree->tx_have) return fail(PFQ_ERR_STATE, "pfq_text_read before a pfq_text_parse or pfq_text_parse_inflated on this tree");
    if (from > tree->tx_len || n > tree->tx_len - from)
        return fail(PFQ_ERR_ARG, "pfq_text_read: bytes [" + std::to_string(from) + ", " + std::to_string(from) + " + " + std::to_string(n) +
                                     ") of a text of " + std::to_string(tree->tx_len) + " bytes");
    PFQ_TRY(use_device(tree->device));
    if (n) HIP_TRY(hipMemcpy(dst, tree->d_tx_text.p + from, n, hipMemcpyDeviceToHost));
    return PFQ_OK;
}

int pfq_debug_last_inflate(pfq_tree *tree, double *ms) {
    return last_stage_ms(tree, ms, &pfq_tree::gz_time, true,
                         "pfq_debug_last_inflate before a pfq_text_inflate with members on this tree");
}

// ---- text output ----------------------------------------------------------------------------------------------------------

static int deflate_device(pfq_tree &t, const uint8_t *d_text, const uint8_t *h_text, uint64_t len, const uint64_t *cuts, uint64_t n_cuts, int s,
                          pfq_bgzf *out);

// pfq_text_format, and pfq_text_format_gz where gz is given: the streams then stay on the device and are deflated there.
static int text_format(pfq_tree *tree, uint64_t first_index, uint32_t block, uint32_t flags, pfq_text_records *out, pfq_bgzf *const *gz) {
    if (!tree || !out || (gz && (!gz[0] || !gz[1]))) return fail(PFQ_ERR_ARG, "null argument");
    if (block < 1 || block > PFQ_FMT_BLOCK_MAX)
        return fail(PFQ_ERR_ARG, "pfq_text_format: block must be 1 .. " + std::to_string(PFQ_FMT_BLOCK_MAX) + ", not " + std::to_string(block));
    if (!(flags & (PFQ_FMT_POS | PFQ_FMT_NEG)) || (flags & ~(PFQ_FMT_POS | PFQ_FMT_NEG)))
        return fail(PFQ_ERR_ARG, "pfq_text_format: flags must be PFQ_FMT_POS, PFQ_FMT_NEG or both");
    pfq_tree &t = *tree;
    PFQ_TRY(insertion_error(t));
    if (t.is_shard)
        return fail(PFQ_ERR_UNSUPPORTED, "pfq_text_format on a subtree shard: a shard sees only its own leaves, so the rows it would print are partial");
    if (!t.tx_have) return fail(PFQ_ERR_STATE, "pfq_text_format before a pfq_text_parse on this tree");
    if (!t.fm_rows || t.fm_rows_leaves != t.leaves.size())
        return fail(PFQ_ERR_STATE, "pfq_text_format: the last query call on this tree was not a successful pfq_text_query of the parsed block with "
                                   "PFQ_WANT_HITS and without PFQ_PAIRED");
    PFQ_TRY(use_device(t.device));
    hipStream_t st = t.copy_stream;
    const uint32_t n = (uint32_t)t.tx_records;
    const size_t nl = t.leaves.size();
    // the whole result blocks of the call: records head .. head + n_whole * block - 1
    uint32_t head = (uint32_t)((block - first_index % block) % block);
    const uint32_t n_whole = head < n ? (n - head) / block : 0;
    if (!n_whole) head = n;
    for (auto &h : t.h_fm_out) HIP_TRY(h.ensure(1));
    *out = pfq_text_records{};
    out->n_records = n;
    out->pos = gz ? nullptr : t.h_fm_out[0].p;
    out->neg = gz ? nullptr : t.h_fm_out[1].p;
    t.out_fm_left.clear();
    out->left = t.out_fm_left.data();
    t.fm_time.valid = false;
    if (!n) {
        if (gz)
            for (int s = 0; s < 2; ++s) PFQ_TRY(deflate_device(t, nullptr, nullptr, 0, nullptr, 0, s, gz[s]));
        return PFQ_OK;
    }
    const bool timed = t.knobs.fmt_time == 1;
    if (timed)
        HIP_TRY(t.fm_time.ensure());
    {  // the leaves' names, uploaded when they are not the ones on the device
        std::vector<uint8_t> names;
        std::vector<uint32_t> name_off(1, 0);
        for (int32_t v : t.leaves) {
            const std::string &s = t.nodes[v].tax_id;
            names.insert(names.end(), s.begin(), s.end());
            name_off.push_back((uint32_t)names.size());
        }
        if (names.size() >> 31) return fail(PFQ_ERR_UNSUPPORTED, "pfq_text_format: 2^31 bytes of leaf names or more");
        if (!t.d_fm_name_off.p || names != t.fm_names || name_off != t.fm_name_off) {
            HIP_TRY(hipStreamSynchronize(st));
            HIP_TRY(t.d_fm_names.ensure(names.size() + 16));
            HIP_TRY(t.d_fm_name_off.ensure(name_off.size()));
            if (!names.empty()) HIP_TRY(hipMemcpy(t.d_fm_names.p, names.data(), names.size(), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t.d_fm_name_off.p, name_off.data(), name_off.size() * 4, hipMemcpyHostToDevice));
            t.fm_names.swap(names);
            t.fm_name_off.swap(name_off);
        }
    }
    HIP_TRY(t.d_fm_idb.ensure(n));
    HIP_TRY(t.d_fm_idl.ensure(n));
    HIP_TRY(t.d_fm_hash.ensure(n));
    HIP_TRY(t.d_fm_long.ensure(n));
    HIP_TRY(t.d_fm_sums.ensure((size_t)n / 4096 + 2));
    for (int s = 0; s < 2; ++s) {
        HIP_TRY(t.d_fm_len[s].ensure(n));
        HIP_TRY(t.d_fm_dst[s].ensure((size_t)n + 1));
    }
    const size_t n_bounds = 2 * ((size_t)n_whole + 2), n_small = pfq::FMT_RES_N + n_bounds + ((size_t)n_whole + 1) / 2;
    HIP_TRY(t.d_fm_small.ensure(n_small));
    HIP_TRY(t.h_fm_small.ensure(n_small));
    HIP_TRY(hipMemsetAsync(t.d_fm_small.p, 0, n_small * 8, st));
    pfq::FmtArgs a{};
    a.text = t.d_tx_text.p;
    a.line_start = t.d_tx_line.p;
    a.rec_line = t.d_tx_rec_line.p;
    a.fastq = t.tx_fastq;
    a.n = n;
    a.head = head;
    a.block = block;
    a.n_whole = n_whole;
    a.flags = flags;
    a.hash_bits = t.knobs.fmt_hash_bits >= 1 && t.knobs.fmt_hash_bits <= 64 ? (uint32_t)t.knobs.fmt_hash_bits : 64u;
    a.grid = t.knobs.fmt_grid >= 1 && t.knobs.fmt_grid <= 65535 ? (uint32_t)t.knobs.fmt_grid : 0u;
    a.seq = t.d_tx_seq[t.tx_sets.cur].p;
    a.seq_off = t.d_tx_off[t.tx_sets.cur].p;
    a.row_off = t.d_hit_off.p;
    a.row_leaves = t.d_hit_leaves.p;
    a.names = t.d_fm_names.p;
    a.name_off = t.d_fm_name_off.p;
    a.id_beg = t.d_fm_idb.p;
    a.id_len = t.d_fm_idl.p;
    a.hash = t.d_fm_hash.p;
    a.res = t.d_fm_small.p;
    a.bounds = a.res + pfq::FMT_RES_N;
    a.state = reinterpret_cast<uint32_t *>(a.bounds + n_bounds);
    a.long_list = t.d_fm_long.p;
    for (int s = 0; s < 2; ++s) {
        a.len[s] = t.d_fm_len[s].p;
        a.dst[s] = t.d_fm_dst[s].p;
    }
    if (timed) HIP_TRY(t.fm_time.mark(0, st));
    pfq::launch_fmt_ids(a, st);
    if (timed) HIP_TRY(t.fm_time.mark(1, st));
    pfq::launch_fmt_sizes(a, nl > 64, st);
    for (int s = 0; s < 2; ++s) pfq::launch_scan_u32(a.len[s], n, t.d_fm_sums.p, t.d_fm_dst[s].p, st);
    pfq::launch_fmt_bounds(a, st);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(t.fm_time.mark(2, st));
    HIP_TRY(hipMemcpyAsync(t.h_fm_small.p, t.d_fm_small.p, n_small * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the totals size the streams)
    const unsigned long long *res = t.h_fm_small.p, *bounds = res + pfq::FMT_RES_N;
    const uint32_t *state = reinterpret_cast<const uint32_t *>(bounds + n_bounds);
    if (res[pfq::FMT_RES_ERR]) return fail(PFQ_ERR_UNSUPPORTED, "pfq_text_format: a record whose output would be 2^32 bytes or more");
    const uint64_t total[2] = {bounds[2 * ((size_t)n_whole + 1)], bounds[2 * ((size_t)n_whole + 1) + 1]};
    for (int s = 0; s < 2; ++s) {
        HIP_TRY(t.d_fm_out[s].ensure(total[s] + 16));
        if (!gz) HIP_TRY(t.h_fm_out[s].ensure(total[s] + 1));
        a.out[s] = t.d_fm_out[s].p;
    }
    pfq::launch_fmt_emit(a, st);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(t.fm_time.mark(3, st));
    for (int s = 0; s < 2; ++s)
        if (total[s] && !gz) HIP_TRY(hipMemcpyAsync(t.h_fm_out[s].p, t.d_fm_out[s].p, total[s], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    t.fm_time.valid = timed;
    // the left runs, from the block states
    if (head) t.out_fm_left.push_back(pfq_text_left{0, head, 0, 0, PFQ_LEFT_HEAD, 0});
    for (uint32_t b = 0; b < n_whole; ++b)
        if (state[b])
            t.out_fm_left.push_back(pfq_text_left{head + (uint64_t)b * block, block, bounds[2 * (size_t)b], bounds[2 * (size_t)b + 1], PFQ_LEFT_REPEATED_ID, 0});
    const uint64_t tail = head + (uint64_t)n_whole * block;
    if (tail < n) t.out_fm_left.push_back(pfq_text_left{tail, n - tail, bounds[2 * (size_t)n_whole], bounds[2 * (size_t)n_whole + 1], PFQ_LEFT_TAIL, 0});
    out->pos_records = res[pfq::FMT_RES_POS_RECORDS];
    out->neg_records = res[pfq::FMT_RES_NEG_RECORDS];
    out->pos_bytes = total[0];
    out->neg_bytes = total[1];
    out->pos = gz ? nullptr : t.h_fm_out[0].p;
    out->neg = gz ? nullptr : t.h_fm_out[1].p;
    out->n_left = t.out_fm_left.size();
    out->left = t.out_fm_left.data();
    if (gz) {  // each stream cut where the caller's own bytes for the left runs belong
        std::vector<uint64_t> cuts(t.out_fm_left.size());
        for (int s = 0; s < 2; ++s) {
            for (size_t i = 0; i < cuts.size(); ++i) cuts[i] = s ? t.out_fm_left[i].neg_at : t.out_fm_left[i].pos_at;
            PFQ_TRY(deflate_device(t, t.d_fm_out[s].p, nullptr, total[s], cuts.data(), cuts.size(), s, gz[s]));
        }
    }
    return PFQ_OK;
}

int pfq_text_format(pfq_tree *tree, uint64_t first_index, uint32_t block, uint32_t flags, pfq_text_records *out) {
    return text_format(tree, first_index, block, flags, out, nullptr);
}

// ---- blocked gzip written on the device ---------------------------------------------------------------------------------------

// text[0, len) on the device (h_text: copied there first) cut, deflated and gathered into stream s's buffers.
static int deflate_device(pfq_tree &t, const uint8_t *d_text, const uint8_t *h_text, uint64_t len, const uint64_t *cuts, uint64_t n_cuts, int s,
                          pfq_bgzf *out) {
    std::vector<uint64_t> &piece_begin = t.df_piece_begin[s], &member_begin = t.df_member_begin[s];
    t.df_mem.clear();
    piece_begin.assign(n_cuts + 2, 0);  // first as the first member of every piece, below as its offset
    for (uint64_t piece = 0; piece <= n_cuts; ++piece) {
        const uint64_t from = piece ? cuts[piece - 1] : 0, to = piece < n_cuts ? cuts[piece] : len;
        piece_begin[piece] = t.df_mem.size();
        for (uint64_t at = from; at < to; at += PFQ_BGZF_MEMBER_TEXT)
            t.df_mem.push_back(pfq::BgzfMember{at, (uint32_t)std::min<uint64_t>(PFQ_BGZF_MEMBER_TEXT, to - at), (uint32_t)piece});
    }
    const uint64_t n = t.df_mem.size();
    piece_begin[n_cuts + 1] = n;
    member_begin.assign(n + 1, 0);
    HIP_TRY(t.h_df_gz[s].ensure(1));
    *out = pfq_bgzf{};
    out->n_members = n;
    out->n_pieces = n_cuts + 1;
    if (n) {
        PFQ_TRY(ensure_copy_stream(t));
        HIP_TRY(t.df_time.ensure());
        hipStream_t st = t.copy_stream;
        long long blocks = t.knobs.deflate_blocks;
        if (blocks < 1 || blocks > 65535) {
            int cus = 0;
            HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t.device));
            blocks = std::max(cus, 1);
        }
        const uint64_t grid = std::min<uint64_t>(n, (uint64_t)blocks);
        if (h_text) {
            HIP_TRY(t.d_df_text.ensure(len + 32));
            d_text = t.d_df_text.p;
        }
        HIP_TRY(t.d_df_mem.ensure(n));
        HIP_TRY(t.d_df_tokens.ensure(grid * pfq::BGZF_TOKENS));
        HIP_TRY(t.d_df_slots.ensure(n * pfq::BGZF_SLOT));
        HIP_TRY(t.d_df_sizes.ensure(n));
        HIP_TRY(t.d_df_off.ensure(n + 1));
        HIP_TRY(t.d_df_sums.ensure(n / 4096 + 2));
        HIP_TRY(t.d_df_gz[s].ensure(len + 31 * n + 16));
        HIP_TRY(t.h_df_off.ensure(n + 1));
        t.df_time.valid = false;
        HIP_TRY(t.df_time.mark(0, st));
        if (h_text) HIP_TRY(hipMemcpyAsync(t.d_df_text.p, h_text, len, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t.d_df_mem.p, t.df_mem.data(), n * sizeof(pfq::BgzfMember), hipMemcpyHostToDevice, st));
        HIP_TRY(t.df_time.mark(1, st));
        pfq::launch_bgzf_deflate(d_text, t.d_df_mem.p, n, t.d_df_tokens.p, t.d_df_slots.p, t.d_df_sizes.p, (uint32_t)blocks, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(t.df_time.mark(2, st));
        pfq::launch_scan_u32(t.d_df_sizes.p, n, t.d_df_sums.p, t.d_df_off.p, st);
        pfq::launch_bgzf_gather(t.d_df_slots.p, t.d_df_off.p, n, t.d_df_gz[s].p, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(t.h_df_off.p, t.d_df_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));  // (the total sizes the copy)
        const uint64_t total = t.h_df_off.p[n];
        if (total > len + 31 * n) return fail(PFQ_ERR_DEVICE, "deflate: members of " + std::to_string(total) + " bytes for " + std::to_string(len) + " of text");
        HIP_TRY(t.h_df_gz[s].ensure(total + 1));
        HIP_TRY(hipMemcpyAsync(t.h_df_gz[s].p, t.d_df_gz[s].p, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(t.df_time.mark(3, st));
        HIP_TRY(hipStreamSynchronize(st));
        t.df_time.valid = true;
        for (uint64_t m = 0; m <= n; ++m) member_begin[m] = t.h_df_off.p[m];
        out->gz_bytes = total;
    }
    for (uint64_t piece = 0; piece <= n_cuts + 1; ++piece) piece_begin[piece] = member_begin[piece_begin[piece]];
    out->gz = t.h_df_gz[s].p;
    out->piece_begin = piece_begin.data();
    out->member_begin = member_begin.data();
    return PFQ_OK;
}

int pfq_bgzf_deflate(pfq_tree *tree, const uint8_t *text, uint64_t len, const uint64_t *cuts, uint64_t n_cuts, pfq_bgzf *out) {
    if (!tree || !out || (len && !text) || (n_cuts && !cuts)) return fail(PFQ_ERR_ARG, "null argument");
    for (uint64_t i = 0; i < n_cuts; ++i)
        if (cuts[i] > len || (i && cuts[i] < cuts[i - 1]))
            return fail(PFQ_ERR_ARG, "pfq_bgzf_deflate: cut " + std::to_string(i) + " (" + std::to_string(cuts[i]) + ") is not ascending or lies beyond the text's " +
                                         std::to_string(len) + " bytes");
    if (len >> 31) return fail(PFQ_ERR_UNSUPPORTED, "pfq_bgzf_deflate: 2^31 bytes of text or more in one call: deflate smaller chunks");
    PFQ_TRY(use_device(tree->device));
    return deflate_device(*tree, nullptr, text, len, cuts, n_cuts, 0, out);
}

int pfq_text_format_gz(pfq_tree *tree, uint64_t first_index, uint32_t block, uint32_t flags, pfq_text_records *out, pfq_bgzf *pos_gz, pfq_bgzf *neg_gz) {
    pfq_bgzf *const gz[2] = {pos_gz, neg_gz};
    return text_format(tree, first_index, block, flags, out, gz);
}

int pfq_debug_last_deflate(pfq_tree *tree, double *ms) {
    return last_stage_ms(tree, ms, &pfq_tree::df_time, true,
                         "pfq_debug_last_deflate before a deflate call with members on this tree");
}

int pfq_debug_last_format(pfq_tree *tree, double *ms) {
    return last_stage_ms(tree, ms, &pfq_tree::fm_time, true,
                         "pfq_debug_last_format before a pfq_text_format with records and PFQ_FMT_TIME=1 on this tree");
}

// ---- read preprocessing ----------------------------------------------------------------------------------------------------

int pfq_prep_reads(pfq_tree *tree, const uint8_t *seq, const uint8_t *qual, const uint64_t *offsets, const uint8_t *has_qual, uint64_t n_reads,
                   const pfq_prep_params *params, pfq_prep *out) {
    if (!tree || !params || !out || (n_reads && (!seq || !offsets))) return fail(PFQ_ERR_ARG, "null argument");
    const pfq_prep_params &pr = *params;
    if (pr.flags & ~(PFQ_PREP_PAIRED | PFQ_PREP_WANT_READS)) return fail(PFQ_ERR_ARG, "pfq_prep_reads: unknown flag bits");
    if (pr.trim_quality > 93) return fail(PFQ_ERR_ARG, "pfq_prep_reads: trim_quality must be 0 (off) or 1 .. 93, not " + std::to_string(pr.trim_quality));
    if (pr.trim_window < 1 || pr.trim_window > 1024) return fail(PFQ_ERR_ARG, "pfq_prep_reads: trim_window must be 1 .. 1024, not " + std::to_string(pr.trim_window));
    if (pr.min_complexity > 100) return fail(PFQ_ERR_ARG, "pfq_prep_reads: min_complexity must be 0 (off) or 1 .. 100, not " + std::to_string(pr.min_complexity));
    const bool paired = (pr.flags & PFQ_PREP_PAIRED) != 0, want_reads = (pr.flags & PFQ_PREP_WANT_READS) != 0;
    if (paired && (n_reads & 1)) return fail(PFQ_ERR_ARG, "PFQ_PREP_PAIRED needs an even number of reads (mates 2i, 2i + 1)");
    const bool overlap = paired && tree->ov_on;  // (the mate overlap step needs mates)
    const bool correct = overlap && tree->mc_high > 0;  // (the correction is part of that step)
    constexpr size_t at_ctot = pfq::PREP_TOT_N + 1 + pfq::ADAPT_TOT_N + pfq::OVL_TOT_N + pfq::OVL_HIST;  // in h_pp_tot; the patches' number behind
    constexpr size_t n_otot = pfq::OVL_TOT_N + pfq::OVL_HIST;
    if (n_reads >= (1ull << 31) - 1024) return fail(PFQ_ERR_UNSUPPORTED, "pfq_prep_reads: 2^31 - 1024 reads or more in one block: ask in pieces");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(ensure_copy_stream(t));
    HIP_TRY(t.pp_ready.ensure(hipEventDisableTiming));
    HIP_TRY(t.pp_sets.ensure());
    HIP_TRY(t.pp_time.ensure());
    HIP_TRY(t.ad_time.ensure());
    HIP_TRY(t.ov_time.ensure());
    HIP_TRY(t.mc_time.ensure());
    HIP_TRY(t.h_pp_tot.ensure(at_ctot + pfq::COR_TOT_N + 1));
    HIP_TRY(t.d_pp_tot.ensure(pfq::PREP_TOT_N));
    const bool adapters = t.ad_on;
    t.ad_last = false;
    t.ov_last = false;
    t.mc_last = false;
    uint64_t n_patches = 0;
    hipStream_t st = t.copy_stream;
    const int slot = t.pp_sets.other();
    HIP_TRY(t.pp_sets.wait(slot));  // the classification that read this set is done
    t.pp_have = false;  // (until this prep has succeeded there is no block to query)
    const uint64_t total = n_reads ? offsets[n_reads] : 0;
    *out = pfq_prep{};
    out->n_reads = n_reads;
    HIP_TRY(t.d_pp_seq[slot].ensure(total + 16));
    HIP_TRY(t.d_pp_off[slot].ensure(n_reads + 1));
    uint64_t n_kept = 0;
    if (!n_reads) {
        HIP_TRY(hipMemsetAsync(t.d_pp_off[slot].p, 0, 8, st));
    } else {
        HIP_TRY(t.d_pp_in.ensure(total + 16));
        HIP_TRY(t.d_pp_inoff.ensure(n_reads + 1));
        if (qual) HIP_TRY(t.d_pp_qual.ensure(total + 16));
        if (qual && has_qual) HIP_TRY(t.d_pp_hq.ensure(n_reads));
        for (DevBuf<uint32_t> *b : {&t.d_pp_begin, &t.d_pp_len, &t.d_pp_reason, &t.d_pp_keep, &t.d_pp_klen, &t.d_pp_kept}) HIP_TRY(b->ensure(n_reads));
        HIP_TRY(t.d_pp_kpos.ensure(n_reads + 1));
        HIP_TRY(t.d_pp_koff.ensure(n_reads + 1));
        HIP_TRY(t.d_pp_sums.ensure(n_reads / 4096 + 2));
        if (total) HIP_TRY(hipMemcpyAsync(t.d_pp_in.p, seq, total, hipMemcpyHostToDevice, st));
        if (total && qual) HIP_TRY(hipMemcpyAsync(t.d_pp_qual.p, qual, total, hipMemcpyHostToDevice, st));
        if (qual && has_qual) HIP_TRY(hipMemcpyAsync(t.d_pp_hq.p, has_qual, n_reads, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t.d_pp_inoff.p, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(t.d_pp_tot.p, 0, pfq::PREP_TOT_N * 8, st));
        pfq::PrepArgs a{};
        a.seq = t.d_pp_in.p;
        a.qual = qual ? t.d_pp_qual.p : nullptr;
        a.off = t.d_pp_inoff.p;
        a.has_qual = (qual && has_qual) ? t.d_pp_hq.p : nullptr;
        a.n_reads = n_reads;
        a.trim_quality = pr.trim_quality;
        a.trim_window = pr.trim_window;
        a.poly_x = pr.poly_x;
        a.min_length = pr.min_length;
        a.max_n = pr.max_n;
        a.min_complexity = pr.min_complexity;
        a.paired = paired ? 1u : 0u;
        a.begin = t.d_pp_begin.p;
        a.len = t.d_pp_len.p;
        a.reason = t.d_pp_reason.p;
        a.keep = t.d_pp_keep.p;
        a.klen = t.d_pp_klen.p;
        a.totals = t.d_pp_tot.p;
        a.kpos = t.d_pp_kpos.p;
        a.koff = t.d_pp_koff.p;
        a.kept = t.d_pp_kept.p;
        a.csr_off = t.d_pp_off[slot].p;
        a.out = t.d_pp_seq[slot].p;
        if (adapters) {  // cut[] first: the steps below then see every read cut there
            HIP_TRY(t.d_pp_cut.ensure(n_reads));
            HIP_TRY(t.d_pp_which.ensure(n_reads));
            HIP_TRY(t.d_pp_atot.ensure(pfq::ADAPT_TOT_N));
            HIP_TRY(hipMemsetAsync(t.d_pp_atot.p, 0, pfq::ADAPT_TOT_N * 8, st));
            pfq::AdaptArgs ad{};
            ad.seq = a.seq;
            ad.off = a.off;
            ad.n_reads = n_reads;
            ad.paired = a.paired;
            ad.cut = t.d_pp_cut.p;
            ad.which = t.d_pp_which.p;
            ad.totals = t.d_pp_atot.p;
            ad.set = t.ad_set;
            HIP_TRY(t.ad_time.mark(0, st));
            pfq::launch_prep_adapter(ad, st);
            HIP_TRY(t.ad_time.mark(1, st));
            a.cut = t.d_pp_cut.p;
        }
        if (overlap) {  // behind the adapter step: the cut the steps below see is the smaller of the two
            HIP_TRY(t.d_pp_oins.ensure(n_reads / 2));
            HIP_TRY(t.d_pp_omm.ensure(n_reads / 2));
            HIP_TRY(t.d_pp_ecut.ensure(n_reads));
            HIP_TRY(t.d_pp_otot.ensure(n_otot));
            HIP_TRY(hipMemsetAsync(t.d_pp_otot.p, 0, n_otot * 8, st));
            pfq::OverlapArgs ov{};
            ov.seq = a.seq;
            ov.off = a.off;
            ov.n_reads = n_reads;
            ov.min_overlap = t.ov_min_overlap;
            ov.max_error_percent = t.ov_max_error_percent;
            ov.adapter_cut = adapters ? t.d_pp_cut.p : nullptr;
            ov.insert = t.d_pp_oins.p;
            ov.mismatches = t.d_pp_omm.p;
            ov.cut = t.d_pp_ecut.p;
            ov.totals = t.d_pp_otot.p;
            if (correct) {  // (the adapter kernel, launched above, has read the reads as they came)
                HIP_TRY(t.d_pp_ctot.ensure(pfq::COR_TOT_N));
                HIP_TRY(hipMemsetAsync(t.d_pp_ctot.p, 0, pfq::COR_TOT_N * 8, st));
                ov.cor_high = t.mc_high;
                ov.cor_low = t.mc_low;
                ov.cor_seq = t.d_pp_in.p;
                ov.cor_qual = qual ? t.d_pp_qual.p : nullptr;
                ov.has_qual = a.has_qual;
                ov.cor_totals = t.d_pp_ctot.p;
                if (want_reads) {  // the kernel counts, launch_prep_patches below lists and corrects
                    HIP_TRY(t.d_pp_ccnt.ensure(n_reads / 2));
                    HIP_TRY(t.d_pp_cat.ensure(n_reads / 2 + 1));
                    HIP_TRY(hipMemsetAsync(t.d_pp_ccnt.p, 0, n_reads / 2 * 4, st));
                    ov.cor_count = t.d_pp_ccnt.p;
                }
            }
            HIP_TRY(t.ov_time.mark(0, st));
            pfq::launch_prep_overlap(ov, st);
            HIP_TRY(t.ov_time.mark(1, st));
            if (correct && want_reads) {
                // the list's length decides its buffer, so the host waits for it here: once more than a call without the list
                HIP_TRY(t.mc_time.mark(0, st));
                pfq::launch_scan_u32(t.d_pp_ccnt.p, n_reads / 2, t.d_pp_sums.p, t.d_pp_cat.p, st);
                HIP_TRY(hipMemcpyAsync(t.h_pp_tot.p + at_ctot + pfq::COR_TOT_N, t.d_pp_cat.p + n_reads / 2, 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                n_patches = t.h_pp_tot.p[at_ctot + pfq::COR_TOT_N];
                if (n_patches) {
                    HIP_TRY(t.d_pp_patch.ensure(n_patches));
                    ov.cor_at = t.d_pp_cat.p;
                    ov.patches = t.d_pp_patch.p;
                    pfq::launch_prep_patches(ov, st);
                }
                HIP_TRY(t.mc_time.mark(1, st));
            }
            a.cut = t.d_pp_ecut.p;
        }
        HIP_TRY(t.pp_time.mark(0, st));
        pfq::launch_prep_trim(a, st);
        pfq::launch_prep_mark(a, st);
        HIP_TRY(t.pp_time.mark(1, st));
        pfq::launch_scan_u32(t.d_pp_keep.p, n_reads, t.d_pp_sums.p, t.d_pp_kpos.p, st);
        pfq::launch_scan_u32(t.d_pp_klen.p, n_reads, t.d_pp_sums.p, t.d_pp_koff.p, st);
        HIP_TRY(t.pp_time.mark(2, st));
        pfq::launch_prep_gather(a, st);
        HIP_TRY(t.pp_time.mark(3, st));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(t.h_pp_tot.p, t.d_pp_tot.p, pfq::PREP_TOT_N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(t.h_pp_tot.p + pfq::PREP_TOT_N, t.d_pp_kpos.p + n_reads, 8, hipMemcpyDeviceToHost, st));
        if (adapters) HIP_TRY(hipMemcpyAsync(t.h_pp_tot.p + pfq::PREP_TOT_N + 1, t.d_pp_atot.p, pfq::ADAPT_TOT_N * 8, hipMemcpyDeviceToHost, st));
        if (overlap) HIP_TRY(hipMemcpyAsync(t.h_pp_tot.p + pfq::PREP_TOT_N + 1 + pfq::ADAPT_TOT_N, t.d_pp_otot.p, n_otot * 8, hipMemcpyDeviceToHost, st));
        if (correct) HIP_TRY(hipMemcpyAsync(t.h_pp_tot.p + at_ctot, t.d_pp_ctot.p, pfq::COR_TOT_N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));  // (the caller's buffers are free from here)
        t.pp_time.valid = true;
        t.ad_time.valid = adapters;
        t.ov_time.valid = overlap;
        t.mc_time.valid = correct && want_reads;
        if (t.h_pp_tot.p[pfq::PREP_TOT_ERR])
            return fail(PFQ_ERR_UNSUPPORTED, "pfq_prep_reads: a read of 2^32 bases or more (or offsets that do not ascend)");
        n_kept = t.h_pp_tot.p[pfq::PREP_TOT_N];
        for (int c = 0; c < 5; ++c) out->n_reason[c] = t.h_pp_tot.p[pfq::PREP_TOT_REASON + c];
        out->bases_in = t.h_pp_tot.p[pfq::PREP_TOT_BASES_IN];
        out->bases_kept = t.h_pp_tot.p[pfq::PREP_TOT_BASES_KEPT];
        out->n_trimmed = t.h_pp_tot.p[pfq::PREP_TOT_TRIMMED];
    }
    out->n_kept = n_kept;
    if (want_reads) {
        t.out_pp_begin.resize(std::max<uint64_t>(n_reads, 1));  // (never NULL with the flag)
        t.out_pp_len.resize(std::max<uint64_t>(n_reads, 1));
        t.out_pp_reason.resize(std::max<uint64_t>(n_reads, 1));
        t.out_pp_kept.resize(std::max<uint64_t>(n_kept, 1));
        if (n_reads) {
            HIP_TRY(hipMemcpyAsync(t.out_pp_begin.data(), t.d_pp_begin.p, n_reads * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(t.out_pp_len.data(), t.d_pp_len.p, n_reads * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(t.out_pp_reason.data(), t.d_pp_reason.p, n_reads * 4, hipMemcpyDeviceToHost, st));
        }
        if (n_kept) HIP_TRY(hipMemcpyAsync(t.out_pp_kept.data(), t.d_pp_kept.p, n_kept * 4, hipMemcpyDeviceToHost, st));
        if (adapters) {
            t.out_pp_cut.resize(std::max<uint64_t>(n_reads, 1));
            t.out_pp_which.resize(std::max<uint64_t>(n_reads, 1));
            if (n_reads) {
                HIP_TRY(hipMemcpyAsync(t.out_pp_cut.data(), t.d_pp_cut.p, n_reads * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(t.out_pp_which.data(), t.d_pp_which.p, n_reads, hipMemcpyDeviceToHost, st));
            }
        }
    }
    if (overlap) {
        if (want_reads) {
            t.out_ov_insert.resize(std::max<uint64_t>(n_reads / 2, 1));
            t.out_ov_mm.resize(std::max<uint64_t>(n_reads / 2, 1));
            if (n_reads) {
                HIP_TRY(hipMemcpyAsync(t.out_ov_insert.data(), t.d_pp_oins.p, n_reads / 2 * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(t.out_ov_mm.data(), t.d_pp_omm.p, n_reads / 2 * 4, hipMemcpyDeviceToHost, st));
            }
        }
        t.ov_out = pfq_prep_overlap{};
        t.ov_out.n_fragments = n_reads / 2;
        t.out_ov_hist.assign(pfq::OVL_HIST, 0);
        if (n_reads) {
            const unsigned long long *ot = t.h_pp_tot.p + pfq::PREP_TOT_N + 1 + pfq::ADAPT_TOT_N;
            t.ov_out.n_analysed = ot[pfq::OVL_TOT_ANALYSED];
            t.ov_out.n_skipped = ot[pfq::OVL_TOT_SKIPPED];
            t.ov_out.n_overlapped = ot[pfq::OVL_TOT_FOUND];
            t.ov_out.n_readthrough = ot[pfq::OVL_TOT_THROUGH];
            t.ov_out.reads_cut = ot[pfq::OVL_TOT_READS];
            t.ov_out.bases_cut = ot[pfq::OVL_TOT_BASES];
            for (uint32_t i = 0; i < pfq::OVL_HIST; ++i) t.out_ov_hist[i] = ot[pfq::OVL_TOT_N + i];
        }
    }
    if (correct) {
        t.mc_out = pfq_prep_corrections{};
        if (want_reads) {
            t.out_mc_patch.resize(std::max<uint64_t>(n_patches, 1));  // (never NULL with the flag)
            if (n_patches) HIP_TRY(hipMemcpyAsync(t.out_mc_patch.data(), t.d_pp_patch.p, n_patches * sizeof(pfq_prep_patch), hipMemcpyDeviceToHost, st));
            t.mc_out.n_patches = n_patches;
        }
        if (n_reads) {
            const unsigned long long *ct = t.h_pp_tot.p + at_ctot;
            t.mc_out.n_fragments_corrected = ct[pfq::COR_TOT_FRAGMENTS];
            t.mc_out.n_bases[0] = ct[pfq::COR_TOT_BASES];
            t.mc_out.n_bases[1] = ct[pfq::COR_TOT_BASES + 1];
            t.mc_out.n_unresolved = ct[pfq::COR_TOT_UNRESOLVED];
            t.mc_out.n_no_quality = ct[pfq::COR_TOT_NO_QUALITY];
        }
    }
    if (adapters) {
        t.ad_out = pfq_prep_adapters{};
        t.ad_out.n_reads = n_reads;
        if (n_reads) {
            const unsigned long long *at = t.h_pp_tot.p + pfq::PREP_TOT_N + 1;
            t.ad_out.n_found = at[pfq::ADAPT_TOT_FOUND];
            t.ad_out.bases_cut = at[pfq::ADAPT_TOT_BASES];
            for (uint32_t i = 0; i < 2 * PFQ_ADAPTER_MAX; ++i) t.ad_out.found[i] = at[pfq::ADAPT_TOT_WHICH + i];
        }
    }
    HIP_TRY(hipEventRecord(t.pp_ready, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (want_reads) {
        out->begin = t.out_pp_begin.data();
        out->len = t.out_pp_len.data();
        out->reason = t.out_pp_reason.data();
        out->kept = t.out_pp_kept.data();
    }
    t.pp_sets.cur = slot;
    t.pp_kept = n_kept;
    t.pp_bases = out->bases_kept;
    t.pp_paired = paired;
    t.pp_have = true;
    t.pp_reads = n_reads;
    t.pp_want_reads = want_reads;
    t.dp_have = false;
    t.ad_last = adapters;
    t.ad_last_reads = adapters && want_reads;
    t.ov_last = overlap;
    t.ov_last_reads = overlap && want_reads;
    t.mc_last = correct;
    t.mc_last_reads = correct && want_reads;
    return PFQ_OK;
}

// ---- adapters ----------------------------------------------------------------------------------------------------------------

int pfq_tree_set_adapters(pfq_tree *tree, const char *const *set1, uint32_t n1, const char *const *set2, uint32_t n2, uint32_t min_overlap,
                          uint32_t max_error_percent) {
    if (!tree || (n1 && !set1) || (n2 && !set2)) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(insertion_error(*tree));
    pfq_tree &t = *tree;
    if (n1 == 0 && n2 == 0) {
        t.ad_on = false;
        t.ad_set = pfq::AdaptSet{};
        return PFQ_OK;
    }
    if (n1 == 0) return fail(PFQ_ERR_ARG, "pfq_tree_set_adapters: set 2 has " + std::to_string(n2) + " adapters but set 1 is empty (second mates fall back to set 1, not the reverse)");
    if (min_overlap < 1 || min_overlap > PFQ_ADAPTER_LEN_MAX)
        return fail(PFQ_ERR_ARG, "pfq_tree_set_adapters: min_overlap must be 1 .. " + std::to_string(PFQ_ADAPTER_LEN_MAX) + ", not " + std::to_string(min_overlap));
    if (max_error_percent > 50) return fail(PFQ_ERR_ARG, "pfq_tree_set_adapters: max_error_percent must be 0 .. 50, not " + std::to_string(max_error_percent));
    pfq::AdaptSet s{};
    s.min_overlap = min_overlap;
    s.max_error_percent = max_error_percent;
    const char *const *sets[2] = {set1, set2};
    const uint32_t ns[2] = {n1, n2};
    for (uint32_t k = 0; k < 2; ++k) {
        const std::string set_name = "set " + std::to_string(k + 1);
        if (ns[k] > PFQ_ADAPTER_MAX)
            return fail(PFQ_ERR_ARG, "pfq_tree_set_adapters: " + set_name + " has " + std::to_string(ns[k]) + " adapters, at most " + std::to_string(PFQ_ADAPTER_MAX));
        s.n[k] = ns[k];
        for (uint32_t i = 0; i < ns[k]; ++i) {
            const std::string name = "adapter " + std::to_string(i) + " of " + set_name;
            const char *seq = sets[k][i];
            if (!seq) return fail(PFQ_ERR_ARG, "pfq_tree_set_adapters: " + name + " is NULL");
            const size_t m = strnlen(seq, PFQ_ADAPTER_LEN_MAX + 1);
            const std::string shown = " '" + std::string(seq, std::min<size_t>(m, PFQ_ADAPTER_LEN_MAX)) + (m > PFQ_ADAPTER_LEN_MAX ? "..." : "") + "'";
            if (m < min_overlap || m > PFQ_ADAPTER_LEN_MAX)
                return fail(PFQ_ERR_ARG, "pfq_tree_set_adapters: " + name + shown + " must have min_overlap = " + std::to_string(min_overlap) + " .. " +
                                             std::to_string(PFQ_ADAPTER_LEN_MAX) + " bases");
            const uint32_t at = k * pfq::ADAPT_MAX + i;
            s.len[at] = (uint8_t)m;
            for (size_t j = 0; j < m; ++j) {
                const uint32_t u = (uint8_t)seq[j] & 0xDFu;
                if (u != 'A' && u != 'C' && u != 'G' && u != 'T')
                    return fail(PFQ_ERR_ARG, "pfq_tree_set_adapters: " + name + shown + " has a letter other than ACGT at position " + std::to_string(j));
                s.code[at][j >> 4] |= ((u >> 1) & 3u) << (2u * (j & 15u));
            }
        }
    }
    t.ad_set = s;
    t.ad_on = true;
    return PFQ_OK;
}

int pfq_prep_last_adapters(pfq_tree *tree, pfq_prep_adapters *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    if (!tree->pp_have) return fail(PFQ_ERR_STATE, "pfq_prep_last_adapters before a pfq_prep_reads on this tree");
    if (!tree->ad_last) return fail(PFQ_ERR_STATE, "pfq_prep_last_adapters: the last pfq_prep_reads on this tree ran without adapters (pfq_tree_set_adapters)");
    *out = tree->ad_out;
    if (tree->ad_last_reads) {
        out->cut = tree->out_pp_cut.data();
        out->which = tree->out_pp_which.data();
    }
    return PFQ_OK;
}

int pfq_debug_last_adapters(pfq_tree *tree, double *ms) {
    return last_stage_ms(tree, ms, &pfq_tree::ad_time, tree && tree->pp_time.valid,
                         "pfq_debug_last_adapters: the last pfq_prep_reads with reads on this tree ran without adapters");
}

// ---- mate overlap ------------------------------------------------------------------------------------------------------------

int pfq_tree_set_mate_overlap(pfq_tree *tree, uint32_t min_overlap, uint32_t max_error_percent) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(insertion_error(*tree));
    pfq_tree &t = *tree;
    if (min_overlap == 0) {
        t.ov_on = false;
        t.ov_min_overlap = t.ov_max_error_percent = 0;
        return PFQ_OK;
    }
    if (min_overlap > PFQ_OVERLAP_LEN_MAX)
        return fail(PFQ_ERR_ARG, "pfq_tree_set_mate_overlap: min_overlap must be 0 (off) or 1 .. " + std::to_string(PFQ_OVERLAP_LEN_MAX) + ", not " + std::to_string(min_overlap));
    if (max_error_percent > 50) return fail(PFQ_ERR_ARG, "pfq_tree_set_mate_overlap: max_error_percent must be 0 .. 50, not " + std::to_string(max_error_percent));
    t.ov_min_overlap = min_overlap;
    t.ov_max_error_percent = max_error_percent;
    t.ov_on = true;
    return PFQ_OK;
}

int pfq_prep_last_overlap(pfq_tree *tree, pfq_prep_overlap *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    if (!tree->pp_have) return fail(PFQ_ERR_STATE, "pfq_prep_last_overlap before a pfq_prep_reads on this tree");
    if (!tree->ov_last)
        return fail(PFQ_ERR_STATE, "pfq_prep_last_overlap: the last pfq_prep_reads on this tree ran without the mate overlap (pfq_tree_set_mate_overlap and PFQ_PREP_PAIRED)");
    *out = tree->ov_out;
    out->hist = tree->out_ov_hist.data();
    if (tree->ov_last_reads) {
        out->insert = tree->out_ov_insert.data();
        out->mismatches = tree->out_ov_mm.data();
    }
    return PFQ_OK;
}

int pfq_debug_last_overlap(pfq_tree *tree, double *ms) {
    return last_stage_ms(tree, ms, &pfq_tree::ov_time, tree && tree->pp_time.valid,
                         "pfq_debug_last_overlap: the last pfq_prep_reads with reads on this tree ran without the mate overlap");
}

// ---- mate correction ---------------------------------------------------------------------------------------------------------

static_assert(sizeof(pfq_prep_patch) == sizeof(pfq::CorPatch) && sizeof(pfq_prep_patch) == 12, "the kernel writes pfq_prep_patch");

int pfq_tree_set_mate_correct(pfq_tree *tree, uint32_t high, uint32_t low) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(insertion_error(*tree));
    pfq_tree &t = *tree;
    if (high == 0) {
        t.mc_high = t.mc_low = 0;
        return PFQ_OK;
    }
    if (high > 93) return fail(PFQ_ERR_ARG, "pfq_tree_set_mate_correct: high must be 0 (off) or 1 .. 93, not " + std::to_string(high));
    if (low >= high) return fail(PFQ_ERR_ARG, "pfq_tree_set_mate_correct: low must be below high = " + std::to_string(high) + ", not " + std::to_string(low));
    t.mc_high = high;
    t.mc_low = low;
    return PFQ_OK;
}

int pfq_prep_last_corrections(pfq_tree *tree, pfq_prep_corrections *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    if (!tree->pp_have) return fail(PFQ_ERR_STATE, "pfq_prep_last_corrections before a pfq_prep_reads on this tree");
    if (!tree->mc_last)
        return fail(PFQ_ERR_STATE, "pfq_prep_last_corrections: the last pfq_prep_reads on this tree ran without the mate correction (pfq_tree_set_mate_correct, pfq_tree_set_mate_overlap and PFQ_PREP_PAIRED)");
    *out = tree->mc_out;
    if (tree->mc_last_reads) out->patches = tree->out_mc_patch.data();
    return PFQ_OK;
}

int pfq_debug_last_corrections(pfq_tree *tree, double *ms) {
    return last_stage_ms(tree, ms, &pfq_tree::mc_time, tree && tree->pp_time.valid,
                         "pfq_debug_last_corrections: the last pfq_prep_reads with reads on this tree wrote no patch list (the mate correction and PFQ_PREP_WANT_READS)");
}

int pfq_prep_query(pfq_tree *tree, float threshold, uint32_t flags, pfq_hits *hits) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(check_flags(*tree, flags, tree->pp_kept, threshold));
    if (!tree->pp_have) return fail(PFQ_ERR_STATE, "pfq_prep_query before a pfq_prep_reads on this tree");
    if ((flags & PFQ_PAIRED) && !tree->pp_paired)
        return fail(PFQ_ERR_ARG, "pfq_prep_query: PFQ_PAIRED on a block prepared without PFQ_PREP_PAIRED (its kept reads are not whole fragments)");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    const int slot = t.pp_sets.cur;
    HIP_TRY(hipStreamWaitEvent(nullptr, t.pp_ready, 0));  // (the classification is ordered behind the prep on the device)
    const int rc = query_device(t, t.d_pp_seq[slot].p, t.d_pp_off[slot].p, t.pp_kept, t.pp_bases, threshold, flags, nullptr, hits);
    HIP_TRY(t.pp_sets.read_by(slot, nullptr));  // (also behind a call that failed half-way: what it queued may read the set)
    PFQ_TRY(rc);
    if (flags & PFQ_WANT_HITS) HIP_TRY(hipStreamSynchronize(nullptr));
    return PFQ_OK;
}

int pfq_debug_prep_csr(pfq_tree *tree, uint8_t *seq_out, uint64_t *off_out) {
    if (!tree || !off_out || (tree->pp_bases && !seq_out)) return fail(PFQ_ERR_ARG, "null argument");
    if (!tree->pp_have) return fail(PFQ_ERR_STATE, "pfq_debug_prep_csr before a pfq_prep_reads on this tree");
    PFQ_TRY(use_device(tree->device));
    const pfq_tree &t = *tree;
    if (t.pp_bases) HIP_TRY(hipMemcpy(seq_out, t.d_pp_seq[t.pp_sets.cur].p, t.pp_bases, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(off_out, t.d_pp_off[t.pp_sets.cur].p, (t.pp_kept + 1) * 8, hipMemcpyDeviceToHost));
    return PFQ_OK;
}

int pfq_debug_last_prep(pfq_tree *tree, double *ms) {
    return last_stage_ms(tree, ms, &pfq_tree::pp_time, true,
                         "pfq_debug_last_prep before a pfq_prep_reads with reads on this tree");
}

// ---- depletion ---------------------------------------------------------------------------------------------------------------

// Everything runs on tree's copy stream, which the prep used: the screen's classification of the prepared slot, then the mark,
// the two scans, the offsets and the gather from the raw block into the same slot, so the stream orders the rewrite of the
// slot behind its last reader.  The null stream, where pfq_prep_query queued the previous block's classification (it reads the
// other slot), is neither waited for nor given work.
int pfq_prep_deplete(pfq_tree *tree, pfq_tree *screen, float threshold, uint32_t flags, pfq_prep_depleted *out) {
    if (!tree || !screen || !out) return fail(PFQ_ERR_ARG, "null argument");
    if (screen == tree) return fail(PFQ_ERR_ARG, "pfq_prep_deplete: the screen is the tree whose block it would deplete");
    if (flags != 0 && flags != PFQ_PAIRED && flags != (PFQ_PAIRED | PFQ_PAIR_BOTH))
        return fail(PFQ_ERR_ARG, "pfq_prep_deplete: flags must be 0, PFQ_PAIRED or PFQ_PAIRED | PFQ_PAIR_BOTH");
    if (screen->device != tree->device)
        return fail(PFQ_ERR_ARG, "pfq_prep_deplete: the screen is on device " + std::to_string(screen->device) + ", the prepared block on device " +
                                     std::to_string(tree->device));
    PFQ_TRY(insertion_error(*tree));
    PFQ_TRY(insertion_error(*screen));
    if (!tree->pp_have) return fail(PFQ_ERR_STATE, "pfq_prep_deplete before a pfq_prep_reads on this tree");
    if ((flags & PFQ_PAIRED) && !tree->pp_paired)
        return fail(PFQ_ERR_ARG, "pfq_prep_deplete: PFQ_PAIRED on a block prepared without PFQ_PREP_PAIRED (its kept reads are not whole fragments)");
    if (screen->root < 0) return fail(PFQ_ERR_STATE, "pfq_prep_deplete: the screen is an empty tree");
    if (screen->is_shard)
        return fail(PFQ_ERR_UNSUPPORTED, "pfq_prep_deplete: the screen is a subtree shard: it sees only its own leaves, so an empty row does not "
                                         "say that the unit misses the database");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree, &s = *screen;
    const bool paired = (flags & PFQ_PAIRED) != 0;
    const uint32_t per = paired ? 2u : 1u;
    const uint64_t n_reads = t.pp_reads, n_before = t.pp_kept, n_units = n_before / per;
    const int slot = t.pp_sets.cur;
    hipStream_t st = t.copy_stream;
    HIP_TRY(t.dp_time.ensure());
    HIP_TRY(t.h_dp_tot.ensure(pfq::DEPL_TOT_N + 2));
    HIP_TRY(t.d_dp_tot.ensure(pfq::DEPL_TOT_N));
    *out = pfq_prep_depleted{};
    out->n_units = n_units;
    uint64_t n_kept = n_before, bases_kept = t.pp_bases;
    if (n_units) {
        // (a classification of this block that pfq_prep_query has queued still reads the slot the gather below rewrites)
        HIP_TRY(t.pp_sets.wait(slot));
        if (!paired) {
            HIP_TRY(t.d_dp_hit.ensure(n_units));
            HIP_TRY(hipMemsetAsync(t.d_dp_hit.p, 0, n_units * 4, st));
        }
        HIP_TRY(hipMemsetAsync(t.d_dp_tot.p, 0, pfq::DEPL_TOT_N * 8, st));
        HIP_TRY(t.dp_time.mark(0, st));
        t.dp_time.valid = false;
        PFQ_TRY(query_device(s, t.d_pp_seq[slot].p, t.d_pp_off[slot].p, n_before, t.pp_bases, threshold, flags, st, nullptr, true, t.d_dp_hit.p));
        HIP_TRY(t.dp_time.mark(1, st));
        pfq::DepleteArgs d{};
        d.hit = t.d_dp_hit.p;
        d.allhit = s.d_allhit.p;
        d.frag_off = paired ? s.d_frag_off.p : nullptr;
        d.pair_mode = paired ? ((flags & PFQ_PAIR_BOTH) ? 2 : 1) : 0;
        d.n_units = n_units;
        d.n_reads = n_reads;
        d.kept = t.d_pp_kept.p;
        d.keep = t.d_pp_keep.p;
        d.klen = t.d_pp_klen.p;
        d.reason = t.d_pp_reason.p;
        d.totals = t.d_dp_tot.p;
        pfq::launch_deplete_mark(d, st);
        pfq::launch_scan_u32(t.d_pp_keep.p, n_reads, t.d_pp_sums.p, t.d_pp_kpos.p, st);
        pfq::launch_scan_u32(t.d_pp_klen.p, n_reads, t.d_pp_sums.p, t.d_pp_koff.p, st);
        pfq::PrepArgs a{};
        a.seq = t.d_pp_in.p;
        a.off = t.d_pp_inoff.p;
        a.n_reads = n_reads;
        a.paired = t.pp_paired ? 1u : 0u;
        a.begin = t.d_pp_begin.p;
        a.len = t.d_pp_len.p;
        a.reason = t.d_pp_reason.p;
        a.keep = t.d_pp_keep.p;
        a.klen = t.d_pp_klen.p;
        a.totals = t.d_pp_tot.p;
        a.kpos = t.d_pp_kpos.p;
        a.koff = t.d_pp_koff.p;
        a.kept = t.d_pp_kept.p;
        a.csr_off = t.d_pp_off[slot].p;
        a.out = t.d_pp_seq[slot].p;
        pfq::launch_prep_gather(a, st);
        HIP_TRY(t.dp_time.mark(2, st));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(t.h_dp_tot.p, t.d_dp_tot.p, pfq::DEPL_TOT_N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(t.h_dp_tot.p + pfq::DEPL_TOT_N, t.d_pp_kpos.p + n_reads, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(t.h_dp_tot.p + pfq::DEPL_TOT_N + 1, t.d_pp_koff.p + n_reads, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(t.pp_ready, st));
        HIP_TRY(hipStreamSynchronize(st));
        t.dp_time.valid = true;
        out->units_removed = t.h_dp_tot.p[pfq::DEPL_TOT_UNITS];
        out->reads_removed = t.h_dp_tot.p[pfq::DEPL_TOT_READS];
        out->bases_removed = t.h_dp_tot.p[pfq::DEPL_TOT_BASES];
        n_kept = t.h_dp_tot.p[pfq::DEPL_TOT_N];
        bases_kept = t.h_dp_tot.p[pfq::DEPL_TOT_N + 1];
        t.pp_kept = n_kept;
        t.pp_bases = bases_kept;
    }
    out->n_kept = n_kept;
    out->bases_kept = bases_kept;
    if (t.pp_want_reads) {
        if (!t.dp_have) {  // the first call since the prep starts from what the prep handed out
            t.out_dp_kept = t.out_pp_kept;
            t.out_dp_reason = t.out_pp_reason;
        }
        if (out->units_removed) {
            t.out_dp_kept.resize(std::max<uint64_t>(n_kept, 1));
            if (n_kept) HIP_TRY(hipMemcpyAsync(t.out_dp_kept.data(), t.d_pp_kept.p, n_kept * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(t.out_dp_reason.data(), t.d_pp_reason.p, n_reads * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        out->kept = t.out_dp_kept.data();
        out->reason = t.out_dp_reason.data();
    }
    t.dp_have = true;
    return PFQ_OK;
}

int pfq_debug_last_deplete(pfq_tree *tree, double *ms) {
    return last_stage_ms(tree, ms, &pfq_tree::dp_time, true,
                         "pfq_debug_last_deplete before a pfq_prep_deplete with units on this tree");
}

int pfq_last_hit_scores(pfq_tree *tree, const uint32_t **scores, uint64_t *n_hits) {
    if (!tree || !scores || !n_hits) return fail(PFQ_ERR_ARG, "null argument");
    if (!tree->scores_valid) return fail(PFQ_ERR_ARG, "the last query call on this tree did not ask for scores (PFQ_WANT_SCORES)");
    *scores = tree->h_hit_scores.p;
    *n_hits = tree->scores_n;
    return PFQ_OK;
}

int pfq_tree_clades(pfq_tree *tree, const pfq_clade **clades, uint64_t *n) {
    if (!tree || !clades || !n) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    PFQ_TRY(ensure_lca(*tree));
    *clades = tree->clades.data();
    *n = tree->clades.size();
    return PFQ_OK;
}

int pfq_clade_counts(pfq_tree *tree, const uint64_t **here, const uint64_t **below, uint64_t *n) {
    if (!tree || !n) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(ensure_lca(t));
    const size_t nc = t.clades.size();
    t.out_here.assign(nc, 0);
    if (nc && !t.leaves.empty()) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(t.out_here.data(), t.d_clade_here.p, nc * 8, hipMemcpyDeviceToHost));
    }
    t.out_below = t.out_here;
    for (size_t c = nc; c-- > 1;) t.out_below[t.clades[c].parent] += t.out_below[c];  // (pre-order: children after their parent)
    if (here) *here = t.out_here.data();
    if (below) *below = t.out_below.data();
    *n = nc;
    return PFQ_OK;
}

int pfq_last_lca(pfq_tree *tree, const uint32_t **lca, uint64_t *n_units) {
    if (!tree || !lca || !n_units) return fail(PFQ_ERR_ARG, "null argument");
    if (!tree->lca_last) return fail(PFQ_ERR_ARG, "the last query call on this tree did not ask for the LCAs (PFQ_WANT_LCA)");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(wait_last_call(t));
    t.out_lca.resize(t.lca_units + 1);
    if (t.lca_units) HIP_TRY(hipMemcpy(t.out_lca.data(), t.d_lca.p, t.lca_units * 4, hipMemcpyDeviceToHost));
    *lca = t.out_lca.data();
    *n_units = t.lca_units;
    return PFQ_OK;
}

int pfq_last_best_rows(pfq_tree *tree, pfq_hits *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    if (!tree->best_last) return fail(PFQ_ERR_ARG, "the last query call on this tree did not ask for the best rows (PFQ_ROWS_BEST)");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(wait_last_call(t));
    t.out_best_off.assign(t.best_units + 1, 0);
    uint64_t total = 0;
    if (t.best_built) {
        HIP_TRY(hipMemcpy(t.out_best_off.data(), t.d_best_off.p, (t.best_units + 1) * 8, hipMemcpyDeviceToHost));
        total = t.out_best_off[t.best_units];
    }
    t.out_best_leaves.resize(total + 1);
    if (total) HIP_TRY(hipMemcpy(t.out_best_leaves.data(), t.d_best_leaves.p, total * 4, hipMemcpyDeviceToHost));
    out->n_reads = t.best_units;
    out->offsets = t.out_best_off.data();
    out->leaves = t.out_best_leaves.data();
    return PFQ_OK;
}

// ---- taxonomy (pfq.h "taxonomy") ----
namespace {
thread_local pfq_taxonomy::File g_tax_file;
thread_local std::vector<const char *> g_tax_file_names;
thread_local pfq_taxonomy::NodeTable g_tax_nodes;
thread_local std::vector<std::string> g_db_leaf_ids;
thread_local std::vector<const char *> g_db_leaf_ptr;
}  // namespace

int pfq_db_leaf_ids(const char *db_dir, const char *const **tax_ids, uint64_t *n_leaves) {
    if (!db_dir || !tax_ids || !n_leaves) return fail(PFQ_ERR_ARG, "null argument");
    *n_leaves = 0;
    pfq_tree t;  // the model only: no filter is read, no device is touched
    PFQ_TRY(read_tree_bin(db_dir, t));
    g_db_leaf_ids.clear();
    for (int32_t v : leaves_dfs(t)) {
        if (!t.nodes[v].has_tax) return fail(PFQ_ERR_FORMAT, "leaf node without tax_id (reference: unwrap panic, query.rs:146)");
        g_db_leaf_ids.push_back(t.nodes[v].tax_id);
    }
    g_db_leaf_ptr.clear();
    for (const std::string &s : g_db_leaf_ids) g_db_leaf_ptr.push_back(s.c_str());
    g_db_leaf_ptr.push_back(nullptr);
    *tax_ids = g_db_leaf_ptr.data();
    *n_leaves = g_db_leaf_ids.size();
    return PFQ_OK;
}

int pfq_taxonomy_read(const char *path, const char *const *leaf_ids, uint64_t n_leaves, pfq_taxonomy_file *out) {
    if (!path || !out || (n_leaves && !leaf_ids)) return fail(PFQ_ERR_ARG, "null argument");
    memset(out, 0, sizeof *out);
    std::vector<std::string> ids;
    for (uint64_t l = 0; l < n_leaves; ++l) {
        if (!leaf_ids[l]) return fail(PFQ_ERR_ARG, "null leaf id");
        ids.push_back(leaf_ids[l]);
    }
    bool io = false;
    const std::string err = pfq_taxonomy::read_file(path, ids, g_tax_file, io);
    if (!err.empty()) return fail(io ? PFQ_ERR_IO : PFQ_ERR_FORMAT, err);
    g_tax_file_names.clear();
    for (const std::string &s : g_tax_file.names) g_tax_file_names.push_back(s.c_str());
    out->n_taxa = g_tax_file.parent.size();
    out->taxon_parent = g_tax_file.parent.data();
    out->taxon_names = g_tax_file_names.data();
    out->n_leaves = n_leaves;
    out->leaf_taxon = g_tax_file.leaf_taxon.data();
    out->lines_considered = g_tax_file.lines_considered;
    out->lines_other = g_tax_file.lines_other;
    out->leaves_without_line = g_tax_file.leaves_without_line;
    return PFQ_OK;
}

int pfq_taxonomy_nodes(uint64_t n_leaves, const char *const *leaf_ids, uint64_t n_taxa, const uint32_t *taxon_parent, const char *const *taxon_names,
                       const uint32_t *leaf_taxon, const pfq_taxon **nodes, uint64_t *n) {
    if (!nodes || !n) return fail(PFQ_ERR_ARG, "null argument");
    *n = 0;
    const std::string err = pfq_taxonomy::build_nodes(n_leaves, leaf_ids, n_taxa, taxon_parent, taxon_names, leaf_taxon, g_tax_nodes);
    if (!err.empty()) return fail(PFQ_ERR_ARG, err);
    *nodes = g_tax_nodes.nodes.data();
    *n = g_tax_nodes.nodes.size();
    return PFQ_OK;
}

int pfq_tree_set_taxonomy(pfq_tree *tree, uint64_t n_taxa, const uint32_t *taxon_parent, const char *const *taxon_names, const uint32_t *leaf_taxon) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(insertion_error(t));
    if (t.is_shard)
        return fail(PFQ_ERR_UNSUPPORTED, "a taxonomy on a subtree shard: a shard sees only its own leaves, so the rows it would count are partial");
    PFQ_TRY(finish_topology(t));
    if (t.root < 0) return fail(PFQ_ERR_STATE, "a taxonomy on an empty tree");
    PFQ_TRY(build_layout(t));
    const size_t nl = t.leaves.size();
    std::vector<const char *> ids;
    for (int32_t v : t.leaves) ids.push_back(t.nodes[v].tax_id.c_str());
    pfq_taxonomy::NodeTable nt;
    const std::string err = pfq_taxonomy::build_nodes(nl, ids.data(), n_taxa, taxon_parent, taxon_names, leaf_taxon, nt);
    if (!err.empty()) return fail(PFQ_ERR_ARG, err);
    HIP_TRY(hipDeviceSynchronize());  // (queued calls may still count on the tables about to go)
    tax_clear(t);
    t.tax = std::move(nt);
    for (size_t v = 0; v < t.tax.nodes.size(); ++v) t.tax.nodes[v].name = t.tax.names[v].c_str();  // (the strings may have moved)
    const size_t nn = t.tax.nodes.size();
    // the sparse table of range minima over the gaps' nodes, as ensure_lca builds the tree's own
    uint32_t levels = 1;
    while ((2ull << (levels - 1)) <= t.tax.gap.size()) ++levels;
    std::vector<uint32_t> tab((size_t)levels * nl, PFQ_NO_CLADE);
    std::copy(t.tax.gap.begin(), t.tax.gap.end(), tab.begin());
    for (uint32_t j = 1; j < levels; ++j) {
        const size_t half = (size_t)1 << (j - 1);
        const uint32_t *prev = tab.data() + (size_t)(j - 1) * nl;
        uint32_t *cur = tab.data() + (size_t)j * nl;
        for (size_t i = 0; i + 2 * half <= t.tax.gap.size(); ++i) cur[i] = std::min(prev[i], prev[i + half]);
    }
    std::vector<uint32_t> parent(nn), first(nn), heaviest(nn, PFQ_NO_CLADE);
    for (size_t v = 0; v < nn; ++v) {
        parent[v] = t.tax.nodes[v].parent;
        first[v] = t.tax.nodes[v].first_rank;
        if (v && (heaviest[parent[v]] == PFQ_NO_CLADE || t.tax.nodes[v].n_leaves > t.tax.nodes[heaviest[parent[v]]].n_leaves)) heaviest[parent[v]] = (uint32_t)v;
    }
    // the hot nodes: from top down the heaviest child while it holds at least half of all leaves (phage taxonomies are top-heavy)
    uint32_t cur = t.tax.top;
    for (uint32_t k = 0; k < pfq::TAX_HOT; ++k) {
        t.tax_hot[k] = PFQ_NO_CLADE;
        if (cur == PFQ_NO_CLADE) continue;
        const uint32_t h = heaviest[cur];
        cur = (h != PFQ_NO_CLADE && 2ull * t.tax.nodes[h].n_leaves >= nl) ? h : PFQ_NO_CLADE;
        t.tax_hot[k] = cur;
    }
    HIP_TRY(t.d_tax_rank.ensure(nl));
    HIP_TRY(t.d_tax_leaf_node.ensure(nl));
    HIP_TRY(t.d_tax_parent.ensure(nn));
    HIP_TRY(t.d_tax_first.ensure(nn));
    HIP_TRY(t.d_tax_gap_min.ensure(tab.size()));
    HIP_TRY(t.d_tax_here.ensure(nn));
    HIP_TRY(t.d_tax_any.ensure(nn));
    HIP_TRY(t.d_tax_misc.ensure(pfq::TAX_MISC_N));
    HIP_TRY(hipMemcpy(t.d_tax_rank.p, t.tax.rank.data(), nl * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.d_tax_leaf_node.p, t.tax.leaf_node.data(), nl * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.d_tax_parent.p, parent.data(), nn * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.d_tax_first.p, first.data(), nn * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.d_tax_gap_min.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    t.tax_set = true;
    return tax_zero(t);
}

int pfq_tree_taxa(pfq_tree *tree, const pfq_taxon **nodes, uint64_t *n) {
    if (!tree || !nodes || !n) return fail(PFQ_ERR_ARG, "null argument");
    *nodes = tree->tax_set ? tree->tax.nodes.data() : nullptr;
    *n = tree->tax_set ? tree->tax.nodes.size() : 0;
    return PFQ_OK;
}

int pfq_taxon_counts(pfq_tree *tree, const uint64_t **here, const uint64_t **below, const uint64_t **any, uint64_t *n) {
    if (!tree || !n) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    const size_t nn = t.tax_set ? t.tax.nodes.size() : 0;
    t.out_tax_here.assign(nn, 0);
    t.out_tax_any.assign(nn, 0);
    if (nn) {
        unsigned long long misc[pfq::TAX_MISC_N];
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(t.out_tax_here.data(), t.d_tax_here.p, nn * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(t.out_tax_any.data(), t.d_tax_any.p, nn * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(misc, t.d_tax_misc.p, sizeof misc, hipMemcpyDeviceToHost));
        // what the kernels count once instead of per node (pfq_kernels.h): the units with a hit touch every node down to top,
        // an all-leaf unit sits on top and touches every node below it
        t.out_tax_here[t.tax.top] += misc[pfq::TAX_MISC_ALL];
        for (size_t v = 0; v < nn; ++v) t.out_tax_any[v] = v <= t.tax.top ? misc[pfq::TAX_MISC_HIT] : t.out_tax_any[v] + misc[pfq::TAX_MISC_ALL];
    }
    t.out_tax_below = t.out_tax_here;
    for (size_t v = nn; v-- > 1;) t.out_tax_below[t.tax.nodes[v].parent] += t.out_tax_below[v];  // (pre-order: children after their parent)
    if (here) *here = t.out_tax_here.data();
    if (below) *below = t.out_tax_below.data();
    if (any) *any = t.out_tax_any.data();
    *n = nn;
    return PFQ_OK;
}

int pfq_last_taxa(pfq_tree *tree, const uint32_t **node, uint64_t *n_units) {
    if (!tree || !node || !n_units) return fail(PFQ_ERR_ARG, "null argument");
    if (!tree->taxa_last) return fail(PFQ_ERR_ARG, "the last query call on this tree did not ask for the taxa (PFQ_WANT_TAXA)");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(wait_last_call(t));
    t.out_tax_node.resize(t.taxa_units + 1);
    if (t.taxa_units) HIP_TRY(hipMemcpy(t.out_tax_node.data(), t.d_tax_node.p, t.taxa_units * 4, hipMemcpyDeviceToHost));
    *node = t.out_tax_node.data();
    *n_units = t.taxa_units;
    return PFQ_OK;
}

int pfq_abundance_reset(pfq_tree *tree) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    HIP_TRY(hipDeviceSynchronize());
    abund_clear(*tree);
    return PFQ_OK;
}

int pfq_coverage_reset(pfq_tree *tree) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    HIP_TRY(hipDeviceSynchronize());
    cover_clear(*tree);
    return PFQ_OK;
}

int pfq_coverage_get(pfq_tree *tree, pfq_coverage *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(build_layout(t));
    HIP_TRY(hipDeviceSynchronize());  // the queued sketches
    const size_t nl = t.leaves.size();
    const bool held = t.d_cov_regs.p != nullptr;
    const uint32_t p = held ? t.cov_p : cover_precision(t.knobs);
    PFQ_TRY(cover_filter_bits(t));
    t.out_cov_regs.assign((nl << p) + 1, 0);
    t.out_cov_units.assign(nl + 1, 0);
    t.out_cov_matched.assign(nl + 1, 0);
    t.out_cov_distinct.assign(nl + 1, 0.0);
    t.out_cov_genome.assign(nl + 1, 0.0);
    if (held && nl) {
        HIP_TRY(hipMemcpy(t.out_cov_regs.data(), t.d_cov_regs.p, nl << p, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(t.out_cov_units.data(), t.d_cov_cnt.p, nl * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(t.out_cov_matched.data(), t.d_cov_cnt.p + nl, nl * 8, hipMemcpyDeviceToHost));
    }
    const double d = (double)t.nbits;
    for (size_t l = 0; l < nl; ++l) {
        if (held) t.out_cov_distinct[l] = cover_estimate(t.out_cov_regs.data() + (l << p), p);
        const uint64_t b = t.cov_bits[l];
        t.out_cov_genome[l] = b >= t.nbits ? 0.0 : -(d / (double)t.hp.num_hashes) * std::log1p(-(double)b / d);
    }
    memset(out, 0, sizeof *out);
    out->n_leaves = nl;
    out->n_units = t.cov_units;
    out->precision = p;
    out->registers = t.out_cov_regs.data();
    out->units = t.out_cov_units.data();
    out->matched = t.out_cov_matched.data();
    out->filter_bits = t.cov_bits.data();
    out->distinct = t.out_cov_distinct.data();
    out->genome_kmers = t.out_cov_genome.data();
    return PFQ_OK;
}

int pfq_coverage_absorb(pfq_tree *dst, pfq_tree *src) {
    if (!dst || !src) return fail(PFQ_ERR_ARG, "null argument");
    if (dst == src) return fail(PFQ_ERR_ARG, "pfq_coverage_absorb: dst and src are one tree");
    pfq_tree &d = *dst, &s = *src;
    PFQ_TRY(use_device(s.device));
    PFQ_TRY(build_layout(s));
    HIP_TRY(hipDeviceSynchronize());
    PFQ_TRY(use_device(d.device));
    PFQ_TRY(build_layout(d));
    HIP_TRY(hipDeviceSynchronize());
    const size_t nl = d.leaves.size();
    if (s.leaves.size() != nl || d.is_shard != s.is_shard || d.shard_first_leaf != s.shard_first_leaf)
        return fail(PFQ_ERR_ARG, "pfq_coverage_absorb: the trees do not hold the same leaves (" + std::to_string(nl) + " and " +
                                 std::to_string(s.leaves.size()) + ")");
    if (d.hp.k != s.hp.k || d.hp.num_hashes != s.hp.num_hashes || d.hp.nbits != s.hp.nbits || d.hp.a1 != s.hp.a1 || d.hp.a2 != s.hp.a2)
        return fail(PFQ_ERR_ARG, "pfq_coverage_absorb: the trees differ in their hash parameters");
    const uint32_t pd = d.d_cov_regs.p ? d.cov_p : cover_precision(d.knobs), ps = s.d_cov_regs.p ? s.cov_p : cover_precision(s.knobs);
    if (pd != ps)
        return fail(PFQ_ERR_ARG, "pfq_coverage_absorb: the sketches differ in precision (" + std::to_string(pd) + " and " + std::to_string(ps) + ")");
    if (s.d_cov_regs.p && nl) {
        PFQ_TRY(cover_ensure(d, nl, nullptr));  // (nothing was absorbed if this fails)
        // staged through host memory: the replicas may sit on different devices, and this runs once per job
        const size_t nr = nl << pd;
        std::vector<uint8_t> rs(nr), rd(nr);
        std::vector<unsigned long long> cs(2 * nl), cd(2 * nl);
        PFQ_TRY(use_device(s.device));
        HIP_TRY(hipMemcpy(rs.data(), s.d_cov_regs.p, nr, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(cs.data(), s.d_cov_cnt.p, 2 * nl * 8, hipMemcpyDeviceToHost));
        PFQ_TRY(use_device(d.device));
        HIP_TRY(hipMemcpy(rd.data(), d.d_cov_regs.p, nr, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(cd.data(), d.d_cov_cnt.p, 2 * nl * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nr; ++i) rd[i] = std::max(rd[i], rs[i]);
        for (size_t i = 0; i < 2 * nl; ++i) cd[i] += cs[i];
        HIP_TRY(hipMemcpy(d.d_cov_regs.p, rd.data(), nr, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d.d_cov_cnt.p, cd.data(), 2 * nl * 8, hipMemcpyHostToDevice));
    }
    d.cov_units += s.cov_units;
    PFQ_TRY(use_device(s.device));
    cover_clear(s);
    PFQ_TRY(use_device(d.device));
    return PFQ_OK;
}

// ---- threshold sweep (pfq.h "threshold sweep") ----
int pfq_tree_set_sweep(pfq_tree *tree, const float *thresholds, uint32_t n) {
    if (!tree || (n && !thresholds)) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    if (n == 0) {
        PFQ_TRY(insertion_error(t));
        HIP_TRY(hipDeviceSynchronize());
        t.sw_thr.clear();
        sweep_drop(t);
        return PFQ_OK;
    }
    if (n > PFQ_SWEEP_MAX) return fail(PFQ_ERR_ARG, "pfq_tree_set_sweep: " + std::to_string(n) + " thresholds, at most " + std::to_string(PFQ_SWEEP_MAX));
    for (uint32_t i = 0; i < n; ++i) {
        if (thresholds[i] != thresholds[i]) return fail(PFQ_ERR_ARG, "pfq_tree_set_sweep: threshold " + std::to_string(i) + " is not a number");
        if (i && !(thresholds[i - 1] < thresholds[i]))
            return fail(PFQ_ERR_ARG, "pfq_tree_set_sweep: the thresholds must be strictly ascending (" + std::to_string(thresholds[i - 1]) + " before " +
                                     std::to_string(thresholds[i]) + ")");
    }
    PFQ_TRY(finish_topology(t));
    if (t.root < 0) return fail(PFQ_ERR_STATE, "pfq_tree_set_sweep on an empty tree");
    PFQ_TRY(sweep_refused(t, "pfq_tree_set_sweep"));
    PFQ_TRY(build_layout(t));
    HIP_TRY(hipDeviceSynchronize());
    sweep_drop(t);
    t.sw_thr.assign(thresholds, thresholds + n);
    const int rc = sweep_ensure(t, t.leaves.size(), nullptr);
    if (rc != PFQ_OK) t.sw_thr.clear();
    PFQ_TRY(rc);
    HIP_TRY(hipDeviceSynchronize());  // (the counters are zero before a call on any stream adds to them)
    return PFQ_OK;
}

int pfq_sweep_reset(pfq_tree *tree) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    HIP_TRY(hipDeviceSynchronize());
    return sweep_zero(*tree);
}

int pfq_sweep_get(pfq_tree *tree, pfq_sweep *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(build_layout(t));
    HIP_TRY(hipDeviceSynchronize());  // the queued counts
    const size_t nl = t.leaves.size(), n_thr = t.sw_thr.size();
    std::vector<uint64_t> st(sweep_words(n_thr, nl), 0);
    if (t.d_sw_state.p && t.sw_nl == nl) HIP_TRY(hipMemcpy(st.data(), t.d_sw_state.p, st.size() * 8, hipMemcpyDeviceToHost));
    const uint64_t *pass = st.data(), *uniq = pass + (n_thr + 1) * nl, *tops = uniq + n_thr * nl;
    t.out_sw_thr = t.sw_thr;
    t.out_sw_thr.push_back(0.0f);
    t.out_sw_leaf_units.assign(n_thr * nl + 1, 0);
    t.out_sw_leaf_unique.assign(n_thr * nl + 1, 0);
    t.out_sw_sums.assign(4 * n_thr + 1, 0);
    uint64_t *hit = t.out_sw_sums.data(), *unique = hit + n_thr, *entries = unique + n_thr, *genomes = entries + n_thr;
    for (size_t th = n_thr; th-- > 0;) {  // leaf_units[th] = leaf_units[th + 1] + pass[th + 1], from the top
        uint64_t *row = t.out_sw_leaf_units.data() + th * nl;
        for (size_t l = 0; l < nl; ++l) {
            row[l] = pass[(th + 1) * nl + l] + (th + 1 < n_thr ? row[nl + l] : 0);
            t.out_sw_leaf_unique[th * nl + l] = uniq[th * nl + l];
            entries[th] += row[l];
            genomes[th] += row[l] != 0;
            unique[th] += uniq[th * nl + l];
        }
        hit[th] = tops[th + 1] + (th + 1 < n_thr ? hit[th + 1] : 0);
    }
    memset(out, 0, sizeof *out);
    out->n_thresholds = (uint32_t)n_thr;
    out->thresholds = t.out_sw_thr.data();
    out->n_leaves = nl;
    out->n_units = n_thr ? t.sw_units : 0;
    out->leaf_units = t.out_sw_leaf_units.data();
    out->leaf_unique = t.out_sw_leaf_unique.data();
    out->units_hit = hit;
    out->units_unique = unique;
    out->entries = entries;
    out->genomes_hit = genomes;
    return PFQ_OK;
}

int pfq_sweep_absorb(pfq_tree *dst, pfq_tree *src) {
    if (!dst || !src) return fail(PFQ_ERR_ARG, "null argument");
    if (dst == src) return fail(PFQ_ERR_ARG, "pfq_sweep_absorb: dst and src are one tree");
    pfq_tree &d = *dst, &s = *src;
    PFQ_TRY(use_device(s.device));
    PFQ_TRY(build_layout(s));
    HIP_TRY(hipDeviceSynchronize());
    PFQ_TRY(use_device(d.device));
    PFQ_TRY(build_layout(d));
    HIP_TRY(hipDeviceSynchronize());
    const size_t nl = d.leaves.size(), n_thr = d.sw_thr.size();
    if (s.leaves.size() != nl || d.is_shard != s.is_shard || d.shard_first_leaf != s.shard_first_leaf)
        return fail(PFQ_ERR_ARG, "pfq_sweep_absorb: the trees do not hold the same leaves (" + std::to_string(nl) + " and " +
                                 std::to_string(s.leaves.size()) + ")");
    if (d.hp.k != s.hp.k || d.hp.num_hashes != s.hp.num_hashes || d.hp.nbits != s.hp.nbits || d.hp.a1 != s.hp.a1 || d.hp.a2 != s.hp.a2)
        return fail(PFQ_ERR_ARG, "pfq_sweep_absorb: the trees differ in their hash parameters");
    if (s.sw_thr.size() != n_thr || (n_thr && memcmp(s.sw_thr.data(), d.sw_thr.data(), n_thr * sizeof(float))))
        return fail(PFQ_ERR_ARG, "pfq_sweep_absorb: the trees' threshold lists differ");
    if (!n_thr) return PFQ_OK;
    if (s.d_sw_state.p && s.sw_nl == nl) {
        PFQ_TRY(sweep_ensure(d, nl, nullptr));  // (nothing was absorbed if this fails)
        // staged through host memory: the replicas may sit on different devices, and this runs once per job
        const size_t words = sweep_words(n_thr, nl);
        std::vector<unsigned long long> hs(words), hd(words);
        PFQ_TRY(use_device(s.device));
        HIP_TRY(hipMemcpy(hs.data(), s.d_sw_state.p, words * 8, hipMemcpyDeviceToHost));
        PFQ_TRY(use_device(d.device));
        HIP_TRY(hipDeviceSynchronize());  // (the zeroing of counters made just now)
        HIP_TRY(hipMemcpy(hd.data(), d.d_sw_state.p, words * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < words; ++i) hd[i] += hs[i];
        HIP_TRY(hipMemcpy(d.d_sw_state.p, hd.data(), words * 8, hipMemcpyHostToDevice));
    }
    d.sw_units += s.sw_units;
    PFQ_TRY(use_device(s.device));
    const int rc = sweep_zero(s);
    PFQ_TRY(use_device(d.device));
    return rc;
}

// ---- pfq_tree_similarity ----
namespace {
// Distinct k-mers behind x set bits of a filter of m bits and h hashes (Swamidass-Baldi, as pfq_coverage.genome_kmers); a full
// filter is not estimable: 0.0.
double sim_kmers(uint64_t x, uint64_t m, uint32_t h) {
    return x >= m ? 0.0 : -((double)m / (double)h) * std::log1p(-(double)x / (double)m);
}
// The leaves a list names, as filter rows of the tree (NULL: every leaf, in order).
int sim_rows(const pfq_tree &t, const char *which, const uint32_t *leaves, uint64_t n, std::vector<uint32_t> &rows) {
    const size_t nl = t.leaves.size();
    rows.clear();
    if (!leaves) {
        rows.assign(t.col_row.begin(), t.col_row.begin() + nl);  // (the first nl columns are the leaves)
        return PFQ_OK;
    }
    rows.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (leaves[i] >= nl)
            return fail(PFQ_ERR_ARG, std::string("pfq_tree_similarity: ") + which + "[" + std::to_string(i) + "] = " + std::to_string(leaves[i]) +
                                         " is not a leaf index (the tree has " + std::to_string(nl) + " leaves)");
        rows.push_back(t.col_row[leaves[i]]);
    }
    return PFQ_OK;
}
}  // namespace

int pfq_tree_similarity(pfq_tree *a, const uint32_t *leaves_a, uint64_t n_a, pfq_tree *b, const uint32_t *leaves_b, uint64_t n_b, pfq_similarity *out) {
    if (!a) return fail(PFQ_ERR_ARG, "pfq_tree_similarity: tree a is NULL");
    if (!out) return fail(PFQ_ERR_ARG, "pfq_tree_similarity: out is NULL");
    if (!b) b = a;
    pfq_tree &ta = *a, &tb = *b;
    // the queued work of both trees, pending insertions included (a sticky insertion error is returned here)
    PFQ_TRY(use_device(tb.device));
    PFQ_TRY(build_layout(tb));
    HIP_TRY(hipDeviceSynchronize());
    if (b != a) {
        PFQ_TRY(use_device(ta.device));
        PFQ_TRY(build_layout(ta));
        HIP_TRY(hipDeviceSynchronize());
    }
    if (ta.leaves.empty() || tb.leaves.empty()) return fail(PFQ_ERR_STATE, "pfq_tree_similarity on an empty tree");
    auto differ = [&](const char *field, uint64_t va, uint64_t vb) {
        return fail(PFQ_ERR_ARG, std::string("pfq_tree_similarity: the trees differ in ") + field + " (" + std::to_string(va) + " and " + std::to_string(vb) +
                                     "): their filters cannot be compared bit by bit");
    };
    if (ta.kmer_size != tb.kmer_size) return differ("kmer_size", ta.kmer_size, tb.kmer_size);
    if (ta.nbits != tb.nbits) return differ("nbits", ta.nbits, tb.nbits);
    if (ta.num_hashes != tb.num_hashes) return differ("num_hashes", ta.num_hashes, tb.num_hashes);
    if (ta.seed1 != tb.seed1) return differ("seed1", ta.seed1, tb.seed1);
    if (ta.seed2 != tb.seed2) return differ("seed2", ta.seed2, tb.seed2);
    if (ta.device != tb.device)
        return fail(PFQ_ERR_ARG, "pfq_tree_similarity: the trees sit on different devices (" + std::to_string(ta.device) + " and " + std::to_string(tb.device) + ")");
    if (!leaves_a) n_a = ta.leaves.size();
    if (!leaves_b) n_b = tb.leaves.size();
    constexpr uint64_t MAX_PAIRS = 1ull << 26;
    if (n_a && n_b > MAX_PAIRS / n_a)
        return fail(PFQ_ERR_UNSUPPORTED, "pfq_tree_similarity: " + std::to_string(n_a) + " x " + std::to_string(n_b) +
                                             " pairs are more than 2^26 in one call: ask in panels (sublists of the leaves)");
    std::vector<uint32_t> rows_a, rows_b;
    PFQ_TRY(sim_rows(ta, "leaves_a", leaves_a, n_a, rows_a));
    PFQ_TRY(sim_rows(tb, "leaves_b", leaves_b, n_b, rows_b));
    const size_t np = (size_t)(n_a * n_b);
    ta.out_sim_shared.assign(np + 1, 0);
    ta.out_sim_bits_a.assign(n_a + 1, 0);
    ta.out_sim_bits_b.assign(n_b + 1, 0);
    if (np) {
        // scratch of this call only (freed on return: it never shows in pfq_info.device_bytes)
        DevBuf<uint32_t> d_rows, d_out;
        DevBuf<unsigned long long> d_pop;
        if (d_rows.ensure(n_a + n_b) != hipSuccess || d_out.ensure(np) != hipSuccess || d_pop.ensure(n_a + n_b) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PFQ_ERR_DEVICE, "pfq_tree_similarity: no device memory for " + std::to_string(np) + " pairs");
        }
        HIP_TRY(hipMemcpy(d_rows.p, rows_a.data(), n_a * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_rows.p + n_a, rows_b.data(), n_b * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(d_out.p, 0, np * 4, nullptr));  // (the slices of the tiled kernel add into it)
        const uint32_t slices = ta.knobs.sim_slices > 0 ? (uint32_t)std::min<long long>(ta.knobs.sim_slices, 65535) : 0;
        // PFQ_SIM_TIME=1 (tools/sim_bench.py): two HIP events round the intersection kernel alone; otherwise no call pays for them
        const bool timed = ta.knobs.sim_time == 1;
        Event ev[2];
        if (timed) {
            HIP_TRY(ev[0].ensure());
            if (ev[1].ensure() != hipSuccess) {
                (void)hipGetLastError();
                return fail(PFQ_ERR_DEVICE, "pfq_tree_similarity: hipEventCreate failed");
            }
            (void)hipEventRecord(ev[0], nullptr);
        }
        ta.sim_slices = pfq::launch_filter_intersections(ta.d_bits.p, d_rows.p, (uint32_t)n_a, tb.d_bits.p, d_rows.p + n_a, (uint32_t)n_b, ta.n_words,
                                                         ta.nbits, slices, ta.knobs.sim_naive == 1, d_out.p, nullptr);
        ta.sim_kernel_ms = 0.0f;
        if (timed) {
            (void)hipEventRecord(ev[1], nullptr);
            if (hipEventSynchronize(ev[1]) == hipSuccess) (void)hipEventElapsedTime(&ta.sim_kernel_ms, ev[0], ev[1]);
        }
        pfq::launch_filter_row_bits(ta.d_bits.p, d_rows.p, (uint32_t)n_a, ta.n_words, ta.nbits, d_pop.p, nullptr);
        pfq::launch_filter_row_bits(tb.d_bits.p, d_rows.p + n_a, (uint32_t)n_b, tb.n_words, tb.nbits, d_pop.p + n_a, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(ta.out_sim_shared.data(), d_out.p, np * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ta.out_sim_bits_a.data(), d_pop.p, n_a * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ta.out_sim_bits_b.data(), d_pop.p + n_a, n_b * 8, hipMemcpyDeviceToHost));
    }
    // the derived values (pfq.h "genome similarity"): this is the one place that computes them
    const uint64_t m = ta.nbits;
    const uint32_t h = ta.num_hashes;
    ta.out_sim_kmers_a.assign(n_a + 1, 0.0);
    ta.out_sim_kmers_b.assign(n_b + 1, 0.0);
    ta.out_sim_shared_kmers.assign(np + 1, 0.0);
    ta.out_sim_jaccard.assign(np + 1, 0.0);
    if (np) {
        for (uint64_t i = 0; i < n_a; ++i) ta.out_sim_kmers_a[i] = sim_kmers(ta.out_sim_bits_a[i], m, h);
        for (uint64_t j = 0; j < n_b; ++j) ta.out_sim_kmers_b[j] = sim_kmers(ta.out_sim_bits_b[j], m, h);
        for (uint64_t i = 0; i < n_a; ++i)
            for (uint64_t j = 0; j < n_b; ++j) {
                const uint64_t A = ta.out_sim_bits_a[i], B = ta.out_sim_bits_b[j], U = A + B - ta.out_sim_shared[i * n_b + j];
                if (A >= m || B >= m || U >= m) continue;  // not estimable: 0
                const double nu = sim_kmers(U, m, h), sh = std::max(0.0, ta.out_sim_kmers_a[i] + ta.out_sim_kmers_b[j] - nu);
                ta.out_sim_shared_kmers[i * n_b + j] = sh;
                ta.out_sim_jaccard[i * n_b + j] = nu > 0.0 ? sh / nu : 0.0;
            }
    }
    memset(out, 0, sizeof *out);
    out->n_a = n_a;
    out->n_b = n_b;
    out->shared_bits = ta.out_sim_shared.data();
    out->bits_a = ta.out_sim_bits_a.data();
    out->bits_b = ta.out_sim_bits_b.data();
    out->kmers_a = ta.out_sim_kmers_a.data();
    out->kmers_b = ta.out_sim_kmers_b.data();
    out->shared_kmers = ta.out_sim_shared_kmers.data();
    out->jaccard = ta.out_sim_jaccard.data();
    return PFQ_OK;
}

int pfq_debug_last_similarity(pfq_tree *a, double *kernel_ms, uint32_t *slices) {
    if (!a) return fail(PFQ_ERR_ARG, "null argument");
    if (kernel_ms) *kernel_ms = (double)a->sim_kernel_ms;
    if (slices) *slices = a->sim_slices;
    return PFQ_OK;
}

// ---- pfq_tree_recluster ----
namespace {
// HIP events of a PFQ_CLUSTER_TIME=1 call: pairs (begin, end) per measured stretch, destroyed with the call
struct ClusterTimer {
    bool on = false;
    std::vector<Event> ev;
    size_t mark() {  // records an event on the null stream; its index
        if (!on) return 0;
        Event e;
        if (e.ensure() != hipSuccess) {
            (void)hipGetLastError();
            on = false;
            return 0;
        }
        (void)hipEventRecord(e, nullptr);
        ev.push_back(std::move(e));
        return ev.size() - 1;
    }
    float between(size_t a, size_t b) const {
        float ms = 0.0f;
        if (on && a < ev.size() && b < ev.size() && hipEventSynchronize(ev[b]) == hipSuccess) (void)hipEventElapsedTime(&ms, ev[a], ev[b]);
        return ms;
    }
};
}  // namespace

int pfq_tree_recluster(pfq_tree *src, pfq_tree **out) {
    if (!src) return fail(PFQ_ERR_ARG, "pfq_tree_recluster: src is NULL");
    if (!out) return fail(PFQ_ERR_ARG, "pfq_tree_recluster: out is NULL");
    *out = nullptr;
    pfq_tree &s = *src;
    // src's queued work, pending insertions included (a sticky insertion error is returned here)
    PFQ_TRY(use_device(s.device));
    PFQ_TRY(build_layout(s));
    HIP_TRY(hipDeviceSynchronize());
    if (s.leaves.empty()) return fail(PFQ_ERR_STATE, "pfq_tree_recluster on an empty tree");
    if (s.is_shard) return fail(PFQ_ERR_UNSUPPORTED, "pfq_tree_recluster: a subtree shard holds only part of the database's leaves");
    const size_t L = s.leaves.size(), nw = (size_t)s.n_words;
    if (L > pfq::CLUSTER_MAX_LEAVES)
        return fail(PFQ_ERR_UNSUPPORTED, "pfq_tree_recluster: " + std::to_string(L) + " leaves are more than the " + std::to_string(pfq::CLUSTER_MAX_LEAVES) +
                                             " whose score matrix is kept in device memory");
    {
        std::unordered_set<std::string> seen;
        for (int32_t v : s.leaves)
            if (!seen.insert(s.nodes[v].bf_path).second)
                return fail(PFQ_ERR_UNSUPPORTED, "pfq_tree_recluster: two leaves share " + s.nodes[v].bf_path + ": the new tree would save two filters under one name");
    }
    std::unique_ptr<pfq_tree> t(new pfq_tree());
    t->device = s.device;
    t->kmer_size = s.kmer_size;
    t->nbits = s.nbits;
    t->num_hashes = s.num_hashes;
    t->seed1 = s.seed1;
    t->seed2 = s.seed2;
    t->false_pos_rate = s.false_pos_rate;
    t->largest_expected_genome = s.largest_expected_genome;
    PFQ_TRY(setup_hash_params(*t));
    const size_t n_nodes = 2 * L - 1;
    if (t->d_bits.ensure(n_nodes * nw) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PFQ_ERR_DEVICE, "not enough device memory for " + std::to_string(n_nodes) + " filters of " + std::to_string(nw * 8) + " bytes");
    }
    t->n_rows = t->row_capacity = n_nodes;
    // nodes in the numbering of the rule (pfq.h "re-clustering"), node n's filter in row n; finish_topology puts them in pre-order
    t->nodes.resize(n_nodes);
    t->filter_paths.resize(n_nodes);
    std::unordered_set<std::string> names;
    for (size_t i = 0; i < L; ++i) {
        const Node &from = s.nodes[s.leaves[i]];
        Node &nd = t->nodes[i];
        nd.bf_path = from.bf_path;
        nd.has_tax = from.has_tax;
        nd.tax_id = from.tax_id;
        nd.filter = (uint32_t)i;
        t->filter_paths[i] = nd.bf_path;
        names.insert(nd.bf_path);
        HIP_TRY(hipMemcpyAsync(t->d_bits.p + i * nw, s.d_bits.p + (size_t)s.col_row[i] * nw, nw * 8, hipMemcpyDeviceToDevice, nullptr));
    }
    ClusterTimer timer;
    timer.on = s.knobs.cluster_time == 1;
    s.cluster_ms[0] = s.cluster_ms[1] = s.cluster_ms[2] = 0.0f;
    s.cluster_nn_bytes = 0;
    s.cluster_rounds = 0;
    uint32_t round = 0;
    if (L > 1) {
        // scratch of this call only (freed on return: it never shows in pfq_info.device_bytes)
        const size_t pitch = (L + 15) & ~(size_t)15;
        constexpr uint64_t MAX_PANEL = 1ull << 26;  // pairs per launch of the intersection kernel
        DevBuf<unsigned long long> d_S, d_pop, d_pos, d_sums;
        DevBuf<uint32_t> d_rows, d_I, d_slot_of, d_best, d_flag, d_triples;
        DevBuf<uint2> d_meta;
        DevBuf<pfq::ClusterMerge> d_list;
        if (d_S.ensure(L * pitch) != hipSuccess || d_I.ensure((size_t)std::min<uint64_t>((uint64_t)L * L, MAX_PANEL)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PFQ_ERR_UNSUPPORTED, "pfq_tree_recluster: the score matrix of " + std::to_string(L) + " leaves (" + std::to_string((L * pitch * 8) >> 20) +
                                                 " MiB) and a panel of shared bits do not fit in device memory beside the two trees");
        }
        HIP_TRY(d_pop.ensure(L));
        HIP_TRY(d_rows.ensure(L));
        HIP_TRY(d_meta.ensure(pitch));
        HIP_TRY(d_slot_of.ensure(n_nodes));
        HIP_TRY(d_best.ensure(L));
        HIP_TRY(d_flag.ensure(n_nodes));
        HIP_TRY(d_pos.ensure(n_nodes + 1));
        HIP_TRY(d_sums.ensure(n_nodes / 4096 + 2));
        HIP_TRY(d_list.ensure(L / 2 + 1));
        HIP_TRY(d_triples.ensure(3 * (L / 2 + 1)));
        std::vector<uint2> meta(pitch, make_uint2(pfq::CLUSTER_NONE, 0u));
        std::vector<uint32_t> slot_of(n_nodes, pfq::CLUSTER_NONE), size_of(n_nodes, 1);
        for (size_t i = 0; i < L; ++i) {
            meta[i] = make_uint2((uint32_t)i, 1u);
            slot_of[i] = (uint32_t)i;
        }
        HIP_TRY(hipMemcpy(d_meta.p, meta.data(), pitch * sizeof(uint2), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_slot_of.p, slot_of.data(), n_nodes * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_rows.p, s.col_row.data(), L * 4, hipMemcpyHostToDevice));  // (the first L columns are the leaves)
        HIP_TRY(hipMemsetAsync(d_S.p, 0, L * pitch * 8, nullptr));
        // stage A: the shared bits of all leaf pairs on or above the diagonal, in panels of rows, and their scores
        const size_t ev_a = timer.mark();
        pfq::launch_filter_row_bits(s.d_bits.p, d_rows.p, (uint32_t)L, nw, s.nbits, d_pop.p, nullptr);
        const uint32_t slices = s.knobs.sim_slices > 0 ? (uint32_t)std::min<long long>(s.knobs.sim_slices, 65535) : 0;
        for (size_t r0 = 0; r0 < L;) {
            const size_t nc = L - r0, nr = std::min<size_t>(nc, std::max<size_t>(1, (size_t)(MAX_PANEL / nc)));
            HIP_TRY(hipMemsetAsync(d_I.p, 0, nr * nc * 4, nullptr));  // (the slices of the tiled kernel add into it)
            pfq::launch_filter_intersections(s.d_bits.p, d_rows.p + r0, (uint32_t)nr, s.d_bits.p, d_rows.p + r0, (uint32_t)nc, nw, s.nbits, slices,
                                             s.knobs.sim_naive == 1, d_I.p, nullptr);
            pfq::launch_cluster_scores(d_I.p, d_pop.p, (uint32_t)r0, (uint32_t)nr, (uint32_t)nc, s.nbits, d_S.p, pitch, nullptr);
            HIP_TRY(hipGetLastError());
            r0 += nr;
        }
        const size_t ev_b = timer.mark();
        // stage B: the rounds.  The host reads back a round's merges only: the topology lives here.
        std::vector<pfq::ClusterMerge> list(L / 2 + 1);
        std::vector<uint32_t> triples;
        std::vector<std::pair<size_t, size_t>> nn_ev;
        size_t made = L, live = L;
        uint64_t counter = 0;
        while (live > 1) {
            const size_t e0 = timer.mark();
            pfq::launch_cluster_nearest(d_S.p, pitch, d_meta.p, (uint32_t)L, d_best.p, nullptr);
            nn_ev.emplace_back(e0, timer.mark());
            s.cluster_nn_bytes += (uint64_t)live * pitch * 8;
            pfq::launch_cluster_mutual(d_slot_of.p, (uint32_t)made, d_best.p, d_meta.p, d_flag.p, nullptr);
            pfq::launch_scan_u32(d_flag.p, made, d_sums.p, d_pos.p, nullptr);
            pfq::launch_cluster_list(d_slot_of.p, (uint32_t)made, d_best.p, d_meta.p, d_flag.p, d_pos.p, d_S.p, pitch, d_list.p, (uint32_t)(L / 2 + 1), nullptr);
            HIP_TRY(hipGetLastError());
            unsigned long long n_merges = 0;
            HIP_TRY(hipMemcpy(&n_merges, d_pos.p + made, 8, hipMemcpyDeviceToHost));
            if (n_merges == 0 || n_merges > live / 2)
                return fail(PFQ_ERR_DEVICE, "pfq_tree_recluster: round " + std::to_string(round) + " found " + std::to_string(n_merges) + " mutual pairs among " +
                                                std::to_string(live) + " clusters");
            HIP_TRY(hipMemcpy(list.data(), d_list.p, (size_t)n_merges * sizeof(pfq::ClusterMerge), hipMemcpyDeviceToHost));
            triples.clear();
            for (size_t p = 0; p < n_merges; ++p) {
                const pfq::ClusterMerge &mg = list[p];
                const uint32_t node = (uint32_t)(made + p);
                if (mg.node_a >= made || mg.node_b >= made || mg.node_a >= mg.node_b)
                    return fail(PFQ_ERR_DEVICE, "pfq_tree_recluster: round " + std::to_string(round) + " lists a pair that is none");
                size_of[node] = size_of[mg.node_a] + size_of[mg.node_b];
                t->merges.push_back(pfq_merge{node, mg.node_a, mg.node_b, round, size_of[node], 0u, mg.score, (uint64_t)size_of[mg.node_a] * size_of[mg.node_b]});
                std::string name;
                do name = "Internal_Node_" + std::to_string(counter++);
                while (names.count(name + ".bf"));
                Node &nd = t->nodes[node];
                nd.has_tax = true;
                nd.tax_id = name;
                nd.bf_path = name + ".bf";
                nd.filter = node;
                nd.left = (int32_t)mg.node_a;
                nd.right = (int32_t)mg.node_b;
                t->filter_paths[node] = nd.bf_path;
                names.insert(nd.bf_path);
                triples.insert(triples.end(), {node, mg.node_a, mg.node_b});
            }
            pfq::launch_cluster_merge(d_S.p, pitch, d_meta.p, d_slot_of.p, (uint32_t)L, d_list.p, (uint32_t)n_merges, (uint32_t)made, nullptr);
            // the new nodes' filters: one launch per round, earlier rounds first (a later round reads their rows)
            HIP_TRY(hipMemcpy(d_triples.p, triples.data(), triples.size() * 4, hipMemcpyHostToDevice));
            pfq::launch_union(t->d_bits.p, nw, d_triples.p, (uint32_t)n_merges, nullptr);
            HIP_TRY(hipGetLastError());
            made += (size_t)n_merges;
            live -= (size_t)n_merges;
            ++round;
        }
        const size_t ev_c = timer.mark();
        HIP_TRY(hipDeviceSynchronize());
        s.cluster_ms[0] = timer.between(ev_a, ev_b);
        s.cluster_ms[1] = timer.between(ev_b, ev_c);
        for (const auto &e : nn_ev) s.cluster_ms[2] += timer.between(e.first, e.second);
    }
    HIP_TRY(hipDeviceSynchronize());
    s.cluster_rounds = round;
    t->internal_counter = t->merges.size();
    t->merge_rounds = round;
    t->root = (int32_t)(n_nodes - 1);
    t->tree_leaves = L;
    t->topology_dirty = true;  // renumbered into pre-order, parent ⊇ child verified on the device
    PFQ_TRY(finish_topology(*t));
    *out = t.release();
    return PFQ_OK;
}

int pfq_tree_merges(pfq_tree *tree, const pfq_merge **merges, uint64_t *n, uint32_t *rounds) {
    if (!tree || !merges || !n) return fail(PFQ_ERR_ARG, "null argument");
    *merges = tree->merges.data();
    *n = tree->merges.size();
    if (rounds) *rounds = tree->merge_rounds;
    return PFQ_OK;
}

int pfq_debug_last_recluster(pfq_tree *src, double *ms, uint64_t *nn_bytes, uint32_t *rounds) {
    if (!src) return fail(PFQ_ERR_ARG, "null argument");
    if (ms)
        for (int i = 0; i < 3; ++i) ms[i] = (double)src->cluster_ms[i];
    if (nn_bytes) *nn_bytes = src->cluster_nn_bytes;
    if (rounds) *rounds = src->cluster_rounds;
    return PFQ_OK;
}

int pfq_abundance_estimate(pfq_tree *tree, uint32_t max_iters, uint64_t tol, pfq_abundance *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    if (!max_iters) return fail(PFQ_ERR_ARG, "pfq_abundance_estimate: max_iters must be at least 1");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(build_layout(t));
    HIP_TRY(hipDeviceSynchronize());  // the queued appends
    if (t.ab_incomplete)
        return fail(PFQ_ERR_STATE, "the abundance log is incomplete: a query call's rows did not fit (it returned PFQ_ERR_UNSUPPORTED); "
                                   "pfq_abundance_reset starts a new log");
    const size_t nl = t.leaves.size();
    memset(out, 0, sizeof *out);
    t.out_mass.assign(nl + 1, 0);
    t.out_unique.assign(nl + 1, 0);
    out->n_leaves = nl;
    out->mass = t.out_mass.data();
    out->unique = t.out_unique.data();
    out->n_units = t.ab_units;
    out->n_unhit = t.ab_unhit;
    out->n_unique = t.ab_unique;
    out->n_ambiguous = t.ab_rows;
    out->n_all_leaves = t.ab_all;
    out->n_entries = t.ab_entries;
    out->iterations = 1;
    out->converged = 1;
    if (!t.ab_units || !nl) return PFQ_OK;  // nothing logged: nothing to iterate
    bool ok = true;
    PFQ_TRY(abund_room(t, 0, 0, ok));  // (the unique counters, should no call have made them)
    HIP_TRY(t.d_ab_a.ensure(nl));
    HIP_TRY(t.d_ab_b.ensure(nl));
    HIP_TRY(t.d_ab_delta.ensure(1));
    unsigned long long *a = t.d_ab_a.p, *nxt = t.d_ab_b.p;
    const uint32_t blocks = t.knobs.abund_blocks > 0 ? (uint32_t)std::min<long long>(t.knobs.abund_blocks, 65535) : 0;
    const bool lds = t.knobs.abund_lds != 0;
    pfq::launch_abund_start(a, nxt, t.d_ab_unique.p, (uint32_t)nl, nullptr);
    unsigned long long delta = 0;
    uint32_t it = 0;
    bool converged = false;
    while (it < max_iters && !converged) {
        HIP_TRY(hipMemsetAsync(t.d_ab_delta.p, 0, 8, nullptr));
        pfq::AbundStep s{t.d_ab_start.p, t.d_ab_len.p, t.d_ab_entries.p, t.ab_rows, (uint32_t)nl, a, nxt};
        pfq::launch_abund_step(s, blocks, lds, nullptr);
        pfq::launch_abund_delta(a, nxt, t.d_ab_unique.p, (uint32_t)nl, t.d_ab_delta.p, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&delta, t.d_ab_delta.p, 8, hipMemcpyDeviceToHost));  // (the one wait per iteration)
        std::swap(a, nxt);  // a: this iteration's result; nxt: unique << 16, the next one's start
        ++it;
        converged = delta <= tol;
    }
    HIP_TRY(hipMemcpy(t.out_mass.data(), a, nl * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t.out_unique.data(), t.d_ab_unique.p, nl * 8, hipMemcpyDeviceToHost));
    out->last_delta = delta;
    out->iterations = it;
    out->converged = converged ? 1 : 0;
    return PFQ_OK;
}

int pfq_abundance_absorb(pfq_tree *dst, pfq_tree *src) {
    if (!dst || !src) return fail(PFQ_ERR_ARG, "null argument");
    if (dst == src) return fail(PFQ_ERR_ARG, "pfq_abundance_absorb: dst and src are one tree");
    pfq_tree &d = *dst, &s = *src;
    if (d.is_shard || s.is_shard) return fail(PFQ_ERR_ARG, "pfq_abundance_absorb: a subtree shard has no abundance log");
    PFQ_TRY(use_device(s.device));
    PFQ_TRY(build_layout(s));
    HIP_TRY(hipDeviceSynchronize());
    PFQ_TRY(use_device(d.device));
    PFQ_TRY(build_layout(d));
    HIP_TRY(hipDeviceSynchronize());
    const size_t nl = d.leaves.size();
    if (s.leaves.size() != nl)
        return fail(PFQ_ERR_ARG, "pfq_abundance_absorb: the trees are not replicas (" + std::to_string(nl) + " and " + std::to_string(s.leaves.size()) +
                                 " leaves)");
    if (d.ab_incomplete || s.ab_incomplete) return fail(PFQ_ERR_STATE, "pfq_abundance_absorb: an abundance log is incomplete; pfq_abundance_reset starts a new one");
    if (!s.ab_units) return PFQ_OK;
    std::string why = abund_refusal(d, s.ab_units, s.ab_entries);
    bool ok = true;
    if (why.empty()) {
        PFQ_TRY(abund_room(d, s.ab_rows, s.ab_entries, ok));
        if (!ok) why = "no device memory for " + std::to_string(s.ab_rows) + " more rows with " + std::to_string(s.ab_entries) + " leaf entries";
    }
    if (!why.empty()) return fail(PFQ_ERR_UNSUPPORTED, "abundance log: " + why + ": nothing was absorbed");
    // staged through host memory: the replicas may sit on different devices, and this runs once per job
    std::vector<unsigned long long> start(s.ab_rows), uq(nl), uq_d(nl);
    std::vector<uint32_t> len(s.ab_rows), ent(s.ab_entries);
    PFQ_TRY(use_device(s.device));
    if (s.ab_rows) {
        HIP_TRY(hipMemcpy(start.data(), s.d_ab_start.p, s.ab_rows * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(len.data(), s.d_ab_len.p, s.ab_rows * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ent.data(), s.d_ab_entries.p, s.ab_entries * 4, hipMemcpyDeviceToHost));
    }
    if (s.d_ab_unique.p) HIP_TRY(hipMemcpy(uq.data(), s.d_ab_unique.p, nl * 8, hipMemcpyDeviceToHost));
    for (auto &v : start) v += d.ab_entries;  // src's entries follow dst's
    PFQ_TRY(use_device(d.device));
    if (s.ab_rows) {
        HIP_TRY(hipMemcpy(d.d_ab_start.p + d.ab_rows, start.data(), s.ab_rows * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d.d_ab_len.p + d.ab_rows, len.data(), s.ab_rows * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d.d_ab_entries.p + d.ab_entries, ent.data(), s.ab_entries * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(uq_d.data(), d.d_ab_unique.p, nl * 8, hipMemcpyDeviceToHost));
    for (size_t l = 0; l < nl; ++l) uq_d[l] += uq[l];
    HIP_TRY(hipMemcpy(d.d_ab_unique.p, uq_d.data(), nl * 8, hipMemcpyHostToDevice));
    d.ab_rows += s.ab_rows;
    d.ab_entries += s.ab_entries;
    d.ab_units += s.ab_units;
    d.ab_unhit += s.ab_unhit;
    d.ab_unique += s.ab_unique;
    d.ab_all += s.ab_all;
    PFQ_TRY(use_device(s.device));
    abund_clear(s);
    PFQ_TRY(use_device(d.device));
    return PFQ_OK;
}

int pfq_leaf_counts(pfq_tree *tree, const char *const **tax_ids, const uint64_t **counts, uint64_t *n_leaves) {
    if (!tree || !n_leaves) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(build_layout(t));
    PFQ_TRY(sync_counts_to_nodes(t));
    t.out_tax.clear();
    t.out_counts.clear();
    for (int32_t v : t.leaves) {
        t.out_tax.push_back(t.nodes[v].tax_id);
        t.out_counts.push_back(t.nodes[v].mapped_reads);
    }
    t.out_tax_ptr.clear();
    for (auto &s : t.out_tax) t.out_tax_ptr.push_back(s.c_str());
    if (tax_ids) *tax_ids = t.out_tax_ptr.data();
    if (counts) *counts = t.out_counts.data();
    *n_leaves = t.leaves.size();
    return PFQ_OK;
}

int pfq_save_leaf_counts(pfq_tree *tree, const char *csv_path) {
    if (!tree || !csv_path) return fail(PFQ_ERR_ARG, "null argument");
    const char *const *ids = nullptr;
    const uint64_t *cnt = nullptr;
    uint64_t n = 0;
    PFQ_TRY(pfq_leaf_counts(tree, &ids, &cnt, &n));
    FILE *f = fopen(csv_path, "wb");
    if (!f) return fail(PFQ_ERR_IO, std::string("cannot create ") + csv_path + ": " + strerror(errno));
    for (uint64_t i = 0; i < n; ++i)
        if (cnt[i] > 0) fprintf(f, "%s,%llu\n", ids[i], (unsigned long long)cnt[i]);  // query.rs:177-182
    if (fclose(f) != 0) return fail(PFQ_ERR_IO, "short write to CLASSIFICATION.csv");
    return PFQ_OK;
}

int pfq_leaf_counts_export(pfq_tree *tree, uint64_t *d_dst, void *stream) {
    if (!tree || !d_dst) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    PFQ_TRY(build_layout(*tree));
    if (!tree->leaves.empty())
        HIP_TRY(hipMemcpyAsync(d_dst, tree->d_counts.p, tree->leaves.size() * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PFQ_OK;
}
int pfq_leaf_counts_import(pfq_tree *tree, const uint64_t *d_src, void *stream) {
    if (!tree || !d_src) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    PFQ_TRY(build_layout(*tree));
    if (!tree->leaves.empty()) {
        HIP_TRY(hipMemcpyAsync(tree->d_counts.p, d_src, tree->leaves.size() * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        HIP_TRY(hipMemcpyAsync(tree->d_counts_base.p, d_src, tree->leaves.size() * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return PFQ_OK;
}
int pfq_leaf_counts_export_delta(pfq_tree *tree, uint64_t *d_dst, void *stream) {
    if (!tree || !d_dst) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    PFQ_TRY(build_layout(*tree));
    pfq::launch_counts_op(reinterpret_cast<unsigned long long *>(d_dst), tree->d_counts.p, tree->d_counts_base.p, (uint32_t)tree->leaves.size(), true,
                          (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return PFQ_OK;
}
int pfq_leaf_counts_import_delta(pfq_tree *tree, const uint64_t *d_src, void *stream) {
    if (!tree || !d_src) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    PFQ_TRY(build_layout(*tree));
    const uint32_t nl = (uint32_t)tree->leaves.size();
    pfq::launch_counts_op(tree->d_counts.p, tree->d_counts_base.p, reinterpret_cast<const unsigned long long *>(d_src), nl, false, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    if (nl) HIP_TRY(hipMemcpyAsync(tree->d_counts_base.p, tree->d_counts.p, (size_t)nl * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PFQ_OK;
}
// ---- several replicas behind one process: one RCCL all-reduce of the per-leaf counters -------------------------------
extern "C++" {
namespace {
struct Rccl {
    void *handle = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string error;
};
Rccl &rccl() {  // loaded once per process; RCCL is a run-time dependency of multi-GPU runs only
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        // (RTLD_LOCAL: an embedding framework may bring an RCCL of its own — PyTorch does — and the two must not see each
        // other's symbols)
        r.handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!r.handle) r.handle = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!r.handle) {
            r.error = std::string("cannot load librccl: ") + dlerror();
            return;
        }
        auto sym = [&](const char *name) {
            void *p = dlsym(r.handle, name);
            if (!p && r.error.empty()) r.error = std::string("librccl lacks ") + name;
            return p;
        };
        r.CommInitAll = (decltype(r.CommInitAll))sym("ncclCommInitAll");
        r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
        r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
        r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
        r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
        r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    });
    return r;
}
thread_local uint32_t g_last_ranks = 0;
// The communicator of a device set is made on first use and kept while the process has a tree open (a caller may reduce
// after every block; ncclCommInitAll costs seconds).  Destroyed with the last tree — not at process exit, where the HIP
// runtime and other users of it (an embedding framework) are already tearing down.
std::mutex g_comm_mutex;
std::map<std::vector<int>, std::vector<ncclComm_t>> g_comm_cache;
}  // namespace
}  // extern "C++"
namespace {
void release_communicators() {
    std::lock_guard<std::mutex> lock(g_comm_mutex);
    if (g_comm_cache.empty()) return;
    Rccl &r = rccl();
    for (auto &kv : g_comm_cache)
        for (auto c : kv.second) (void)r.CommDestroy(c);
    g_comm_cache.clear();
}
}  // namespace

uint32_t pfq_last_allreduce_ranks(void) { return g_last_ranks; }

int pfq_device_count(int *n) {
    if (!n) return fail(PFQ_ERR_ARG, "null argument");
    *n = 0;
    if (hipGetDeviceCount(n) != hipSuccess || *n <= 0) {
        (void)hipGetLastError();
        *n = 0;
        return fail(PFQ_ERR_DEVICE, "no HIP device available (libpfq has no CPU fallback)");
    }
    return PFQ_OK;
}

int pfq_trees_allreduce_counts(pfq_tree *const *trees, uint32_t n_trees) {
    g_last_ranks = 0;
    if (!trees || n_trees == 0) return fail(PFQ_ERR_ARG, "null argument");
    for (uint32_t i = 0; i < n_trees; ++i)
        if (!trees[i]) return fail(PFQ_ERR_ARG, "null tree");
    // every replica: same leaf set, queued work finished
    std::map<int, std::vector<pfq_tree *>> by_dev;  // device -> replicas on it, the first one leads
    for (uint32_t i = 0; i < n_trees; ++i) {
        pfq_tree &t = *trees[i];
        for (uint32_t j = 0; j < i; ++j)
            if (trees[j] == trees[i]) return fail(PFQ_ERR_ARG, "the same tree listed twice");
        PFQ_TRY(use_device(t.device));
        PFQ_TRY(build_layout(t));
        HIP_TRY(hipDeviceSynchronize());
        if (t.leaves.size() != trees[0]->leaves.size())
            return fail(PFQ_ERR_ARG, "the trees are not replicas of one database: " + std::to_string(t.leaves.size()) + " vs " +
                                         std::to_string(trees[0]->leaves.size()) + " leaves");
        for (size_t l = 0; l < t.leaves.size(); ++l)
            if (t.nodes[t.leaves[l]].tax_id != trees[0]->nodes[trees[0]->leaves[l]].tax_id)
                return fail(PFQ_ERR_ARG, "the trees are not replicas of one database: leaf " + std::to_string(l) + " differs");
        by_dev[t.device].push_back(&t);
    }
    const uint32_t nl = (uint32_t)trees[0]->leaves.size();
    if (n_trees == 1 || nl == 0) return PFQ_OK;
    // What a replica adds to the job is what it counted since it was opened (or last reduced): counters - base.  The stored
    // mapped_reads of a database that was saved after a query are in every replica's base and must count once, as on one
    // device and in the reference (query.rs:143 accumulates on the loaded value).
    // (1) every replica's delta; replicas that share a device are added into the device's first replica
    for (auto &kv : by_dev) {
        HIP_TRY(hipSetDevice(kv.first));
        for (size_t r = 0; r < kv.second.size(); ++r) {
            pfq_tree &t = *kv.second[r];
            pfq::launch_counts_op(t.d_counts_delta.p, t.d_counts.p, t.d_counts_base.p, nl, true, nullptr);
            if (r) pfq::launch_counts_op(kv.second[0]->d_counts_delta.p, kv.second[0]->d_counts_delta.p, t.d_counts_delta.p, nl, false, nullptr);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    // (2) one all-reduce (sum, u64[n_leaves]) over RCCL across the devices, in place in each device's first replica.
    // Replicas that all share one device need no communicator (loading librccl and ncclCommInitAll cost seconds);
    // PFQ_RCCL_ALWAYS=1 makes a one-rank communicator anyway, so that the RCCL path can be exercised on a one-GPU box.
    // The communicator of a device set is made once per process and kept (a caller may reduce after every block).
    const char *always = getenv("PFQ_RCCL_ALWAYS");
    if (by_dev.size() > 1 || (always && atoi(always) != 0)) {
        Rccl &r = rccl();
        if (!r.error.empty()) return fail(PFQ_ERR_DEVICE, r.error);
        std::vector<int> devs;
        for (auto &kv : by_dev) devs.push_back(kv.first);
        auto &comm_cache = g_comm_cache;
        std::lock_guard<std::mutex> lock(g_comm_mutex);  // (one collective of this process at a time)
        auto it = comm_cache.find(devs);
        if (it == comm_cache.end()) {
            std::vector<ncclComm_t> fresh(devs.size());
            const ncclResult_t rc0 = r.CommInitAll(fresh.data(), (int)devs.size(), devs.data());
            if (rc0 != ncclSuccess) return fail(PFQ_ERR_DEVICE, std::string("ncclCommInitAll: ") + r.GetErrorString(rc0));
            it = comm_cache.emplace(devs, std::move(fresh)).first;
        }
        std::vector<ncclComm_t> &comms = it->second;
        ncclResult_t rc = r.GroupStart();
        for (size_t i = 0; i < devs.size() && rc == ncclSuccess; ++i) {
            (void)hipSetDevice(devs[i]);
            unsigned long long *buf = by_dev[devs[i]][0]->d_counts_delta.p;
            rc = r.AllReduce(buf, buf, nl, ncclUint64, ncclSum, comms[i], nullptr);
        }
        const ncclResult_t rc_end = r.GroupEnd();
        if (rc == ncclSuccess) rc = rc_end;
        hipError_t he = hipSuccess;
        for (size_t i = 0; i < devs.size(); ++i) {
            (void)hipSetDevice(devs[i]);
            const hipError_t e = hipDeviceSynchronize();
            if (he == hipSuccess) he = e;
        }
        if (rc != ncclSuccess || he != hipSuccess) {  // a communicator that failed is not reused
            for (auto c : comms) (void)r.CommDestroy(c);
            comm_cache.erase(it);
        }
        if (rc != ncclSuccess) return fail(PFQ_ERR_DEVICE, std::string("ncclAllReduce: ") + r.GetErrorString(rc));
        if (he != hipSuccess) return fail(PFQ_ERR_DEVICE, std::string("all-reduce of the leaf counters: ") + hipGetErrorString(he));
        g_last_ranks = (uint32_t)devs.size();
    }
    // (3) every replica: counters = its base + the job's delta, and that is its new base (a second call changes nothing)
    for (auto &kv : by_dev) {
        HIP_TRY(hipSetDevice(kv.first));
        const unsigned long long *total = kv.second[0]->d_counts_delta.p;
        for (size_t q = 0; q < kv.second.size(); ++q) {
            pfq_tree &t = *kv.second[q];
            pfq::launch_counts_op(t.d_counts.p, t.d_counts_base.p, total, nl, false, nullptr);
            HIP_TRY(hipMemcpyAsync(t.d_counts_base.p, t.d_counts.p, (size_t)nl * 8, hipMemcpyDeviceToDevice, nullptr));
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    return PFQ_OK;
}

int pfq_leaf_counts_reset(pfq_tree *tree) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    PFQ_TRY(build_layout(*tree));
    HIP_TRY(hipDeviceSynchronize());
    if (!tree->leaves.empty()) {
        HIP_TRY(hipMemset(tree->d_counts.p, 0, tree->leaves.size() * 8));
        HIP_TRY(hipMemset(tree->d_counts_base.p, 0, tree->leaves.size() * 8));
        if (tree->lca_valid) HIP_TRY(hipMemset(tree->d_clade_here.p, 0, tree->clades.size() * 8));
        PFQ_TRY(tax_zero(*tree));
    }
    for (auto &nd : tree->nodes) nd.mapped_reads = nd.base_reads = 0;
    abund_clear(*tree);
    cover_clear(*tree);
    PFQ_TRY(sweep_zero(*tree));
    return PFQ_OK;
}

int pfq_last_stats(pfq_tree *tree, pfq_stats *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    memset(out, 0, sizeof *out);
    if (!t.d_stats.p) return PFQ_OK;
    PFQ_TRY(wait_last_call(t));
    unsigned long long h[pfq::ST_N];
    HIP_TRY(hipMemcpy(h, t.d_stats.p, sizeof h, hipMemcpyDeviceToHost));
    out->n_reads = t.last_n_reads;
    out->n_candidates = h[pfq::ST_CANDIDATES];
    out->n_hits = h[pfq::ST_HITS];
    out->n_allhit_reads = h[pfq::ST_ALLHIT];
    out->algorithmic_bytes = h[pfq::ST_ALG_BYTES];
    out->path = t.last_path;
    out->n_slices = t.last_slices;
    out->tile_mode = t.last_tile_mode;
    out->tile_bin_build = t.last_tile_bin;
    if (t.d_cursors.p) {
        unsigned long long c[CUR_TAIL_SHAPES + 1];
        HIP_TRY(hipMemcpy(c, t.d_cursors.p, sizeof c, hipMemcpyDeviceToHost));
        const uint32_t shapes = t.last_path ? (uint32_t)c[CUR_TAIL_SHAPES] : 0u;  // pfq::TAIL_SHAPE_*
        out->pair_stage = t.last_sort | ((shapes & 7u) << 4) | ((shapes & pfq::TAIL_SHAPE_FULL) ? 4u : 0u) |
                          ((t.last_path && h[pfq::ST_BATCHED]) ? 8u : 0u) | ((t.last_path && t.last_tile_mode && t.last_tile_stream) ? 0x80u : 0u);
        out->entry_pack = (t.last_path && t.last_tile_mode && t.last_entry_pack) ? 1u : 0u;
        out->n_chunks = (uint32_t)c[CUR_CHUNKS_FLAGGED];
        out->n_fallback_pairs = (uint32_t)(c[CUR_CHUNKS_FLAGGED] >> 32);
        out->tile_entries = c[CUR_TILE_ENTRIES];
        if (t.last_tile_mode && t.hint_entry_cap) {
            out->tile_passes_launched = t.last_passes;
            out->tile_passes_needed = (uint32_t)std::max<uint64_t>(1, (c[CUR_TILE_ENTRIES] + t.hint_entry_cap - 1) / t.hint_entry_cap);
        }
    }
    out->leaf_groups = t.last_leaf_groups;
    out->coarse_cols = t.last_coarse_cols;
    out->coarse_probes = t.last_coarse_probes;
    out->group_reads = h[pfq::ST_LISTED];
    return PFQ_OK;
}
int pfq_profile_begin(pfq_tree *tree, uint32_t max_calls) {
    if (!tree) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    if (t.prof_ev.size() < PROF_EV * (size_t)max_calls) t.prof_ev.resize(PROF_EV * (size_t)max_calls);
    for (Event &e : t.prof_ev) HIP_TRY(e.ensure());
    t.prof_cap = max_calls;
    t.prof_used = 0;
    t.prof_bucketed.assign(max_calls, 0);
    return PFQ_OK;
}
int pfq_profile_end(pfq_tree *tree, pfq_profile *out) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    memset(out, 0, sizeof *out);
    PFQ_TRY(wait_last_call(t));
    for (size_t c = 0; c < t.prof_used; ++c) {
        const Event *ev = &t.prof_ev[PROF_EV * c];
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        out->classify_ms += ms;
        if (t.prof_bucketed[c]) {
            HIP_TRY(hipEventElapsedTime(&ms, ev[1], ev[2]));
            out->bucket_ms += ms;
            HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[3]));
            out->bin_ms += ms;
            HIP_TRY(hipEventElapsedTime(&ms, ev[3], ev[4]));
            out->test_ms += ms;
            HIP_TRY(hipEventElapsedTime(&ms, ev[4], ev[5]));
            out->verify_ms += ms;
            HIP_TRY(hipEventElapsedTime(&ms, ev[5], ev[6]));
            out->finalize_ms += ms;
        }
    }
    out->calls = t.prof_used;
    t.prof_cap = t.prof_used = 0;
    return PFQ_OK;
}
int pfq_set_option(pfq_tree *tree, const char *name, const char *value) {
    if (!tree || !name) return fail(PFQ_ERR_ARG, "null argument");
    if (!strcmp(name, "PFQ_COVER_P")) {  // the precision of the coverage sketch: in range, and not changed under a sketch that holds units
        Knobs k = tree->knobs;
        set_knob(k, name, value);
        if (k.cover_p != -1 && (k.cover_p < (long long)pfq::COVER_P_MIN || k.cover_p > (long long)pfq::COVER_P_MAX))
            return fail(PFQ_ERR_ARG, std::string("PFQ_COVER_P must be 4..16, not ") + value);
        if (tree->d_cov_regs.p && cover_precision(k) != tree->cov_p) {
            if (tree->cov_units)
                return fail(PFQ_ERR_STATE, "PFQ_COVER_P cannot change while the coverage sketch holds units (precision " + std::to_string(tree->cov_p) +
                                           "); pfq_coverage_reset empties it");
            PFQ_TRY(use_device(tree->device));
            HIP_TRY(hipDeviceSynchronize());
            cover_clear(*tree);  // (made by a call without units: the next flagged call makes it anew)
        }
    }
    if (!strcmp(name, "PFQ_TEXT_TILE") && value && *value) {  // the text a block scans: a power of two, at most the built-in
        const long long v = strtoll(value, nullptr, 10);
        if (v < (long long)pfq::TEXT_TILE_MIN || v > (long long)pfq::TEXT_TILE_DEFAULT || (v & (v - 1)))
            return fail(PFQ_ERR_ARG, std::string("PFQ_TEXT_TILE must be a power of two from 256 to 8192, not ") + value);
    }
    if (!strcmp(name, "PFQ_FMT_HASH_BITS") && value && *value) {  // bits of the id hash pfq_text_format keeps
        const long long v = strtoll(value, nullptr, 10);
        if (v < 1 || v > 64) return fail(PFQ_ERR_ARG, std::string("PFQ_FMT_HASH_BITS must be 1 .. 64, not ") + value);
    }
    if (!strcmp(name, "PFQ_FMT_GRID") && value && *value) {  // a cap on the grids of pfq_text_format
        const long long v = strtoll(value, nullptr, 10);
        if (v < 1 || v > 65535) return fail(PFQ_ERR_ARG, std::string("PFQ_FMT_GRID must be 1 .. 65535, not ") + value);
    }
    if (!strcmp(name, "PFQ_INFLATE_BLOCKS") && value && *value) {  // a cap on the grid of k_gz_inflate
        const long long v = strtoll(value, nullptr, 10);
        if (v < 1 || v > 65535) return fail(PFQ_ERR_ARG, std::string("PFQ_INFLATE_BLOCKS must be 1 .. 65535, not ") + value);
    }
    if (!strcmp(name, "PFQ_DEFLATE_BLOCKS") && value && *value) {  // a cap on the grid of k_bgzf_deflate
        const long long v = strtoll(value, nullptr, 10);
        if (v < 1 || v > 65535) return fail(PFQ_ERR_ARG, std::string("PFQ_DEFLATE_BLOCKS must be 1 .. 65535, not ") + value);
    }
    if (!strcmp(name, "PFQ_FRAME_PIECE") && value && *value) {  // the windows of a piece are whole: a positive multiple of 64
        const long long v = strtoll(value, nullptr, 10);
        if (v <= 0 || v % 64 || v > (1ll << 30)) return fail(PFQ_ERR_ARG, std::string("PFQ_FRAME_PIECE must be a positive multiple of 64 up to 2^30, not ") + value);
    }
    if (!set_knob(tree->knobs, name, value)) return fail(PFQ_ERR_ARG, std::string("unknown option ") + name);
    // knobs of the device layout (column groups, coarse level): the layout is rebuilt before the next use
    if (!strcmp(name, "PFQ_COARSE") || !strcmp(name, "PFQ_COARSE_COLS") || !strcmp(name, "PFQ_GROUP_LOG2") || !strcmp(name, "PFQ_COARSE_MIN_LEAVES") ||
        !strcmp(name, "PFQ_TILE_LISTS")) {  // (the position slots are made with the layout)
        if (tree->layout_valid) {
            PFQ_TRY(use_device(tree->device));
            PFQ_TRY(sync_counts_to_nodes(*tree));
            tree->layout_valid = false;
            tree->drop_tile_lists();
        }
    }
    return PFQ_OK;
}
int pfq_set_path(pfq_tree *tree, int path) {
    if (!tree || path < -1 || path > 1) return fail(PFQ_ERR_ARG, "bad argument");
    tree->force_path = path;
    return PFQ_OK;
}

int pfq_debug_last_capacity(pfq_tree *tree, uint64_t *out, uint64_t n) {
    if (!tree || (n && !out)) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    uint64_t v[PFQ_CAPACITY_N] = {};
    if (t.d_cursors.p) {
        PFQ_TRY(wait_last_call(t));
        unsigned long long c[CUR_KMISS + 1];
        HIP_TRY(hipMemcpy(c, t.d_cursors.p, sizeof c, hipMemcpyDeviceToHost));
        uint32_t sorted = 0;
        if (t.last_nb && t.d_bucket.n > 2 * t.last_nb) HIP_TRY(hipMemcpy(&sorted, t.d_bucket.p + 2 * t.last_nb, 4, hipMemcpyDeviceToHost));
        const uint64_t w[PFQ_CAPACITY_N] = {c[CUR_PAIR], t.last_pair_cap, c[CUR_GUARD], t.last_guard_cap, c[CUR_MISS_WORDS], t.last_miss_cap, c[CUR_KMISS], t.last_kmiss_cap,
                                            t.last_hit_cursor0, t.last_hit_cap0, t.last_attempts, sorted};
        if (t.last_path) memcpy(v, w, sizeof v);
        else v[8] = w[8], v[9] = w[9], v[10] = w[10];  // (the direct path has no pair buffers)
    }
    for (uint64_t i = 0; i < n && i < PFQ_CAPACITY_N; ++i) out[i] = v[i];
    return PFQ_OK;
}

int pfq_tile_lists_info(pfq_tree *tree, uint64_t out[4]) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(build_layout(t));
    out[0] = t.tile_list_cols;
    out[1] = t.tile_list_cols ? t.d_tile_lists.bytes() : 0;
    out[2] = out[3] = 0;
    if (t.d_cursors.p) {
        PFQ_TRY(wait_last_call(t));
        unsigned long long c[2];
        HIP_TRY(hipMemcpy(c, t.d_cursors.p + CUR_TILE_LIST, sizeof c, hipMemcpyDeviceToHost));
        out[2] = c[0];
        out[3] = c[1];
    }
    return PFQ_OK;
}
int pfq_screen_info(pfq_tree *tree, double out[4]) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(build_layout(t));
    PFQ_TRY(cover_filter_bits(t));
    out[0] = t.last_path ? (double)t.last_screen_kmers : 0.0;
    out[1] = t.screen_E;
    out[2] = (double)t.rw;
    out[3] = (double)t.n_groups;
    return PFQ_OK;
}
int pfq_pair_info(pfq_tree *tree, uint64_t out[4]) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (t.last_path && t.d_stats.p) {
        PFQ_TRY(wait_last_call(t));
        unsigned long long r = 0;
        HIP_TRY(hipMemcpy(&r, t.d_stats.p + pfq::ST_PAIR_RESERVATIONS, sizeof r, hipMemcpyDeviceToHost));
        out[1] = t.last_pair_ahead;
        out[2] = r;
    }
    return PFQ_OK;
}
int pfq_debug_tile_list(pfq_tree *tree, uint64_t col, uint64_t tile, uint32_t *out, uint64_t n) {
    if (!tree || (n && !out)) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    PFQ_TRY(build_layout(t));
    const uint64_t n_tiles = (t.n_words * 64 + (1ull << pfq::TILE_LOG2) - 1) >> pfq::TILE_LOG2;
    if (col >= t.n_cols || tile >= n_tiles) return fail(PFQ_ERR_ARG, "column / tile out of range");
    uint32_t row = pfq::TILE_LIST_NONE;
    if (t.tile_list_cols) HIP_TRY(hipMemcpy(&row, t.d_tile_list_row.p + col, 4, hipMemcpyDeviceToHost));
    if (row == pfq::TILE_LIST_NONE) return fail(PFQ_ERR_STATE, "column " + std::to_string(col) + " has no position slots (its tiles are loaded dense)");
    HIP_TRY(hipMemcpy(out, t.d_tile_lists.p + (row * n_tiles + tile) * pfq::TILE_LIST_CAP, std::min<uint64_t>(n, pfq::TILE_LIST_CAP) * 4, hipMemcpyDeviceToHost));
    return PFQ_OK;
}

int pfq_debug_tile_bucket(pfq_tree *tree, uint64_t chunk, uint64_t tile, uint32_t *out, uint64_t cap) {
    if (!tree || !out) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    if (!t.d_cursors.p || !t.last_tile_mode || t.last_block_mode || !t.last_n_tiles) return fail(PFQ_ERR_STATE, "the last call ran no LDS-tile pass at threshold 1");
    if (cap < PFQ_TILE_BUCKET_WORDS) return fail(PFQ_ERR_ARG, "the buffer holds less than the header and the tables");
    PFQ_TRY(wait_last_call(t));
    unsigned long long n_chunks = 0;
    HIP_TRY(hipMemcpy(&n_chunks, t.d_cursors.p + CUR_CHUNKS_FLAGGED, 8, hipMemcpyDeviceToHost));
    n_chunks = std::min<uint64_t>(n_chunks & 0xffffffffu, t.d_chunks.n);
    memset(out, 0, PFQ_TILE_BUCKET_WORDS * 4);
    out[7] = (uint32_t)n_chunks;
    if (chunk >= n_chunks || tile >= t.last_n_tiles) return fail(PFQ_ERR_ARG, "chunk / tile out of range");
    pfq::ChunkDesc dsc;
    HIP_TRY(hipMemcpy(&dsc, t.d_chunks.p + chunk, sizeof dsc, hipMemcpyDeviceToHost));
    uint32_t fill = 0;
    HIP_TRY(hipMemcpy(&fill, t.d_gfill.p + chunk * t.last_n_tiles + tile, 4, hipMemcpyDeviceToHost));
    out[0] = fill;
    out[1] = t.last_entry_pack ? pfq::pack_bucket_words(dsc.cap) : dsc.cap;
    out[2] = dsc.first;
    out[3] = dsc.n;
    out[4] = dsc.leaf;
    out[5] = dsc.pass;
    out[6] = t.last_entry_pack ? 1u : 0u;
    if (t.last_entry_pack) {
        HIP_TRY(hipMemcpy(out + 8, t.d_n_rounds.p + chunk, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out + 16, t.d_round_p0.p + chunk * pfq::PACK_ROUNDS, pfq::PACK_ROUNDS * 4, hipMemcpyDeviceToHost));
    }
    std::vector<uint2> pairs(dsc.n);
    if (dsc.n) HIP_TRY(hipMemcpy(pairs.data(), t.d_sorted.p + dsc.first, dsc.n * sizeof(uint2), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < dsc.n && i < (1u << pfq::CHUNK_PAIRS_LOG2); ++i) out[16 + pfq::PACK_ROUNDS + i] = pairs[i].x;
    const uint64_t words = std::min<uint64_t>(std::min(fill, out[1]), cap - PFQ_TILE_BUCKET_WORDS);
    if (words) HIP_TRY(hipMemcpy(out + PFQ_TILE_BUCKET_WORDS, t.d_entries.p + dsc.base + tile * dsc.cap, words * 4, hipMemcpyDeviceToHost));
    return PFQ_OK;
}

int pfq_debug_kmer_indices(pfq_tree *tree, const uint8_t *seq, uint64_t len, uint64_t *out_idx, uint64_t *n_kmers) {
    if (!tree || !n_kmers || (len && !seq)) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    pfq_tree &t = *tree;
    uint64_t n = (t.kmer_size >= 1 && len >= t.kmer_size) ? len - t.kmer_size + 1 : 0;
    *n_kmers = n;
    if (!n || !out_idx) return PFQ_OK;
    DevBuf<uint8_t> d_s;
    DevBuf<uint64_t> d_o;
    HIP_TRY(d_s.ensure(len + 16));
    HIP_TRY(d_o.ensure(n * t.num_hashes));
    HIP_TRY(hipMemcpy(d_s.p, seq, len, hipMemcpyHostToDevice));
    pfq::launch_debug_indices(t.hp, d_s.p, len, d_o.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_idx, d_o.p, n * t.num_hashes * 8, hipMemcpyDeviceToHost));
    return PFQ_OK;
}

int pfq_debug_node_filter(pfq_tree *tree, uint64_t node, uint64_t *out_words, uint64_t n_words) {
    if (!tree || !out_words) return fail(PFQ_ERR_ARG, "null argument");
    PFQ_TRY(use_device(tree->device));
    PFQ_TRY(finish_topology(*tree));
    if (node >= tree->nodes.size() || n_words != tree->n_words) return fail(PFQ_ERR_ARG, "node / n_words out of range");
    HIP_TRY(hipMemcpy(out_words, tree->d_bits.p + (uint64_t)tree->nodes[node].filter * tree->n_words, n_words * 8,
                      hipMemcpyDeviceToHost));
    return PFQ_OK;
}

int pfq_synth_genomes_device(uint8_t *d_out, uint64_t n_genomes, uint64_t genome_len, uint64_t seed_base, void *stream) {
    if (!d_out) return fail(PFQ_ERR_ARG, "null argument");
    pfq::launch_synth_genomes(d_out, n_genomes, genome_len, seed_base, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return PFQ_OK;
}
int pfq_synth_reads_device(uint8_t *d_out, uint64_t first_read, uint64_t n_reads, uint64_t read_len, const uint8_t *d_genomes,
                           uint64_t genome_len, uint64_t n_genomes, uint64_t seed, void *stream) {
    if (!d_out) return fail(PFQ_ERR_ARG, "null argument");
    pfq::launch_synth_reads(d_out, first_read, n_reads, read_len, d_genomes, genome_len, n_genomes, seed, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return PFQ_OK;
}

}  // extern "C"
