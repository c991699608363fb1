// pfq_tax.hip — PFQ_WANT_TAXA: every unit (read, or fragment with PFQ_PAIRED) is counted on the nodes of a taxonomy the user
// has laid over the leaves (pfq.h "taxonomy", DESIGN.md §5 "Taxonomy").  A post-stage on the call's final CSR: no kernel of
// pfq_kernels.hip or pfq_lca.hip is involved.
//
// Nodes are in pre-order and every node covers a contiguous range of ranks (rank = a genome's position in that order), so
//   taxon(row) = the shallowest (= smallest) gap node between the row's lowest and highest rank: one range minimum, two loads
//     of one level of a sparse table, as in k_lca_map — but the rows ascend in leaf index, not in rank, so the two ends are
//     the minimum and the maximum of rank[leaf] over the row;
//   any: entry e is the first genome of its row inside node t exactly when first_rank[t] > p(e), p(e) = the largest rank of
//     the row below rank(e) (-1: none): no row entry lies in [first_rank[t], rank(e)).  first_rank does not grow on the way up,
//     so the walk t = leaf_node[e], parent[t], .. stops at the first node that fails, and over the row every touched node is
//     counted once — without sorting the row and without a visited set.
// Nodes 0 .. top (the root and the one-child chain below it, top = the deepest node above every genome) are touched by every
// unit with a hit: the walks stop below them and the units are counted with a ballot.  A row that lists all n_leaves leaves
// walks nothing: it is a unit on `top` and on every node's `any`, counted in misc[TAX_MISC_ALL] and applied at read-out.
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

constexpr uint32_t TAX_ROW_SHORT = 64;  // entries a single thread takes (as LCA_ROW_SHORT); longer rows are queued for a wave

struct TaxArgs {
    const unsigned long long *off;
    const uint32_t *leaves;
    uint64_t n_units;
    TaxTables tb;
    uint32_t *node;               // [n_units]
    uint32_t *long_list;          // [n_units]
    unsigned long long *n_long;
};

// lowest common node of the ranks lo <= hi; leaf_lo: the leaf at rank lo
__device__ __forceinline__ uint32_t tax_lca(const TaxTables &tb, uint32_t lo, uint32_t hi, uint32_t leaf_lo) {
    if (lo == hi) return tb.leaf_node[leaf_lo];
    const uint32_t j = 31u - (uint32_t)__clz((int)(hi - lo));  // gaps lo .. hi - 1
    const uint32_t *lvl = tb.gap_min + (uint64_t)j * tb.n_leaves;
    return min(lvl[lo], lvl[hi - (1u << j)]);
}
// index of t among the hot nodes, TAX_HOT: none (unused slots hold TAX_NO_NODE, which is no node)
__device__ __forceinline__ uint32_t tax_hot_index(const TaxTables &tb, uint32_t t) {
    uint32_t k = TAX_HOT;
#pragma unroll
    for (uint32_t i = 0; i < TAX_HOT; ++i)
        if (t == tb.hot[i]) k = i;
    return k;
}

// Rows of up to TAX_ROW_SHORT entries, a thread each.  LDS: `here` and `any` are counted in two u32 histograms of the block
// (a block's count of one node is at most its units; dynamic LDS, 8 n_nodes bytes: a small taxonomy leaves the CU its
// occupancy, TAX_HIST_LDS nodes take the 64 KiB a block may have) and flushed once per node; else global atomics.  What every lane of a
// wave would add to one address — the units with a hit, the all-leaf units, `here` of top and both counters of the hot nodes
// (the heaviest child chain below top) — is counted with ballots into wave-uniform registers and added once per wave at the end.
template <bool LDS>
__global__ void __launch_bounds__(256) k_tax_rows(TaxArgs a) {
    extern __shared__ uint32_t tax_hist[];  // LDS: [2][n_nodes]
    const TaxTables &tb = a.tb;
    uint32_t *const h_here = tax_hist, *const h_any = tax_hist + (LDS ? tb.n_nodes : 0);
    if (LDS) {
        for (uint32_t c = threadIdx.x; c < tb.n_nodes; c += blockDim.x) h_here[c] = h_any[c] = 0;
        __syncthreads();
    }
    const uint32_t lane = lane_id(), top = tb.top_node;
    uint32_t n_hit = 0, n_all = 0, n_top = 0;                    // wave-uniform
    uint32_t c_here0 = 0, c_here1 = 0, c_here2 = 0, c_here3 = 0;  // units on / touching hot node 0 .. 3
    uint32_t c_any0 = 0, c_any1 = 0, c_any2 = 0, c_any3 = 0;
    static_assert(TAX_HOT == 4, "the hot counters are named one by one");
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < a.n_units; base += stride) {  // (base is wave-uniform)
        const uint64_t u = base + threadIdx.x;
        const bool valid = u < a.n_units;
        uint32_t node = TAX_NO_NODE, hot_here = 0, hot_any = 0;
        bool all = false, queued = false;
        if (valid) {
            const unsigned long long o0 = a.off[u], o1 = a.off[u + 1];
            const unsigned long long len = o1 - o0;
            if (len == 0) {
            } else if (len == tb.n_leaves) {
                all = true;
                node = top;
            } else if (len > TAX_ROW_SHORT) {
                queued = true;
                a.long_list[atomicAdd(a.n_long, 1ull)] = (uint32_t)u;
            } else {
                uint32_t lo = 0xffffffffu, hi = 0, leaf_lo = 0;
                for (unsigned long long j = o0; j < o1; ++j) {
                    const uint32_t l = a.leaves[j], r = tb.rank[l];
                    if (r < lo) {
                        lo = r;
                        leaf_lo = l;
                    }
                    hi = max(hi, r);
                }
                node = tax_lca(tb, lo, hi, leaf_lo);
                if (node != top) {
                    const uint32_t k = tax_hot_index(tb, node);
                    if (k < TAX_HOT) hot_here = 1u << k;
                    else if (LDS) atomicAdd(&h_here[node], 1u);
                    else atomicAdd(&tb.here[node], 1ull);
                }
                for (unsigned long long e = o0; e < o1; ++e) {
                    const uint32_t l = a.leaves[e], r = tb.rank[l];
                    int32_t p = -1;  // the row's largest rank below r (the row is re-read: the L1 serves it)
                    for (unsigned long long j = o0; j < o1; ++j) {
                        const uint32_t q = tb.rank[a.leaves[j]];
                        if (q < r) p = max(p, (int32_t)q);
                    }
                    for (uint32_t t = tb.leaf_node[l]; t > top && (int32_t)tb.first_rank[t] > p; t = tb.parent[t]) {
                        const uint32_t k = tax_hot_index(tb, t);
                        if (k < TAX_HOT) hot_any |= 1u << k;
                        else if (LDS) atomicAdd(&h_any[t], 1u);
                        else atomicAdd(&tb.any[t], 1ull);
                    }
                }
            }
            if (!queued) a.node[u] = node;
        }
        n_hit += (uint32_t)__popcll(ballot64(node != TAX_NO_NODE));
        n_all += (uint32_t)__popcll(ballot64(all));
        n_top += (uint32_t)__popcll(ballot64(node == top && !all));
        c_here0 += (uint32_t)__popcll(ballot64((hot_here & 1u) != 0));
        c_here1 += (uint32_t)__popcll(ballot64((hot_here & 2u) != 0));
        c_here2 += (uint32_t)__popcll(ballot64((hot_here & 4u) != 0));
        c_here3 += (uint32_t)__popcll(ballot64((hot_here & 8u) != 0));
        c_any0 += (uint32_t)__popcll(ballot64((hot_any & 1u) != 0));
        c_any1 += (uint32_t)__popcll(ballot64((hot_any & 2u) != 0));
        c_any2 += (uint32_t)__popcll(ballot64((hot_any & 4u) != 0));
        c_any3 += (uint32_t)__popcll(ballot64((hot_any & 8u) != 0));
    }
    if (lane == 0) {
        if (n_hit) atomicAdd(&tb.misc[TAX_MISC_HIT], (unsigned long long)n_hit);
        if (n_all) atomicAdd(&tb.misc[TAX_MISC_ALL], (unsigned long long)n_all);
        if (n_top) atomicAdd(&tb.here[top], (unsigned long long)n_top);
        if (c_here0) atomicAdd(&tb.here[tb.hot[0]], (unsigned long long)c_here0);
        if (c_here1) atomicAdd(&tb.here[tb.hot[1]], (unsigned long long)c_here1);
        if (c_here2) atomicAdd(&tb.here[tb.hot[2]], (unsigned long long)c_here2);
        if (c_here3) atomicAdd(&tb.here[tb.hot[3]], (unsigned long long)c_here3);
        if (c_any0) atomicAdd(&tb.any[tb.hot[0]], (unsigned long long)c_any0);
        if (c_any1) atomicAdd(&tb.any[tb.hot[1]], (unsigned long long)c_any1);
        if (c_any2) atomicAdd(&tb.any[tb.hot[2]], (unsigned long long)c_any2);
        if (c_any3) atomicAdd(&tb.any[tb.hot[3]], (unsigned long long)c_any3);
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < tb.n_nodes; c += blockDim.x) {
            if (h_here[c]) atomicAdd(&tb.here[c], (unsigned long long)h_here[c]);
            if (h_any[c]) atomicAdd(&tb.any[c], (unsigned long long)h_any[c]);
        }
    }
}

// The queued rows (more than TAX_ROW_SHORT entries, not all leaves), a wave each: the lanes share the row for its two ends, then
// every lane walks from its own entries; p(e) is found by re-reading the row (every lane reads the same address: one request).
// Such rows are few: global atomics.
__global__ void __launch_bounds__(256) k_tax_long(TaxArgs a) {
    const TaxTables &tb = a.tb;
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6, top = tb.top_node;
    const uint64_t n_long = *a.n_long;
    uint32_t n_hit = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; q < n_long; q += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t u = a.long_list[q];
        const unsigned long long o0 = a.off[u], o1 = a.off[u + 1];
        unsigned long long lo = ~0ull;  // (rank << 32 | leaf) of the lowest rank
        uint32_t hi = 0;
        for (unsigned long long j = o0 + lane; j < o1; j += 64) {
            const uint32_t l = a.leaves[j], r = tb.rank[l];
            lo = min(lo, ((unsigned long long)r << 32) | l);
            hi = max(hi, r);
        }
        for (int d = 32; d > 0; d >>= 1) {
            lo = min(lo, (unsigned long long)__shfl_xor(lo, d));
            hi = max(hi, (uint32_t)__shfl_xor(hi, d));
        }
        const uint32_t node = tax_lca(tb, (uint32_t)(lo >> 32), hi, (uint32_t)lo);
        if (lane == 0) {
            a.node[u] = node;
            atomicAdd(&tb.here[node], 1ull);
        }
        ++n_hit;
        for (unsigned long long e = o0 + lane; e < o1; e += 64) {
            const uint32_t l = a.leaves[e], r = tb.rank[l];
            int32_t p = -1;
            for (unsigned long long j = o0; j < o1; ++j) {
                const uint32_t x = tb.rank[a.leaves[j]];
                if (x < r) p = max(p, (int32_t)x);
            }
            for (uint32_t t = tb.leaf_node[l]; t > top && (int32_t)tb.first_rank[t] > p; t = tb.parent[t]) atomicAdd(&tb.any[t], 1ull);
        }
    }
    if (lane == 0 && n_hit) atomicAdd(&tb.misc[TAX_MISC_HIT], (unsigned long long)n_hit);
}

void launch_tax_rows(const unsigned long long *d_off, const uint32_t *d_leaves, uint64_t n_units, const TaxTables &tb, uint32_t *d_node,
                     uint32_t *d_long, unsigned long long *d_n_long, hipStream_t st) {
    if (!n_units) return;
    TaxArgs a{};
    a.off = d_off;
    a.leaves = d_leaves;
    a.n_units = n_units;
    a.tb = tb;
    a.node = d_node;
    a.long_list = d_long;
    a.n_long = d_n_long;
    const bool lds = tb.n_nodes <= TAX_HIST_LDS;
    // LDS: a block flushes up to 2 n_nodes atomics, so it takes at least 8 units per node; global atomics: 4096 units per block
    const uint64_t per_block = lds ? std::max<uint64_t>(4096, 8ull * tb.n_nodes) : 4096;
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_units + per_block - 1) / per_block, 1024));
    if (lds) hipLaunchKernelGGL(k_tax_rows<true>, dim3(blocks), dim3(256), 2 * (size_t)tb.n_nodes * sizeof(uint32_t), st, a);
    else hipLaunchKernelGGL(k_tax_rows<false>, dim3(blocks), dim3(256), 0, st, a);
    const uint32_t wblocks = (uint32_t)std::min<uint64_t>((n_units + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 1024);
    hipLaunchKernelGGL(k_tax_long, dim3(wblocks), dim3(256), 0, st, a);
}

}  // namespace pfq
