// pfq_lca.hip — PFQ_WANT_LCA: every unit (read, or fragment with PFQ_PAIRED) is assigned to the lowest common ancestor of the
// leaves it hit, as a clade index (clades = the nodes reachable from the root, numbered in pre-order; DESIGN.md "Lowest
// common ancestor").  A post-stage on the hit sets the call has produced: no kernel of pfq_kernels.hip is involved.
//
// Leaf columns are in left-to-right DFS order, so lca(H) = lca(min H, max H), and the LCA of leaves lo < hi is the shallowest
// of the nodes that separate adjacent leaves lo..hi ("gaps": gap i lies between leaves i and i + 1, its node is their LCA).
// An ancestor comes before its descendants in pre-order, and every gap node of the range lies in the subtree of the LCA, so
// the shallowest gap node of a range is the one with the smallest clade index: a sparse table of range minima over the gaps'
// clade indices answers a unit with two loads whatever the tree's depth (a caterpillar of 131 072 leaves: 17 levels).
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

// span[u] = (lowest hit leaf, ~highest hit leaf): both fields only ever decrease, from the 0xff the host fills them with;
// (0xffffffff, 0xffffffff) = no hit.
__device__ __forceinline__ bool span_empty(const uint2 s) { return s.x == LCA_NO_CLADE; }

// Source 1 — unordered (read, leaf) hit pairs, no CSR: two atomic minima per pair on the read's span.
__global__ void __launch_bounds__(256) k_lca_span_pairs(const uint2 *__restrict__ pairs, uint64_t n_pairs, uint2 *span) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pairs; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 p = pairs[i];
        atomicMin(&span[p.x].x, p.y);
        atomicMin(&span[p.x].y, ~p.y);
    }
}

// Source 3 — PFQ_LCA_BEST: the span of the row's entries whose score is the row's maximum.  Rows are ascending, so these are
// the first and the last entry that reach it.  A thread takes a row of up to LCA_ROW_SHORT entries; longer ones (threshold
// <= 0 lists every leaf) are queued for a wave.
constexpr uint32_t LCA_ROW_SHORT = 64;
__global__ void __launch_bounds__(256) k_lca_best_span(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ leaves,
                                                       const uint32_t *__restrict__ scores, uint64_t n_units, uint2 *__restrict__ span,
                                                       uint32_t *__restrict__ long_list, unsigned long long *n_long) {
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long o0 = off[u], o1 = off[u + 1];
        if (o1 - o0 > LCA_ROW_SHORT) {
            long_list[atomicAdd(n_long, 1ull)] = (uint32_t)u;
            continue;
        }
        uint32_t best = 0, lo = LCA_NO_CLADE, hi = 0;
        for (unsigned long long j = o0; j < o1; ++j) {
            const uint32_t s = scores[j], l = leaves[j];
            if (lo == LCA_NO_CLADE || s > best) {
                best = s;
                lo = l;
            }
            if (s == best) hi = l;
        }
        span[u] = lo == LCA_NO_CLADE ? make_uint2(LCA_NO_CLADE, LCA_NO_CLADE) : make_uint2(lo, ~hi);
    }
}
__global__ void __launch_bounds__(256) k_lca_best_long(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ leaves,
                                                       const uint32_t *__restrict__ scores, const uint32_t *__restrict__ long_list,
                                                       const unsigned long long *__restrict__ n_long_ptr, uint2 *__restrict__ span) {
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t n_long = *n_long_ptr;
    for (uint64_t q = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; q < n_long; q += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t u = long_list[q];
        const unsigned long long o0 = off[u], o1 = off[u + 1];
        uint32_t best = 0;
        for (unsigned long long j = o0 + lane; j < o1; j += 64) best = max(best, scores[j]);
        for (int d = 32; d > 0; d >>= 1) best = max(best, (uint32_t)__shfl_xor(best, d));
        uint32_t lo = LCA_NO_CLADE, nhi = LCA_NO_CLADE;  // nhi = ~(highest leaf at the maximum)
        for (unsigned long long j = o0 + lane; j < o1; j += 64)
            if (scores[j] == best) {
                const uint32_t l = leaves[j];
                lo = min(lo, l);
                nhi = min(nhi, ~l);
            }
        for (int d = 32; d > 0; d >>= 1) {
            lo = min(lo, (uint32_t)__shfl_xor(lo, d));
            nhi = min(nhi, (uint32_t)__shfl_xor(nhi, d));
        }
        if (lane == 0) span[u] = make_uint2(lo, nhi);
    }
}

// (lo, hi) -> clade, lca[u], here[clade] += 1.
//   span != nullptr: spans (sources 1 and 3); allhit (source 1 only): flagged reads hit every leaf.
//   else the ends of row u of the ascending CSR off / leaves (source 2); pair_mode != 0 (fragments; 1: either, 2: both): a
//   fragment whose row is empty but whose mates' all-hit flags make it an all-leaf fragment was left unlisted and hit every leaf.
// LDS: the block counts in LDS (u32: a block's count of one clade is at most its units) and flushes once per clade; else
// global atomics.  Units on the top clade (what every all-hit unit gets) share one bucket: one add per wave for them.
struct LcaArgs {
    const uint2 *span;
    const uint8_t *allhit;
    const unsigned long long *off;
    const uint32_t *leaves;
    int pair_mode;
    uint64_t n_units;
    uint32_t n_leaves, n_clades, top_clade;
    const uint32_t *leaf_clade;  // [n_leaves]
    const uint32_t *gap_min;     // [levels][n_leaves]: level j, entry i = min clade of gaps [i, i + 2^j)
    uint32_t *lca;               // [n_units]
    unsigned long long *here;    // [n_clades]
};
constexpr uint32_t LCA_HIST_LDS = 8192;
template <bool LDS>
__global__ void __launch_bounds__(256) k_lca_map(LcaArgs a) {
    __shared__ uint32_t h[LDS ? LCA_HIST_LDS : 1];
    if (LDS) {
        for (uint32_t c = threadIdx.x; c < a.n_clades; c += blockDim.x) h[c] = 0;
        __syncthreads();
    }
    const uint32_t lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < a.n_units; base += stride) {  // (base is wave-uniform)
        const uint64_t u = base + threadIdx.x;
        const bool valid = u < a.n_units;
        uint32_t lo = LCA_NO_CLADE, hi = 0;
        if (valid) {
            if (a.span) {
                const uint2 s = a.span[u];
                if (a.allhit && a.allhit[u]) {
                    lo = 0;
                    hi = a.n_leaves - 1;
                } else if (!span_empty(s)) {
                    lo = s.x;
                    hi = ~s.y;
                }
            } else {
                const unsigned long long o0 = a.off[u], o1 = a.off[u + 1];
                if (o1 > o0) {
                    lo = a.leaves[o0];
                    hi = a.leaves[o1 - 1];
                } else if (a.pair_mode) {
                    const bool fa = a.allhit[2 * u] != 0, fb = a.allhit[2 * u + 1] != 0;
                    if (a.pair_mode == 2 ? (fa && fb) : (fa || fb)) {
                        lo = 0;
                        hi = a.n_leaves - 1;
                    }
                }
            }
        }
        uint32_t c = LCA_NO_CLADE;
        if (lo != LCA_NO_CLADE) {
            if (lo == hi) c = a.leaf_clade[lo];
            else {
                const uint32_t j = 31u - (uint32_t)__clz((int)(hi - lo));  // gaps lo .. hi - 1
                const uint32_t *lvl = a.gap_min + (uint64_t)j * a.n_leaves;
                c = min(lvl[lo], lvl[hi - (1u << j)]);
            }
        }
        if (valid) a.lca[u] = c;
        const bool on_top = c == a.top_clade;  // (LCA_NO_CLADE is no clade index)
        const uint64_t m_top = ballot64(on_top);
        if (m_top && lane == (uint32_t)__builtin_ctzll(m_top)) {
            if (LDS) atomicAdd(&h[c], (uint32_t)__popcll(m_top));
            else atomicAdd(&a.here[c], (unsigned long long)__popcll(m_top));
        }
        if (c != LCA_NO_CLADE && !on_top) {
            if (LDS) atomicAdd(&h[c], 1u);
            else atomicAdd(&a.here[c], 1ull);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < a.n_clades; c += blockDim.x)
            if (h[c]) atomicAdd(&a.here[c], (unsigned long long)h[c]);
    }
}

static uint32_t lca_map_blocks(uint64_t n_units, uint32_t n_clades) {
    // LDS: a block flushes up to n_clades atomics, so it takes at least 8 units per clade; global atomics: 4096 units per block
    const uint64_t per_block = n_clades <= LCA_HIST_LDS ? std::max<uint64_t>(4096, 8ull * n_clades) : 4096;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_units + per_block - 1) / per_block, 1024));
}
static void launch_lca_map(const LcaArgs &a, hipStream_t st) {
    if (!a.n_units) return;
    const uint32_t blocks = lca_map_blocks(a.n_units, a.n_clades);
    if (a.n_clades <= LCA_HIST_LDS) hipLaunchKernelGGL(k_lca_map<true>, dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_lca_map<false>, dim3(blocks), dim3(256), 0, st, a);
}

void launch_lca_pairs(const uint2 *d_pairs, uint64_t n_pairs, const uint8_t *d_allhit, uint64_t n_reads, uint2 *d_span, const LcaTables &tb,
                      uint32_t *d_lca, hipStream_t st) {
    if (!n_reads) return;
    if (n_pairs) hipLaunchKernelGGL(k_lca_span_pairs, dim3(2048), dim3(256), 0, st, d_pairs, n_pairs, d_span);
    LcaArgs a{};
    a.span = d_span;
    a.allhit = d_allhit;
    a.n_units = n_reads;
    a.n_leaves = tb.n_leaves;
    a.n_clades = tb.n_clades;
    a.top_clade = tb.top_clade;
    a.leaf_clade = tb.leaf_clade;
    a.gap_min = tb.gap_min;
    a.lca = d_lca;
    a.here = tb.here;
    launch_lca_map(a, st);
}
void launch_lca_rows(const unsigned long long *d_off, const uint32_t *d_leaves, uint64_t n_units, const uint8_t *d_allhit, int pair_mode,
                     const LcaTables &tb, uint32_t *d_lca, hipStream_t st) {
    LcaArgs a{};
    a.off = d_off;
    a.leaves = d_leaves;
    a.allhit = d_allhit;
    a.pair_mode = pair_mode;
    a.n_units = n_units;
    a.n_leaves = tb.n_leaves;
    a.n_clades = tb.n_clades;
    a.top_clade = tb.top_clade;
    a.leaf_clade = tb.leaf_clade;
    a.gap_min = tb.gap_min;
    a.lca = d_lca;
    a.here = tb.here;
    launch_lca_map(a, st);
}
void launch_lca_best(const unsigned long long *d_off, const uint32_t *d_leaves, const uint32_t *d_scores, uint64_t n_units, uint2 *d_span,
                     uint32_t *d_long, unsigned long long *d_n_long, const LcaTables &tb, uint32_t *d_lca, hipStream_t st) {
    if (!n_units) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_units + 255) / 256, 4096);
    const uint32_t wblocks = (uint32_t)std::min<uint64_t>((n_units + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 1024);
    hipLaunchKernelGGL(k_lca_best_span, dim3(blocks), dim3(256), 0, st, d_off, d_leaves, d_scores, n_units, d_span, d_long, d_n_long);
    hipLaunchKernelGGL(k_lca_best_long, dim3(wblocks), dim3(256), 0, st, d_off, d_leaves, d_scores, d_long, d_n_long, d_span);
    LcaArgs a{};
    a.span = d_span;
    a.n_units = n_units;
    a.n_leaves = tb.n_leaves;
    a.n_clades = tb.n_clades;
    a.top_clade = tb.top_clade;
    a.leaf_clade = tb.leaf_clade;
    a.gap_min = tb.gap_min;
    a.lca = d_lca;
    a.here = tb.here;
    launch_lca_map(a, st);
}

}  // namespace pfq
