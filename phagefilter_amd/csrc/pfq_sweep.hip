// pfq_sweep.hip — PFQ_WANT_SWEEP: the call's final CSR and its scores counted against a list of T thresholds at once (pfq.h
// "threshold sweep", DESIGN.md §5 "Threshold sweep").  A post-stage on the rows and the scores the call has produced, queued
// behind the score kernel like pfq_best.hip: no kernel of pfq_kernels.hip is involved, and nothing the call hands to the
// caller is touched.
//
// Per entry e = (u, l) with score s: p(e) = #{t : s >= need_kmers(thr[t], n_kmers(u))}, a prefix of the ascending list, and
// pass[p][l] += 1.  Per unit: top = max p, arg = the leaf of the first entry at it, second = the second-largest p with
// multiplicity; tops[top] += 1 and uniq[t][arg] += 1 for second <= t < top.  A thread takes a row of up to SWEEP_ROW_SHORT
// entries; longer ones (a threshold <= 0, a unit without k-mers) are queued on a cursor for a wave, as k_best_count does.
// All state is integer: the result does not depend on the order of the adds.
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

constexpr uint32_t SWEEP_ROW_SHORT = 64;  // entries a single thread takes (as BEST_ROW_SHORT); longer rows are queued for a wave
// Bins of `pass` a block counts in LDS: 32 KiB of u32 like LCA_HIST_LDS, half of what a block may declare, so that four blocks
// of a CU's 160 KiB stay resident beside each other; 1024 leaves x (5 thresholds + 1) fit.  A block's count of one bin is at
// most its rows (a row lists a leaf once), so u32 holds it.  More bins, or PFQ_SWEEP_LDS=0: global atomics.
constexpr uint32_t SWEEP_HIST_LDS = 8192;
constexpr uint32_t SWEEP_TOPS = SWEEP_MAX + 1;

// the T needs of a unit of n k-mers; the slots past T can never be reached by a u32 score
struct SweepNeeds {
    uint64_t v[SWEEP_MAX];
};
__device__ __forceinline__ SweepNeeds sweep_needs(const SweepArgs &a, uint64_t u) {
    const uint64_t len = a.read_off[u + 1] - a.read_off[u];
    const uint64_t n = len >= a.k ? len - a.k + 1 : 0;
    SweepNeeds nd;
#pragma unroll
    for (uint32_t t = 0; t < SWEEP_MAX; ++t) nd.v[t] = t < a.n_thr ? need_kmers(a.thr[t], n) : ~0ull;
    return nd;
}
__device__ __forceinline__ uint32_t sweep_passed(const SweepNeeds &nd, uint32_t s) {
    uint32_t p = 0;
#pragma unroll
    for (uint32_t t = 0; t < SWEEP_MAX; ++t) p += (uint64_t)s >= nd.v[t];
    return p;
}
template <bool LDS>
__device__ __forceinline__ void sweep_pass_add(const SweepArgs &a, uint32_t *h, uint32_t p, uint32_t l) {
    const uint32_t bin = p * a.n_leaves + l;  // (LDS: below SWEEP_HIST_LDS; else (T + 1) * L bins, below 2^32: see launch_sweep)
    if (LDS) atomicAdd(&h[bin], 1u);
    else atomicAdd(&a.pass[(uint64_t)p * a.n_leaves + l], 1ull);
}
// what a unit adds besides its entries: tops in the block's LDS bins, uniq straight to memory (at most T adds)
__device__ __forceinline__ void sweep_unit_add(const SweepArgs &a, uint32_t *tops, uint32_t top, uint32_t second, uint32_t arg) {
    atomicAdd(&tops[top], 1u);
    for (uint32_t t = second; t < top; ++t) atomicAdd(&a.uniq[(uint64_t)t * a.n_leaves + arg], 1ull);
}
template <bool LDS>
__device__ __forceinline__ void sweep_lds_clear(const SweepArgs &a, uint32_t *h, uint32_t *tops) {
    if (LDS)
        for (uint32_t b = threadIdx.x; b < (a.n_thr + 1) * a.n_leaves; b += blockDim.x) h[b] = 0;
    if (threadIdx.x < SWEEP_TOPS) tops[threadIdx.x] = 0;
    __syncthreads();
}
template <bool LDS>
__device__ __forceinline__ void sweep_lds_flush(const SweepArgs &a, const uint32_t *h, const uint32_t *tops) {
    __syncthreads();
    if (LDS)
        for (uint32_t b = threadIdx.x; b < (a.n_thr + 1) * a.n_leaves; b += blockDim.x)
            if (h[b]) atomicAdd(&a.pass[b], (unsigned long long)h[b]);
    if (threadIdx.x <= a.n_thr && tops[threadIdx.x]) atomicAdd(&a.tops[threadIdx.x], (unsigned long long)tops[threadIdx.x]);
}

// rows of up to SWEEP_ROW_SHORT entries: a thread each; longer ones go to long_list
template <bool LDS>
__global__ void __launch_bounds__(256) k_sweep_rows(SweepArgs a) {
    __shared__ uint32_t h[LDS ? SWEEP_HIST_LDS : 1];
    __shared__ uint32_t tops[SWEEP_TOPS];
    sweep_lds_clear<LDS>(a, h, tops);
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.n_units; u += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long o0 = a.off[u], o1 = a.off[u + 1];
        if (o1 - o0 > SWEEP_ROW_SHORT) {
            a.long_list[atomicAdd(a.n_long, 1ull)] = (uint32_t)u;
            continue;
        }
        const SweepNeeds nd = sweep_needs(a, u);
        uint32_t top = 0, second = 0, arg = 0;
        for (unsigned long long j = o0; j < o1; ++j) {
            const uint32_t l = a.leaves[j], p = sweep_passed(nd, a.scores[j]);
            sweep_pass_add<LDS>(a, h, p, l);
            if (p > top) {
                second = top;
                top = p;
                arg = l;
            } else {
                second = max(second, p);
            }
        }
        sweep_unit_add(a, tops, top, second, arg);
    }
    sweep_lds_flush<LDS>(a, h, tops);
}

// the queued rows: a wave each, lanes stride the row.  A lane's (top, first index at it, second) combine across the wave: on
// equal top the lower index wins, and the second of a union is the largest of the lower top and both seconds.  A lane without
// entries holds (0, none, 0), which changes nothing.
template <bool LDS>
__global__ void __launch_bounds__(256) k_sweep_long(SweepArgs a) {
    __shared__ uint32_t h[LDS ? SWEEP_HIST_LDS : 1];
    __shared__ uint32_t tops[SWEEP_TOPS];
    sweep_lds_clear<LDS>(a, h, tops);
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t n_long = *a.n_long;
    for (uint64_t q = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; q < n_long; q += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t u = a.long_list[q];
        const unsigned long long o0 = a.off[u], o1 = a.off[u + 1];
        const SweepNeeds nd = sweep_needs(a, u);
        uint32_t top = 0, second = 0, idx = 0xffffffffu;  // idx: the entry's place in the row (a row holds at most n_leaves entries)
        for (unsigned long long j = o0 + lane; j < o1; j += 64) {
            const uint32_t p = sweep_passed(nd, a.scores[j]);
            sweep_pass_add<LDS>(a, h, p, a.leaves[j]);
            if (p > top) {
                second = top;
                top = p;
                idx = (uint32_t)(j - o0);
            } else {
                second = max(second, p);
            }
        }
        for (int d = 32; d > 0; d >>= 1) {
            const uint32_t top2 = (uint32_t)__shfl_xor(top, d), second2 = (uint32_t)__shfl_xor(second, d), idx2 = (uint32_t)__shfl_xor(idx, d);
            second = max(min(top, top2), max(second, second2));
            if (top2 > top || (top2 == top && idx2 < idx)) idx = idx2;
            top = max(top, top2);
        }
        if (lane == 0) sweep_unit_add(a, tops, top, second, top ? a.leaves[o0 + idx] : 0u);
    }
    sweep_lds_flush<LDS>(a, h, tops);
}

void launch_sweep(const SweepArgs &a, bool lds, hipStream_t st) {
    if (!a.n_units) return;
    const uint64_t bins = (uint64_t)(a.n_thr + 1) * a.n_leaves;
    lds = lds && bins <= SWEEP_HIST_LDS;
    // LDS: a block flushes up to `bins` atomics, so it takes at least 8 units per bin (as lca_map_blocks); else 256 units per block
    const uint64_t per_block = lds ? std::max<uint64_t>(256, 8 * bins) : 256;
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((a.n_units + per_block - 1) / per_block, SWEEP_GRID_ROWS));
    const uint64_t per_wblock = lds ? std::max<uint64_t>(WAVES_PER_BLOCK, bins / 8) : WAVES_PER_BLOCK;
    const uint32_t wblocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((a.n_units + per_wblock - 1) / per_wblock, SWEEP_GRID_LONG));
    if (lds) {
        hipLaunchKernelGGL(k_sweep_rows<true>, dim3(blocks), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_sweep_long<true>, dim3(wblocks), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(k_sweep_rows<false>, dim3(blocks), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_sweep_long<false>, dim3(wblocks), dim3(256), 0, st, a);
    }
}

}  // namespace pfq
