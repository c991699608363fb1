// pfq_deplete.hip — pfq_prep_deplete: the units of a prepared block that hit a second tree (the screen) leave the block
// (DESIGN.md "Depletion"; the contract is the comment of pfq.h "depletion").  A post-stage on what the screen's classification
// of the block has left on the device; no kernel of pfq_kernels.hip or pfq_prep.hip is changed, and the compaction behind the
// mark is the prep's own: the two scans, k_prep_offsets and k_prep_gather again, from the raw block.
//
//   k_deplete_pairs    reads: hit[read] = 1 for every unordered (read, leaf) hit pair of the screen's call (the input of
//                      launch_lca_pairs).  Every writer of a word stores the same 1, so no atomic is needed.
//   k_deplete_mark     a thread per unit (a kept read, or a kept fragment): the verdict — reads: hit[u] or the all-hit byte;
//                      fragments: a row of the screen's final fragment CSR that is not empty, or an all-leaf fragment that the
//                      CSR leaves unlisted (both all-hit bytes with PFQ_PAIR_BOTH, either without), the rule of k_lca_map — then,
//                      through kept[], keep = klen = 0 and reason = PFQ_PREP_DEPLETED for the reads behind a removed unit, and
//                      the totals (block partial sums, one atomic per block and counter, as k_prep_mark).
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

__global__ void __launch_bounds__(256) k_deplete_pairs(const uint2 *__restrict__ pairs, uint64_t n_pairs, uint64_t n_units, uint32_t *__restrict__ hit) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pairs; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = pairs[i].x;
        if (r < n_units) hit[r] = 1u;
    }
}

__global__ void __launch_bounds__(256) k_deplete_mark(DepleteArgs a) {
    __shared__ unsigned long long s_t[4][DEPL_TOT_N];
    unsigned long long t[DEPL_TOT_N];
#pragma unroll
    for (uint32_t c = 0; c < DEPL_TOT_N; ++c) t[c] = 0;
    const uint32_t per = a.pair_mode ? 2u : 1u;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.n_units; u += (uint64_t)gridDim.x * blockDim.x) {
        bool gone;
        if (a.pair_mode) {
            const bool fa = a.allhit[2u * u] != 0, fb = a.allhit[2u * u + 1u] != 0;
            gone = (a.frag_off && a.frag_off[u + 1] > a.frag_off[u]) || (a.pair_mode == 2 ? (fa && fb) : (fa || fb));
        } else {
            gone = a.hit[u] != 0u || a.allhit[u] != 0;
        }
        if (!gone) continue;
        t[DEPL_TOT_UNITS] += 1u;
        for (uint32_t m = 0; m < per; ++m) {
            const uint32_t r = a.kept[per * u + m];
            if (r >= a.n_reads) continue;  // (kept[] holds indices of the block; never taken)
            t[DEPL_TOT_READS] += 1u;
            t[DEPL_TOT_BASES] += a.klen[r];
            a.keep[r] = 0u;
            a.klen[r] = 0u;
            a.reason[r] = PREP_DEPLETED;
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < DEPL_TOT_N; ++c) {
        unsigned long long v = t[c];
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
        if (lane_id() == 0) s_t[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < DEPL_TOT_N) {
        const unsigned long long v = s_t[0][threadIdx.x] + s_t[1][threadIdx.x] + s_t[2][threadIdx.x] + s_t[3][threadIdx.x];
        if (v) atomicAdd(a.totals + threadIdx.x, v);
    }
}

void launch_deplete_pairs(const uint2 *d_pairs, uint64_t n_pairs, uint64_t n_units, uint32_t *d_hit, hipStream_t st) {
    if (!n_pairs || !n_units) return;
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_pairs + 255) / 256, 2048));
    hipLaunchKernelGGL(k_deplete_pairs, dim3(blocks), dim3(256), 0, st, d_pairs, n_pairs, n_units, d_hit);
}
void launch_deplete_mark(const DepleteArgs &a, hipStream_t st) {
    if (!a.n_units) return;
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((a.n_units + 255) / 256, PREP_GRID));
    hipLaunchKernelGGL(k_deplete_mark, dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace pfq
