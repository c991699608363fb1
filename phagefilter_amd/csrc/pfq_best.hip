// pfq_best.hip — PFQ_ROWS_BEST: every row of the call's final CSR reduced to the entries whose score is the row's maximum
// (pfq.h "best rows", DESIGN.md §5 "Best rows").  A post-stage on the rows and the scores the call has produced, queued behind
// the score kernel: no kernel of pfq_kernels.hip is involved, and what the call hands to the caller is not touched.  The result
// is a second CSR (best_off, best_leaves) that the taxonomy, the abundance log and the coverage sketch read in place of the first.
//
// Count, scan, fill.  The rows ascend in leaf index and so do the best rows: a thread writes its kept entries in the order it
// meets them; a wave walks a long row 64 entries at a time, the ballot of the kept lanes gives every kept lane its slot (the
// kept lanes below it) and the chunks' popcounts add up to the running base.  No atomics on entries; one cursor queues the
// rows of more than BEST_ROW_SHORT entries (threshold <= 0 lists every leaf) for a wave, as k_lca_best_span does.
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

constexpr uint32_t BEST_ROW_SHORT = 64;  // entries a single thread takes (as LCA_ROW_SHORT); longer rows are queued for a wave

// cnt[u] = entries of row u at the row's maximum; rows longer than BEST_ROW_SHORT are queued and counted by k_best_count_long
__global__ void __launch_bounds__(256) k_best_count(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ scores,
                                                    uint64_t n_units, uint32_t *__restrict__ cnt, uint32_t *__restrict__ long_list,
                                                    unsigned long long *n_long) {
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long o0 = off[u], o1 = off[u + 1];
        if (o1 - o0 > BEST_ROW_SHORT) {
            long_list[atomicAdd(n_long, 1ull)] = (uint32_t)u;
            continue;
        }
        uint32_t best = 0, n = 0;
        for (unsigned long long j = o0; j < o1; ++j) {
            const uint32_t s = scores[j];
            if (s > best) {
                best = s;
                n = 0;
            }
            n += s == best;
        }
        cnt[u] = n;
    }
}
// the row's maximum over a wave: every lane returns it
__device__ __forceinline__ uint32_t best_wave_max(const uint32_t *__restrict__ scores, unsigned long long o0, unsigned long long o1, uint32_t lane) {
    uint32_t best = 0;
    for (unsigned long long j = o0 + lane; j < o1; j += 64) best = max(best, scores[j]);
    for (int d = 32; d > 0; d >>= 1) best = max(best, (uint32_t)__shfl_xor(best, d));
    return best;
}
__global__ void __launch_bounds__(256) k_best_count_long(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ scores,
                                                         const uint32_t *__restrict__ long_list, const unsigned long long *__restrict__ n_long_ptr,
                                                         uint32_t *__restrict__ cnt) {
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t n_long = *n_long_ptr;
    for (uint64_t q = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; q < n_long; q += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t u = long_list[q];
        const unsigned long long o0 = off[u], o1 = off[u + 1];
        const uint32_t best = best_wave_max(scores, o0, o1, lane);
        uint32_t n = 0;
        for (unsigned long long j = o0 + lane; j < o1; j += 64) n += scores[j] == best;
        for (int d = 32; d > 0; d >>= 1) n += (uint32_t)__shfl_xor(n, d);
        if (lane == 0) cnt[u] = n;
    }
}

// best_leaves[best_off[u] ..] = the entries of row u at the row's maximum, in the row's order
__global__ void __launch_bounds__(256) k_best_fill(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ leaves,
                                                   const uint32_t *__restrict__ scores, uint64_t n_units,
                                                   const unsigned long long *__restrict__ best_off, uint32_t *__restrict__ best_leaves) {
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long o0 = off[u], o1 = off[u + 1];
        if (o1 - o0 > BEST_ROW_SHORT) continue;  // (k_best_fill_long's)
        uint32_t best = 0;
        for (unsigned long long j = o0; j < o1; ++j) best = max(best, scores[j]);
        unsigned long long w = best_off[u];
        for (unsigned long long j = o0; j < o1; ++j)
            if (scores[j] == best) best_leaves[w++] = leaves[j];
    }
}
__global__ void __launch_bounds__(256) k_best_fill_long(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ leaves,
                                                        const uint32_t *__restrict__ scores, const uint32_t *__restrict__ long_list,
                                                        const unsigned long long *__restrict__ n_long_ptr,
                                                        const unsigned long long *__restrict__ best_off, uint32_t *__restrict__ best_leaves) {
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t n_long = *n_long_ptr;
    for (uint64_t q = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; q < n_long; q += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t u = long_list[q];
        const unsigned long long o0 = off[u], o1 = off[u + 1];
        const uint32_t best = best_wave_max(scores, o0, o1, lane);
        unsigned long long base = best_off[u];                          // wave-uniform: the slot of the chunk's first kept entry
        for (unsigned long long c = o0; c < o1; c += 64) {              // (c is wave-uniform: every lane reaches the ballot)
            const unsigned long long j = c + lane;
            const bool keep = j < o1 && scores[j] == best;
            const uint64_t m = ballot64(keep);
            if (keep) best_leaves[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = leaves[j];
            base += (uint32_t)__popcll(m);
        }
    }
}

void launch_best_rows(const unsigned long long *d_off, const uint32_t *d_leaves, const uint32_t *d_scores, uint64_t n_units, uint32_t *d_cnt,
                      unsigned long long *d_sums, uint32_t *d_long, unsigned long long *d_n_long, unsigned long long *d_best_off,
                      uint32_t *d_best_leaves, hipStream_t st) {
    if (!n_units) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_units + 255) / 256, 4096);
    const uint32_t wblocks = (uint32_t)std::min<uint64_t>((n_units + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 1024);
    hipLaunchKernelGGL(k_best_count, dim3(blocks), dim3(256), 0, st, d_off, d_scores, n_units, d_cnt, d_long, d_n_long);
    hipLaunchKernelGGL(k_best_count_long, dim3(wblocks), dim3(256), 0, st, d_off, d_scores, d_long, d_n_long, d_cnt);
    launch_scan_u32(d_cnt, n_units, d_sums, d_best_off, st);
    hipLaunchKernelGGL(k_best_fill, dim3(blocks), dim3(256), 0, st, d_off, d_leaves, d_scores, n_units, d_best_off, d_best_leaves);
    hipLaunchKernelGGL(k_best_fill_long, dim3(wblocks), dim3(256), 0, st, d_off, d_leaves, d_scores, d_long, d_n_long, d_best_off, d_best_leaves);
}

}  // namespace pfq
