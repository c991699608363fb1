// pfq_abund.hip — PFQ_WANT_ABUNDANCE: the rows of the calls' hit CSR (one per unit: a read, or a fragment with PFQ_PAIRED) are
// logged on the device, and pfq_abundance_estimate runs a fixed-point EM over the log that gives every leaf its share of the
// ambiguous rows (DESIGN.md "Abundance").  A post-stage on the CSR the call has built: no kernel of pfq_kernels.hip is involved.
//
// All state is integer (masses are u64 in units of 2^-16 units) and every sum is a sum of integers, so the result does not
// depend on launch shape, atomic order or the order in which the rows were logged.
//
// The log: row r holds entries[row_start[r] .. row_start[r] + row_len[r]), leaf columns, ascending.  Only ambiguous rows are
// kept (two or more leaves, not all of them); a row of one leaf is a count in unique[], empty rows and rows that list every
// leaf of a tree of more than one leaf are only counted.  A row's class follows from its length alone (rows are ascending and
// duplicate-free).
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

constexpr uint32_t ABUND_ROW_SHORT = 64;   // a thread takes a row of up to this many entries, a wave a longer one
constexpr uint32_t ABUND_UNIQ_LDS = 8192;  // append: unique[] counted per block in LDS (u32) up to this many leaves

// ---- count ------------------------------------------------------------------------------------------------------------
// What a CSR would add to the log, from its offsets alone: cnt[ABUND_CNT_*] += units per class and the ambiguous rows' entries.
// The host reads the five words before it appends: it makes exactly that much room, or refuses the call.
__global__ void __launch_bounds__(256) k_abund_count(const unsigned long long *__restrict__ off, uint64_t n_units, uint32_t n_leaves,
                                                     unsigned long long *cnt) {
    __shared__ unsigned long long part[ABUND_CNT_N];
    if (threadIdx.x < ABUND_CNT_N) part[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long c[ABUND_CNT_N] = {0, 0, 0, 0, 0};
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long len = off[u + 1] - off[u];
        const bool amb = len > 1 && len != n_leaves;
        c[ABUND_CNT_UNHIT] += len == 0;
        c[ABUND_CNT_UNIQUE] += len == 1;
        c[ABUND_CNT_ALL] += len > 1 && len == n_leaves;
        c[ABUND_CNT_ROWS] += amb;
        c[ABUND_CNT_ENTRIES] += amb ? len : 0;
    }
    for (uint32_t i = 0; i < ABUND_CNT_N; ++i) {
        unsigned long long v = c[i];
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
        if (lane_id() == 0 && v) atomicAdd(&part[i], v);
    }
    __syncthreads();
    if (threadIdx.x < ABUND_CNT_N && part[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], part[threadIdx.x]);
}
void launch_abund_count(const unsigned long long *d_off, uint64_t n_units, uint32_t n_leaves, unsigned long long *d_cnt, hipStream_t st) {
    if (!n_units) return;
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_units + 2047) / 2048, 1024));
    hipLaunchKernelGGL(k_abund_count, dim3(blocks), dim3(256), 0, st, d_off, n_units, n_leaves, d_cnt);
}

// ---- append -----------------------------------------------------------------------------------------------------------
// A wave reserves the rows and the entries of its ambiguous units with one atomic each (the log keeps no order: the estimate
// is a function of the multiset of rows), then every thread copies its own short row and the wave copies the long ones.
template <bool LDS>
__global__ void __launch_bounds__(256) k_abund_append(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ leaves,
                                                      uint64_t n_units, uint32_t n_leaves, AbundLog g) {
    __shared__ uint32_t h[LDS ? ABUND_UNIQ_LDS : 1];
    if (LDS) {
        for (uint32_t l = threadIdx.x; l < n_leaves; l += blockDim.x) h[l] = 0;
        __syncthreads();
    }
    const uint32_t lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n_units; base += stride) {  // (base is wave-uniform)
        const uint64_t u = base + threadIdx.x;
        unsigned long long o0 = 0, len = 0;
        if (u < n_units) {
            o0 = off[u];
            len = off[u + 1] - o0;
        }
        if (len == 1) {
            const uint32_t l = leaves[o0];
            if (l < n_leaves) {
                if (LDS) atomicAdd(&h[l], 1u);
                else atomicAdd(&g.unique[l], 1ull);
            }
        }
        const bool amb = len > 1 && len != n_leaves;
        const uint64_t m_amb = ballot64(amb);
        if (!m_amb) continue;
        unsigned long long incl = amb ? len : 0;  // inclusive scan of the ambiguous rows' lengths over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long v = __shfl_up(incl, d);
            if ((int)lane >= d) incl += v;
        }
        const unsigned long long total = __shfl(incl, 63);
        unsigned long long rbase = 0, ebase = 0;
        if (lane == 0) {
            rbase = atomicAdd(&g.cursors[0], (unsigned long long)__popcll(m_amb));
            ebase = atomicAdd(&g.cursors[1], total);
        }
        rbase = __shfl(rbase, 0);
        ebase = __shfl(ebase, 0);
        const unsigned long long r = rbase + (unsigned long long)__popcll(m_amb & ((1ull << lane) - 1ull));
        const unsigned long long e = ebase + incl - (amb ? len : 0);
        // (the host has made room for exactly what the call logs; the caps keep a wrong count from writing outside the log)
        const bool fits = amb && r < g.row_cap && e + len <= g.entry_cap;
        if (fits) {
            g.row_start[r] = e;
            g.row_len[r] = (uint32_t)len;
            if (len <= ABUND_ROW_SHORT)
                for (unsigned long long j = 0; j < len; ++j) g.entries[e + j] = leaves[o0 + j];
        }
        uint64_t m_long = ballot64(fits && len > ABUND_ROW_SHORT);
        while (m_long) {
            const int src = __builtin_ctzll(m_long);
            m_long &= m_long - 1;
            const unsigned long long so = __shfl(o0, src), se = __shfl(e, src), sl = __shfl(len, src);
            for (unsigned long long j = lane; j < sl; j += 64) g.entries[se + j] = leaves[so + j];
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t l = threadIdx.x; l < n_leaves; l += blockDim.x)
            if (h[l]) atomicAdd(&g.unique[l], (unsigned long long)h[l]);
    }
}

void launch_abund_append(const unsigned long long *d_off, const uint32_t *d_leaves, uint64_t n_units, uint32_t n_leaves, const AbundLog &g,
                         hipStream_t st) {
    if (!n_units) return;
    const bool lds = n_leaves <= ABUND_UNIQ_LDS;
    const uint64_t per_block = lds ? std::max<uint64_t>(4096, 8ull * n_leaves) : 4096;  // (a block flushes up to n_leaves atomics)
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_units + per_block - 1) / per_block, 1024));
    if (lds) hipLaunchKernelGGL(k_abund_append<true>, dim3(blocks), dim3(256), 0, st, d_off, d_leaves, n_units, n_leaves, g);
    else hipLaunchKernelGGL(k_abund_append<false>, dim3(blocks), dim3(256), 0, st, d_off, d_leaves, n_units, n_leaves, g);
}

// ---- EM ---------------------------------------------------------------------------------------------------------------
// a[l] = 1 << 16, nxt[l] = unique[l] << 16: the state before the first iteration.
__global__ void __launch_bounds__(256) k_abund_start(unsigned long long *__restrict__ a, unsigned long long *__restrict__ nxt,
                                                     const unsigned long long *__restrict__ unique, uint32_t n_leaves) {
    for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < n_leaves; l += gridDim.x * blockDim.x) {
        a[l] = 1ull << ABUND_Q;
        nxt[l] = unique[l] << ABUND_Q;
    }
}

// floor((av << 16) / D) for 0 < av <= D, av < 2^48, without a 64-bit divide.  rinv = 1.0 / (double)D.
// The true quotient q is at most 2^16 because av <= D.  (double)av is exact (48 bits), * 65536.0 is exact, the product with
// rinv and rinv itself carry a relative error of at most a few 2^-53 each, (double)D at most 2^-53: the estimate is within
// 2^16 * 2^-50 < 1 of q, so its integer part is floor(q) - 1, floor(q) or floor(q) + 1, and the two tests below, in exact
// integer arithmetic, move it to floor(q): they pick the one value t with t * D <= x < (t + 1) * D.  No product overflows:
// (t - 1) * D and t * D are only formed where they are known to be <= x < 2^64.
__device__ __forceinline__ unsigned long long abund_quot(unsigned long long av, unsigned long long D, double rinv) {
    const unsigned long long x = av << ABUND_Q;
    unsigned long long t = (unsigned long long)((double)av * 65536.0 * rinv);
    if (t && x - (t - 1) * D < D) --t;   // t was floor(q) + 1 (t - 1 <= floor(q), so (t - 1) * D <= x)
    else if (x - t * D >= D) ++t;        // t was floor(q) - 1 (here t * D <= x)
    return t;
}

// One iteration's adds: for every logged row R with D = sum of a over R > 0, nxt[l] += (a[l] << 16) / D for l in R.
//   HIST: the block adds into a u64 histogram in LDS and flushes its non-zero bins with one global atomic each;
//   else: global atomics.  ALDS: a[] is copied into LDS first (HIST only).
// LDS is dynamic: n_leaves u64 for the histogram, then n_leaves u64 for a[].
template <bool HIST, bool ALDS>
__global__ void __launch_bounds__(256) k_abund_step(AbundStep s) {
    extern __shared__ unsigned long long abund_lds[];
    unsigned long long *hist = abund_lds;
    unsigned long long *la = abund_lds + s.n_leaves;
    if (HIST) {
        for (uint32_t l = threadIdx.x; l < s.n_leaves; l += blockDim.x) {
            hist[l] = 0;
            if (ALDS) la[l] = s.a[l];
        }
        __syncthreads();
    }
    auto A = [&](uint32_t l) -> unsigned long long { return ALDS ? la[l] : s.a[l]; };
    auto add = [&](uint32_t l, unsigned long long q) {
        if (HIST) atomicAdd(&hist[l], q);
        else atomicAdd(&s.nxt[l], q);
    };
    const uint32_t lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < s.n_rows; base += stride) {  // (base is wave-uniform)
        const uint64_t r = base + threadIdx.x;
        unsigned long long e0 = 0;
        uint32_t len = 0;
        if (r < s.n_rows) {
            e0 = s.row_start[r];
            len = s.row_len[r];
        }
        if (len && len <= ABUND_ROW_SHORT) {
            unsigned long long D = 0;
            for (uint32_t j = 0; j < len; ++j) D += A(s.entries[e0 + j]);
            if (D) {
                const double rinv = 1.0 / (double)D;
                for (uint32_t j = 0; j < len; ++j) {
                    const uint32_t l = s.entries[e0 + j];
                    const unsigned long long av = A(l);
                    if (av) add(l, abund_quot(av, D, rinv));
                }
            }
        }
        uint64_t m_long = ballot64(len > ABUND_ROW_SHORT);
        while (m_long) {
            const int src = __builtin_ctzll(m_long);
            m_long &= m_long - 1;
            const unsigned long long se = __shfl(e0, src);
            const uint32_t sl = __shfl(len, src);
            unsigned long long D = 0;
            for (uint32_t j = lane; j < sl; j += 64) D += A(s.entries[se + j]);
            for (int d = 32; d > 0; d >>= 1) D += __shfl_xor(D, d);
            if (!D) continue;
            const double rinv = 1.0 / (double)D;
            for (uint32_t j = lane; j < sl; j += 64) {
                const uint32_t l = s.entries[se + j];
                const unsigned long long av = A(l);
                if (av) add(l, abund_quot(av, D, rinv));
            }
        }
    }
    if (HIST) {
        __syncthreads();
        for (uint32_t l = threadIdx.x; l < s.n_leaves; l += blockDim.x)
            if (hist[l]) atomicAdd(&s.nxt[l], hist[l]);
    }
}

// delta = max over l of |nxt[l] - a[l]|; a[] is done with and becomes the next iteration's start, unique << 16.
__global__ void __launch_bounds__(256) k_abund_delta(unsigned long long *__restrict__ a, const unsigned long long *__restrict__ nxt,
                                                     const unsigned long long *__restrict__ unique, uint32_t n_leaves,
                                                     unsigned long long *delta) {
    __shared__ unsigned long long wmax[4];
    unsigned long long d = 0;
    for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < n_leaves; l += gridDim.x * blockDim.x) {
        const unsigned long long x = a[l], y = nxt[l];
        d = max(d, x > y ? x - y : y - x);
        a[l] = unique[l] << ABUND_Q;
    }
    for (int s = 32; s > 0; s >>= 1) d = max(d, (unsigned long long)__shfl_xor(d, s));
    if (lane_id() == 0) wmax[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        d = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        if (d) atomicMax(delta, d);
    }
}

static uint32_t leaf_blocks(uint32_t n_leaves) { return std::max<uint32_t>(1, std::min<uint32_t>((n_leaves + 255) / 256, 256)); }

void launch_abund_start(unsigned long long *d_a, unsigned long long *d_nxt, const unsigned long long *d_unique, uint32_t n_leaves, hipStream_t st) {
    if (!n_leaves) return;
    hipLaunchKernelGGL(k_abund_start, dim3(leaf_blocks(n_leaves)), dim3(256), 0, st, d_a, d_nxt, d_unique, n_leaves);
}
void launch_abund_delta(unsigned long long *d_a, const unsigned long long *d_nxt, const unsigned long long *d_unique, uint32_t n_leaves,
                        unsigned long long *d_delta, hipStream_t st) {
    if (!n_leaves) return;
    hipLaunchKernelGGL(k_abund_delta, dim3(leaf_blocks(n_leaves)), dim3(256), 0, st, d_a, d_nxt, d_unique, n_leaves, d_delta);
}

// blocks = 0: the built-in grid.  lds = false: global atomics whatever the tree's size.
void launch_abund_step(const AbundStep &s, uint32_t blocks, bool lds, hipStream_t st) {
    if (!s.n_rows || !s.n_leaves) return;
    const bool hist = lds && s.n_leaves <= ABUND_HIST_LDS, a_lds = hist && s.n_leaves <= ABUND_A_LDS;
    const size_t bytes = hist ? (size_t)s.n_leaves * 8 * (a_lds ? 2 : 1) : 0;
    if (!blocks) {
        // LDS: as many blocks per CU as its 160 KiB hold, two to eight (256 CUs), and enough rows per block to be worth its
        // flush of up to n_leaves atomics.  Measured at 1024 leaves, 3.7 M rows of ~7 entries: 256 blocks 0.27 ms an iteration,
        // 458 0.18, 1024 and 2048 0.13, 4096 0.16 (DESIGN.md "Abundance").
        const uint64_t per_cu = hist ? std::max<uint64_t>(2, std::min<uint64_t>(8, (160u << 10) / std::max<size_t>(bytes, 1))) : 8;
        const uint64_t per_block = hist ? std::max<uint64_t>(2048, 2ull * s.n_leaves) : 2048;
        blocks = (uint32_t)std::min<uint64_t>((s.n_rows + per_block - 1) / per_block, 256 * per_cu);
    }
    blocks = std::max<uint32_t>(1, std::min<uint32_t>(blocks, 65535));
    if (a_lds) hipLaunchKernelGGL((k_abund_step<true, true>), dim3(blocks), dim3(256), bytes, st, s);
    else if (hist) hipLaunchKernelGGL((k_abund_step<true, false>), dim3(blocks), dim3(256), bytes, st, s);
    else hipLaunchKernelGGL((k_abund_step<false, false>), dim3(blocks), dim3(256), 0, st, s);
}

}  // namespace pfq
