// pfq_prep_groups.h — what the per-read kernels of pfq_prep_reads share (pfq_prep.hip, pfq_adapt.hip, pfq_overlap.hip): a group of G lanes that
// takes a read in pieces of 16 G bytes, 16 aligned bytes a lane, and the loop that hands the reads of a length range to groups.
#pragma once
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

constexpr uint32_t NONE = 0xffffffffu;

__device__ __forceinline__ uint32_t up(uint32_t c) { return c & 0xDFu; }
__device__ __forceinline__ bool is_n(uint32_t u) { return !(u == 'A' || u == 'C' || u == 'G' || u == 'T'); }

// A group of G lanes: 16 or 64 (part of a wave: shuffles of width G) or 256 (the block: wave shuffles, four words of LDS and
// two barriers; every thread of the block must then arrive).
template <int G>
struct Grp {
    static constexpr uint32_t PIECE = G * 16u;
    __device__ static __forceinline__ uint32_t rank() { return G == 256 ? threadIdx.x : (threadIdx.x & (uint32_t)(G - 1)); }
    template <typename Op>
    __device__ static __forceinline__ uint32_t reduce(uint32_t v, uint32_t *s_x, Op op) {
        constexpr int W = G < 64 ? G : 64;
#pragma unroll
        for (int d = W / 2; d > 0; d >>= 1) v = op(v, (uint32_t)__shfl_xor((int)v, d, W));
        if (G == 256) {
            if (lane_id() == 0) s_x[threadIdx.x >> 6] = v;
            __syncthreads();
            v = op(op(s_x[0], s_x[1]), op(s_x[2], s_x[3]));
            __syncthreads();
        }
        return v;
    }
    __device__ static __forceinline__ uint32_t gmin(uint32_t v, uint32_t *s_x) { return reduce(v, s_x, [](uint32_t a, uint32_t b) { return a < b ? a : b; }); }
    __device__ static __forceinline__ uint32_t gmax(uint32_t v, uint32_t *s_x) { return reduce(v, s_x, [](uint32_t a, uint32_t b) { return a > b ? a : b; }); }
    __device__ static __forceinline__ uint32_t gsum(uint32_t v, uint32_t *s_x) { return reduce(v, s_x, [](uint32_t a, uint32_t b) { return a + b; }); }
    // inclusive scan over the group's lanes; total = the group's sum
    __device__ static __forceinline__ uint32_t scan(uint32_t v, uint32_t &total, uint32_t *s_x) {
        constexpr int W = G < 64 ? G : 64;
        const uint32_t l = threadIdx.x & (uint32_t)(W - 1);
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < W; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d, W);
            if ((int)l >= d) incl += o;
        }
        total = (uint32_t)__shfl((int)incl, W - 1, W);
        if (G == 256) {
            const uint32_t wave = threadIdx.x >> 6;
            if (lane_id() == 63) s_x[wave] = incl;
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (uint32_t w = 0; w < 4; ++w) {
                if (w < wave) before += s_x[w];
                all += s_x[w];
            }
            __syncthreads();
            incl += before;
            total = all;
        }
        return incl;
    }
    // between the group's stores to its ring and its loads from it (and back): the lanes of a wave run in step and LDS serves
    // a wave in order, so inside a wave only the compiler has to keep the order
    __device__ static __forceinline__ void ring_sync() {
        if (G == 256) {
            __syncthreads();
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
};

// The 16 aligned bytes at abase + x that belong to this lane (zero beyond the span: nothing is loaded there), and which of them
// are bases of the read: byte k is base jb + k for lo <= k < hi.  abase is 16-byte aligned, sh = the read's first byte in it.
struct Chunk {
    uint32_t w[4];
    uint32_t lo, hi;
    int64_t jb;
    __device__ __forceinline__ uint32_t byte(uint32_t k) const { return (w[k >> 2] >> (8u * (k & 3u))) & 0xffu; }
    __device__ __forceinline__ uint32_t pos(uint32_t k) const { return (uint32_t)(jb + (int64_t)k); }
};
__device__ __forceinline__ Chunk load_chunk(const uint8_t *__restrict__ abase, uint64_t x, uint32_t sh, uint32_t L) {
    Chunk c;
    c.jb = (int64_t)x - (int64_t)sh;
    const int64_t left = (int64_t)L - c.jb;  // bases at or behind byte 0
    c.lo = c.jb < 0 ? (uint32_t)(-c.jb) : 0u;
    c.hi = left <= 0 ? 0u : left >= 16 ? 16u : (uint32_t)left;
    if (c.lo >= c.hi) {
        c.lo = c.hi = 0;
        c.w[0] = c.w[1] = c.w[2] = c.w[3] = 0;
    } else {
        const uint4 v = *reinterpret_cast<const uint4 *>(abase + x);
        c.w[0] = v.x, c.w[1] = v.y, c.w[2] = v.z, c.w[3] = v.w;
    }
    return c;
}

// The 2-bit planes of a lane's 16 bytes (pfq_adapt.hip, pfq_overlap.hip): code has (u >> 1) & 3 of the upper-cased byte k at bits
// 2k, 2k + 1; nmask has bit 2k set where byte k is none of A C G T.
__device__ __forceinline__ void planes_of(const Chunk &c, uint32_t &code, uint32_t &nmask) {
    code = nmask = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {  // four bases a step: bits 1, 2 of every byte, then the four pairs brought together
        uint32_t t = (c.w[i] >> 1) & 0x03030303u;
        t |= t >> 6;
        code |= ((t & 0xfu) | ((t >> 12) & 0xf0u)) << (8u * i);
    }
    // not A C G T: v = up(c) ^ 'A' is 0, 2, 6 or 21 for the four letters; a byte of x is v's low five bits, and 32 more if
    // v has bit 6 or 7 (bit 5 never: up() cleared it), so a table of 32 bits and x >> 5 decide
    constexpr uint32_t NOT_LETTER = ~((1u << 0) | (1u << 2) | (1u << 6) | (1u << 21));
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t v = (c.w[i] & 0xDFDFDFDFu) ^ 0x41414141u;
        const uint32_t x = (v & 0x1F1F1F1Fu) | ((((v | (v >> 1)) & 0x40404040u)) >> 1);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t idx = (x >> (8u * j)) & 0x3fu;
            nmask |= (((NOT_LETTER >> (idx & 31u)) | (idx >> 5)) & 1u) << (2u * (4u * i + j));
        }
    }
}

// The even bits of word w (bases 16 w .. 16 w + 15) that lie inside an overlap of o bases.
__device__ __forceinline__ uint32_t overlap_mask(uint32_t o, uint32_t w) {
    const uint32_t cnt = o > 16u * w ? min(o - 16u * w, 16u) : 0u;
    return cnt >= 16u ? 0x55555555u : (0x55555555u & ((1u << (2u * cnt)) - 1u));
}

// f(i, off[i], length) by a whole group for every i < n whose length off[i + 1] - off[i] is in [lo, hi].  A block looks at
// blockDim.x entries a trip, a thread each; the groups of a wave share the wave's 64 (G = 256: the block's 256).  Lengths of
// 2^32 or more (or offsets that descend) belong to nobody; the build with lo == 0 reports them in *err.
template <int G, typename F>
__device__ __forceinline__ void for_lengths(const uint64_t *__restrict__ off, uint64_t n, uint32_t lo, uint32_t hi, unsigned long long *err, F f) {
    __shared__ uint64_t s_mask[4];
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {  // (uniform in the block)
        const uint64_t i = base + threadIdx.x;
        bool mine = false;
        if (i < n) {
            const uint64_t len = off[i + 1] - off[i];
            if (len >> 32) {
                if (lo == 0 && err) atomicOr(err, 1ull);
            } else {
                mine = (uint32_t)len >= lo && (uint32_t)len <= hi;
            }
        }
        uint64_t mask = ballot64(mine);
        if (G == 256) {
            if (lane_id() == 0) s_mask[threadIdx.x >> 6] = mask;
            __syncthreads();
            for (uint32_t w = 0; w < 4; ++w) {
                uint64_t m = s_mask[w];
                while (m) {
                    const uint64_t j = base + w * 64u + (uint32_t)(__ffsll((unsigned long long)m) - 1);
                    m &= m - 1;
                    f(j, off[j], (uint32_t)(off[j + 1] - off[j]));
                }
            }
            __syncthreads();
        } else {
            const uint64_t wave_base = base + (threadIdx.x & ~63u);
            for (uint32_t bit = lane_id() / G; bit < 64u; bit += 64u / G) {
                if (!((mask >> bit) & 1ull)) continue;
                const uint64_t j = wave_base + bit;
                f(j, off[j], (uint32_t)(off[j + 1] - off[j]));
            }
        }
    }
}

inline uint32_t prep_grid(uint64_t n, uint32_t per_block) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(PREP_GRID, (n + per_block - 1) / per_block)); }

}  // namespace pfq
