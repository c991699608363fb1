// pfq_sim.hip — pfq_tree_similarity: shared set bits of every pair of listed filters (DESIGN.md "Similarity").
//
//   out[i * n_b + j] = popcount(bits_a[rows_a[i]] & bits_b[rows_b[j]])     over bit indices < nbits
//
// An all-pairs popcount of ANDs is a GEMM over bits: M = n_a, N = n_b, K = nbits, with (and, popcount-accumulate) in the place
// of (multiply, add).  k_sim_tile is tiled like one: a block of 256 threads owns SIM_TILE x SIM_TILE pairs, a thread an 8 x 8
// block of u32 counters in registers, and the block walks its slice of K in chunks of SIM_CHUNK 64-bit words that it stages
// into LDS — word-major, so that the four A and four B operands a thread needs for one 32-bit word are 16-byte reads — while
// the loads of the next chunk are in flight.  K is also cut into gridDim.y slices (few tiles would leave most of the chip
// idle); a slice adds its partial counts to `out` with one u32 atomic add per pair.  Integer adds commute: the result is
// exact whatever the slice count and the arrival order.  The caller zeroes `out`.
//
// k_sim_pair is the plain form, one block per pair, every filter read from memory once per pair: the A/B baseline and the
// second implementation the tests compare with (PFQ_SIM_NAIVE=1).  With `diag` it gives the set bits of every listed filter.
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

constexpr uint32_t SIM_TILE = 128;           // rows of A and of B per block
constexpr uint32_t SIM_CHUNK = 16;           // 64-bit words of every row per stage: one 128-byte line
constexpr uint32_t SIM_CHUNK32 = 2 * SIM_CHUNK;
constexpr uint32_t SIM_PIECES = SIM_CHUNK / 2;                        // 16-byte pieces of a row's chunk
constexpr uint32_t SIM_LOADS = 2 * SIM_TILE * SIM_PIECES / 256;       // pieces a thread stages per chunk
static_assert(SIM_PIECES == 8 && SIM_LOADS == 8, "k_sim_tile's staging indices are written for 8 pieces and 8 loads");

// two 64-bit words that are only 8-byte aligned (a row starts at row * n_words words)
struct __attribute__((aligned(8))) SimPiece {
    uint64_t lo, hi;
};

// Words [w, w + 2) of one row with everything at or beyond nbits cleared: words past the end read as 0 and the last word is
// masked (a filter that was loaded from a file may carry anything in its padding).
__device__ __forceinline__ SimPiece sim_load_piece(const uint64_t *__restrict__ row, uint64_t w, uint64_t n_words, uint64_t tail_mask) {
    SimPiece p{0, 0};
    if (w + 1 < n_words) {
        p = *reinterpret_cast<const SimPiece *>(row + w);
        if (w + 2 == n_words) p.hi &= tail_mask;
    } else if (w < n_words) {
        p.lo = row[w] & tail_mask;
    }
    return p;
}

// LDS image of a chunk: s[word32][column], columns 0..127 the tile's A rows, 128..255 its B rows.  A thread stages 16-byte
// pieces of rows (lanes 8q..8q+7 of a wave: the eight pieces of one row's line) and stores each piece's four 32-bit words into
// four word rows: with a plain column index the 8 pieces x 4 rows of a half-wave would meet on 4 banks, 8 deep.  The column is
// therefore XORed with 8 * piece: the half-wave's stores spread over all 32 banks two deep, which a 4-byte store does not pay
// for.  The XOR moves whole groups of 8 columns, so the readers' 16-byte groups of four columns stay contiguous and aligned, and
// the 16 groups that the lanes of a 16-byte read name still fill one 256-byte bank row: no conflict on the read side.
__device__ __forceinline__ uint32_t sim_col(uint32_t col, uint32_t piece) { return col ^ (piece << 3); }

__global__ void __launch_bounds__(256, 2)
k_sim_tile(const uint64_t *__restrict__ bits_a, const uint32_t *__restrict__ rows_a, uint32_t n_a, const uint64_t *__restrict__ bits_b,
           const uint32_t *__restrict__ rows_b, uint32_t n_b, uint64_t n_words, uint64_t tail_mask, uint32_t tiles_b, uint32_t *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t s[2][SIM_CHUNK32][2 * SIM_TILE];  // 64 KiB: two blocks per CU
    const uint32_t t = threadIdx.x, tx = t & 15u, ty = t >> 4;
    const uint32_t a0 = (blockIdx.x / tiles_b) * SIM_TILE, b0 = (blockIdx.x % tiles_b) * SIM_TILE;
    // this block's chunks of K
    const uint64_t n_chunks = (n_words + SIM_CHUNK - 1) / SIM_CHUNK;
    const uint64_t c_begin = n_chunks * blockIdx.y / gridDim.y, c_end = n_chunks * (blockIdx.y + 1) / gridDim.y;
    if (c_begin >= c_end) return;  // (block-uniform)

    // what this thread stages: piece `piece` of columns col0 + 32 j, j < 8 (columns < 128: A rows, else B rows)
    const uint32_t piece = t & 7u, col0 = t >> 3;
    const uint64_t *src[SIM_LOADS];
#pragma unroll
    for (uint32_t j = 0; j < SIM_LOADS; ++j) {
        const uint32_t col = col0 + 32u * j;
        const bool is_a = col < SIM_TILE;
        const uint32_t r = is_a ? a0 + col : b0 + (col - SIM_TILE);
        const bool has = r < (is_a ? n_a : n_b);
        src[j] = has ? (is_a ? bits_a + (uint64_t)rows_a[r] * n_words : bits_b + (uint64_t)rows_b[r] * n_words) : nullptr;
    }
    SimPiece st[SIM_LOADS];
    auto fetch = [&](uint64_t c) {
        const uint64_t w = c * SIM_CHUNK + 2u * piece;
#pragma unroll
        for (uint32_t j = 0; j < SIM_LOADS; ++j) st[j] = src[j] ? sim_load_piece(src[j], w, n_words, tail_mask) : SimPiece{0, 0};
    };
    auto stage = [&](uint32_t buf) {
#pragma unroll
        for (uint32_t j = 0; j < SIM_LOADS; ++j) {
            const uint32_t col = col0 + 32u * j;
            const uint32_t at = (col & SIM_TILE) | sim_col(col & (SIM_TILE - 1u), piece);
            s[buf][4u * piece + 0u][at] = (uint32_t)st[j].lo;
            s[buf][4u * piece + 1u][at] = (uint32_t)(st[j].lo >> 32);
            s[buf][4u * piece + 2u][at] = (uint32_t)st[j].hi;
            s[buf][4u * piece + 3u][at] = (uint32_t)(st[j].hi >> 32);
        }
    };

    uint32_t acc[8][8];
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i)
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) acc[i][j] = 0;

    fetch(c_begin);
    stage(0);
    __syncthreads();
    uint32_t buf = 0;
    for (uint64_t c = c_begin; c < c_end; ++c, buf ^= 1u) {
        const bool more = c + 1 < c_end;
        if (more) fetch(c + 1);  // in flight during this chunk's arithmetic
#pragma unroll 1
        for (uint32_t q = 0; q < SIM_PIECES; ++q) {
            // a thread's pairs: A rows 4 ty + {0..3} and 64 + 4 ty + {0..3}, B rows 4 tx + {0..3} and 64 + 4 tx + {0..3}
            const uint32_t ca = sim_col(4u * ty, q), cb = SIM_TILE + sim_col(4u * tx, q);
#pragma unroll 1  // (unrolled twice the operands of two words are live at once: 256 VGPRs and scratch; the block's other waves cover the reads)
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t *row = s[buf][4u * q + k];
                const uint4 al = *reinterpret_cast<const uint4 *>(row + ca), ah = *reinterpret_cast<const uint4 *>(row + ca + 64u);
                const uint4 bl = *reinterpret_cast<const uint4 *>(row + cb), bh = *reinterpret_cast<const uint4 *>(row + cb + 64u);
                const uint32_t a[8] = {al.x, al.y, al.z, al.w, ah.x, ah.y, ah.z, ah.w};
                const uint32_t b[8] = {bl.x, bl.y, bl.z, bl.w, bh.x, bh.y, bh.z, bh.w};
#pragma unroll
                for (uint32_t i = 0; i < 8; ++i)
#pragma unroll
                    for (uint32_t j = 0; j < 8; ++j) acc[i][j] += (uint32_t)__popc(a[i] & b[j]);
            }
        }
        if (more) stage(buf ^ 1u);  // (its last readers passed the barrier that ended the previous chunk)
        __syncthreads();
    }

#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t ra = a0 + (i < 4 ? 4u * ty + i : 64u + 4u * ty + (i - 4u));
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t rb = b0 + (j < 4 ? 4u * tx + j : 64u + 4u * tx + (j - 4u));
            if (ra < n_a && rb < n_b && acc[i][j]) atomicAdd(&out[(uint64_t)ra * n_b + rb], acc[i][j]);
        }
    }
}

// One block per pair p = i * n_b + j (DIAG: per row i of the A list, against itself: its set bits).
template <bool DIAG, typename Out>
__global__ void __launch_bounds__(256) k_sim_pair(const uint64_t *__restrict__ bits_a, const uint32_t *__restrict__ rows_a,
                                                  const uint64_t *__restrict__ bits_b, const uint32_t *__restrict__ rows_b, uint32_t n_b,
                                                  uint64_t n_words, uint64_t tail_mask, Out *__restrict__ out) {
    __shared__ unsigned long long s_w[4];
    const uint32_t i = DIAG ? blockIdx.x : blockIdx.x / n_b, j = DIAG ? 0u : blockIdx.x % n_b;
    const uint64_t *a = bits_a + (uint64_t)rows_a[i] * n_words;
    const uint64_t *b = DIAG ? a : bits_b + (uint64_t)rows_b[j] * n_words;
    unsigned long long c = 0;
    for (uint64_t w = threadIdx.x; w < n_words; w += blockDim.x) {
        const uint64_t x = a[w] & b[w];
        c += (unsigned long long)__popcll(w + 1 == n_words ? x & tail_mask : x);
    }
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if (lane_id() == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (Out)(s_w[0] + s_w[1] + s_w[2] + s_w[3]);
}

static uint64_t sim_tail_mask(uint64_t nbits) { return (nbits & 63u) ? (1ull << (nbits & 63u)) - 1ull : ~0ull; }

uint32_t launch_filter_intersections(const uint64_t *bits_a, const uint32_t *d_rows_a, uint32_t n_a, const uint64_t *bits_b, const uint32_t *d_rows_b,
                                     uint32_t n_b, uint64_t n_words, uint64_t nbits, uint32_t slices, bool naive, uint32_t *d_out, hipStream_t st) {
    if (!n_a || !n_b || !n_words) return 0;
    const uint64_t tail = sim_tail_mask(nbits);
    if (naive) {
        hipLaunchKernelGGL((k_sim_pair<false, uint32_t>), dim3(n_a * n_b), dim3(256), 0, st, bits_a, d_rows_a, bits_b, d_rows_b, n_b, n_words, tail, d_out);
        return 1;
    }
    const uint32_t tiles_a = (n_a + SIM_TILE - 1) / SIM_TILE, tiles_b = (n_b + SIM_TILE - 1) / SIM_TILE;
    const uint64_t tiles = (uint64_t)tiles_a * tiles_b, n_chunks = (n_words + SIM_CHUNK - 1) / SIM_CHUNK;
    // built-in: about 4096 blocks, eight rounds of the 512 that are resident: short blocks even out the tail (the sweep of
    // PFQ_SIM_SLICES in profiles/sim_bench.txt); never more slices than chunks
    uint64_t s = slices ? slices : (4096 + tiles - 1) / tiles;
    s = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(s, n_chunks), 65535));
    hipLaunchKernelGGL(k_sim_tile, dim3((uint32_t)tiles, (uint32_t)s), dim3(256), 0, st, bits_a, d_rows_a, n_a, bits_b, d_rows_b, n_b, n_words, tail,
                       tiles_b, d_out);
    return (uint32_t)s;
}

void launch_filter_row_bits(const uint64_t *bits, const uint32_t *d_rows, uint32_t n_rows, uint64_t n_words, uint64_t nbits, unsigned long long *d_out,
                            hipStream_t st) {
    if (!n_rows) return;
    hipLaunchKernelGGL((k_sim_pair<true, unsigned long long>), dim3(n_rows), dim3(256), 0, st, bits, d_rows, bits, d_rows, 1u, n_words, sim_tail_mask(nbits),
                       d_out);
}

}  // namespace pfq
