// pfq_tilelist.hip — position slots of sparse filter tiles (DESIGN.md §3 "Position slots").
//
// A leaf filter has the size the root needs, so it is almost empty: a 50 kbp genome sets 0.7 % of its bits, ~7 300 of the
// 2^20 bits of a tile.  k_tile_test<0> (pfq_kernels.hip) rebuilds such a tile in LDS from the tile-relative positions of its
// set bits — a slot of TILE_LIST_CAP u32, 32 KiB — instead of loading its 128 KiB.  The slots are made here, once per device
// layout, in two launches:
//   k_tile_list_count   one block per (column, tile): the tile's set bits; col_max[column] = the largest of its tiles
//   k_tile_list_fill    one block per (listed column, tile): the positions, in the order an LDS cursor hands out places;
//                       the rest of the slot is TILE_LIST_NONE
// Between the two the host reads the n_cols maxima back (no filter data) and gives every column whose tiles all fit a row
// of slots.  The filter words are taken as they are, padding of the last word included: a slot lists exactly the bits a
// dense load of the tile would have brought.
#include "pfq_kernels.h"

namespace pfq {

constexpr uint32_t TILE_WORDS64 = 1u << (TILE_LOG2 - 6);  // 64-bit filter words per tile
constexpr uint32_t LIST_THREADS = 256;

__global__ void __launch_bounds__(LIST_THREADS) k_tile_list_count(const uint64_t *__restrict__ bits, uint64_t n_words, const uint32_t *__restrict__ col_row,
                                                                  uint32_t n_tiles, uint32_t *__restrict__ col_max) {
    __shared__ uint32_t s_sum[LIST_THREADS / 64];
    const uint32_t col = blockIdx.x / n_tiles, t = blockIdx.x % n_tiles;
    const uint64_t *row = bits + (uint64_t)col_row[col] * n_words;
    const uint64_t w0 = (uint64_t)t * TILE_WORDS64;
    uint32_t n = 0;
    for (uint32_t i = threadIdx.x; i < TILE_WORDS64 && w0 + i < n_words; i += LIST_THREADS) n += (uint32_t)__popcll(row[w0 + i]);
    for (int sft = 32; sft; sft >>= 1) n += (uint32_t)__shfl_down((int)n, sft);
    if ((threadIdx.x & 63u) == 0) s_sum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < LIST_THREADS / 64; ++w) sum += s_sum[w];
        atomicMax(&col_max[col], sum);
    }
}

__global__ void __launch_bounds__(LIST_THREADS) k_tile_list_fill(const uint64_t *__restrict__ bits, uint64_t n_words, const uint32_t *__restrict__ col_row,
                                                                 const uint32_t *__restrict__ list_cols, uint32_t n_tiles, uint32_t *__restrict__ lists) {
    __shared__ uint32_t s_cur;
    const uint32_t row_l = blockIdx.x / n_tiles, t = blockIdx.x % n_tiles;
    const uint64_t *row = bits + (uint64_t)col_row[list_cols[row_l]] * n_words;
    uint32_t *slot = lists + ((uint64_t)row_l * n_tiles + t) * TILE_LIST_CAP;
    const uint64_t w0 = (uint64_t)t * TILE_WORDS64;
    if (threadIdx.x == 0) s_cur = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < TILE_WORDS64 && w0 + i < n_words; i += LIST_THREADS) {
        uint64_t w = row[w0 + i];
        if (!w) continue;
        uint32_t at = atomicAdd(&s_cur, (uint32_t)__popcll(w));
        for (; w; w &= w - 1, ++at)
            if (at < TILE_LIST_CAP) slot[at] = i * 64u + (uint32_t)__ffsll((long long)w) - 1u;  // (the count pass saw <= cap bits: always true)
    }
    __syncthreads();
    for (uint32_t i = s_cur + threadIdx.x; i < TILE_LIST_CAP; i += LIST_THREADS) slot[i] = TILE_LIST_NONE;
}

void launch_tile_list_count(const uint64_t *bits, uint64_t n_words, const uint32_t *col_row, uint32_t n_cols, uint32_t n_tiles, uint32_t *col_max,
                            hipStream_t st) {
    hipLaunchKernelGGL(k_tile_list_count, dim3(n_cols * n_tiles), dim3(LIST_THREADS), 0, st, bits, n_words, col_row, n_tiles, col_max);
}
void launch_tile_list_fill(const uint64_t *bits, uint64_t n_words, const uint32_t *col_row, const uint32_t *list_cols, uint32_t n_list_cols, uint32_t n_tiles,
                           uint32_t *lists, hipStream_t st) {
    hipLaunchKernelGGL(k_tile_list_fill, dim3(n_list_cols * n_tiles), dim3(LIST_THREADS), 0, st, bits, n_words, col_row, list_cols, n_tiles, lists);
}

}  // namespace pfq
