// pfq_adapt.hip — the adapter step of pfq_prep_reads: cut[r] and which[r] by the rule of pfq.h "adapters" (DESIGN.md "Adapters").
//
//   k_prep_adapter<G>   per read: the smallest position at which an adapter of the read's set matches, and the lowest such
//                       adapter.  The groups, the pieces and the three builds by length are those of k_prep_trim.
//
// Bit-parallel: a lane turns its 16 aligned bytes into a word of 2-bit codes, (u >> 1) & 3 of the upper-cased base, and a word
// that has bit 2i set where base i is none of A C G T.  The group lays both planes of the piece down in LDS, a word a lane,
// and four more words for the 64 bases behind the piece.  A lane then judges the positions it holds: the 128-bit window that
// begins at base k of its bytes is five consecutive words of a plane funnel-shifted by 2k; XOR with the adapter's codes, the
// pair bits folded to the even bits, the N plane ORed in, masked to the overlap, counted.  The adapters are kernel arguments.
#include "pfq_prep_groups.h"

namespace pfq {

// One read, by the group: rank 0 leaves cut and which and adds to the block's totals.  p_code, p_n: the group's G + 4 words each.
template <int G>
__device__ __forceinline__ void adapt_one(const AdaptArgs &a, uint64_t r, uint64_t start, uint32_t L, uint32_t *p_code, uint32_t *p_n, uint32_t *s_x,
                                          unsigned long long *s_tot) {
    using GR = Grp<G>;
    constexpr uint32_t PIECE = GR::PIECE;
    const uint32_t rk = GR::rank(), sh = (uint32_t)(start & 15u);
    const uint8_t *sbase = a.seq + (start - sh);
    const uint32_t O = a.set.min_overlap, E = a.set.max_error_percent;
    const uint32_t first = (a.paired && (r & 1u) && a.set.n[1]) ? ADAPT_MAX : 0u, n_ad = a.set.n[first ? 1 : 0];
    uint32_t cut = L, which = 0xffu;
    if (L >= O) {
        const uint64_t n_pieces = ((uint64_t)sh + (L - O) + PIECE) / PIECE;  // the pieces that hold a position p <= L - O
        for (uint64_t pc = 0; pc < n_pieces; ++pc) {
            const Chunk c = load_chunk(sbase, pc * PIECE + rk * 16u, sh, L);
            uint32_t code, nmask;
            planes_of(c, code, nmask);
            GR::ring_sync();  // (the planes of the piece before, or of the read before, have been read)
            p_code[rk] = code;
            p_n[rk] = nmask;
            if (rk < 4u) {  // the 64 bases behind the piece, if the read reaches there (uniform in the group)
                code = nmask = 0;
                if ((pc + 1u) * PIECE < (uint64_t)sh + L) planes_of(load_chunk(sbase, (pc + 1u) * PIECE + rk * 16u, sh, L), code, nmask);
                p_code[G + rk] = code;
                p_n[G + rk] = nmask;
            }
            GR::ring_sync();
            uint32_t best = NONE, best_ad = 0xffu;
            if (c.lo < c.hi) {
                uint32_t cw[5], nw[5];
#pragma unroll
                for (uint32_t i = 0; i < 5; ++i) cw[i] = p_code[rk + i], nw[i] = p_n[rk + i];
                // adapter by adapter, so that what depends on the adapter alone stays in registers over the lane's positions; a
                // later adapter can only win at a smaller position
                for (uint32_t ad = 0; ad < n_ad; ++ad) {
                    const uint32_t m = a.set.len[first + ad], full_mm = E * m / 100u;
                    uint32_t code[4], full[4];
#pragma unroll
                    for (uint32_t w = 0; w < 4; ++w) {
                        code[w] = a.set.code[first + ad][w];
                        full[w] = overlap_mask(m, w);
                    }
                    for (uint32_t k = c.lo; k < c.hi; ++k) {
                        const uint32_t p = c.pos(k), left = L - p;
                        if (left < O || p >= best) break;
                        const bool whole = left >= m;  // the whole adapter lies in the read: the masks and the bound are the adapter's
                        const uint32_t o = whole ? m : left;  // (o >= O: m >= O and left >= O)
                        uint32_t mm = 0;
#pragma unroll
                        for (uint32_t w = 0; w < 4; ++w) {
                            if (16u * w >= m) break;
                            const uint32_t x = __builtin_amdgcn_alignbit(cw[w + 1], cw[w], 2u * k) ^ code[w];
                            const uint32_t bad = x | (x >> 1) | __builtin_amdgcn_alignbit(nw[w + 1], nw[w], 2u * k);
                            mm += (uint32_t)__popc(bad & (whole ? full[w] : overlap_mask(o, w)));
                        }
                        if (whole ? mm <= full_mm : 100u * mm <= E * o) {
                            best = p;
                            best_ad = ad;
                            break;
                        }
                    }
                }
            }
            const uint32_t found = GR::gmin(best, s_x);
            if (found != NONE) {  // (uniform in the group; later pieces hold later positions)
                cut = found;
                which = GR::gmin(best == found ? best_ad : 0xffu, s_x);
                break;
            }
        }
    }
    if (rk == 0) {
        a.cut[r] = cut;
        a.which[r] = (uint8_t)which;
        if (cut < L) {
            atomicAdd(s_tot + ADAPT_TOT_FOUND, 1ull);
            atomicAdd(s_tot + ADAPT_TOT_BASES, (unsigned long long)(L - cut));
            atomicAdd(s_tot + ADAPT_TOT_WHICH + first + which, 1ull);
        }
    }
}

template <int G>
__global__ void __launch_bounds__(256) k_prep_adapter(AdaptArgs a, uint32_t len_lo, uint32_t len_hi) {
    constexpr uint32_t GROUPS = 256 / G, WORDS = G + 4;
    __shared__ uint32_t s_x[4];
    __shared__ uint32_t s_code[GROUPS * WORDS], s_n[GROUPS * WORDS];
    __shared__ unsigned long long s_tot[ADAPT_TOT_N];
    if (threadIdx.x < ADAPT_TOT_N) s_tot[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t g = G == 256 ? 0u : threadIdx.x / G;
    for_lengths<G>(a.off, a.n_reads, len_lo, len_hi, nullptr,
                   [&](uint64_t r, uint64_t start, uint32_t L) { adapt_one<G>(a, r, start, L, s_code + g * WORDS, s_n + g * WORDS, s_x, s_tot); });
    __syncthreads();
    if (threadIdx.x < ADAPT_TOT_N) {  // one atomic per block and counter
        const unsigned long long v = s_tot[threadIdx.x];
        if (v) atomicAdd(a.totals + threadIdx.x, v);
    }
}

// The three builds' length ranges are those of launch_prep_trim.
void launch_prep_adapter(const AdaptArgs &a, hipStream_t st) {
    if (!a.n_reads) return;
    const uint32_t grid = prep_grid(a.n_reads, 256);
    hipLaunchKernelGGL(k_prep_adapter<16>, dim3(grid), dim3(256), 0, st, a, 0u, PREP_SHORT_MAX);
    hipLaunchKernelGGL(k_prep_adapter<64>, dim3(grid), dim3(256), 0, st, a, PREP_SHORT_MAX + 1u, PREP_WAVE_MAX);
    hipLaunchKernelGGL(k_prep_adapter<256>, dim3(grid), dim3(256), 0, st, a, PREP_WAVE_MAX + 1u, 0xffffffffu);
}

}  // namespace pfq
