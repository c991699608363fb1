// pfq_prep.hip — pfq_prep_reads: reads trimmed and filtered on the device before classification (DESIGN.md "Read
// preprocessing"; the contract is the comment of pfq.h "read preprocessing").  Nothing of pfq_kernels.hip is involved beyond
// the scan behind launch_scan_u32.
//
//   k_prep_trim<G>     per read (begin, len, reason): a GROUP of G lanes takes a read in pieces of 16 G bytes, 16 aligned bytes a
//                      lane, the running sum and the running answers carried from piece to piece.  Three builds share the
//                      reads by length: G = 16 (four reads a wave), G = 64 (a wave a read), G = 256 (a block a read).
//   k_prep_mark        the mate rule, keep flags and kept lengths, the totals (block partial sums, one atomic per block and counter)
//   scan x 2           the kept reads' ranks and the kept bases' offsets
//   k_prep_offsets     kept[] and the CSR offsets
//   k_prep_gather<G>   the kept intervals moved to their places: 16-byte stores to the aligned body of a read
//
// Every step of the contract is a scan or a min / max reduction over positions:
//   quality   one forward pass: p's prefix sums (lane-local, then a group scan, then the carry), the first good base (min), the
//             first bad window (min).  A window is judged by the lane that holds its LAST base: S(last) - S(first - 1), the
//             second read from a ring of prefix sums in LDS that reaches W + 1 positions behind the piece.  Then a backward
//             pass for the last good base before the cut (max; it ends in the first piece it looks at unless that is all bad).
//   poly-X    a backward pass from the cut: the last position that differs from up(s[e - 1]) (max).
//   N, complexity   a forward pass over [b, e): two sums.
// The later passes look again at bytes the quality pass has just read and take the L2 hit (see DESIGN: a 150-base read is one
// piece of one group, so what is re-read is a line or two that another lane of the same wave loaded microseconds ago; keeping
// the pieces in LDS would cost 16 bytes a lane of LDS per buffer for every length, to save those hits).
// Grp<G>, load_chunk and for_lengths are in pfq_prep_groups.h, shared with the adapter step (pfq_adapt.hip), which runs first
// when adapters are set and leaves cut[]: the read is then s[0, cut).
#include "pfq_prep_groups.h"

namespace pfq {

// One read, by the group: rank 0 leaves (begin, len, reason before the mate rule).  ring: the group's ring_mask + 1 words of LDS.
template <int G>
__device__ __forceinline__ void prep_one(const PrepArgs &a, uint64_t r, uint64_t start, uint32_t L, uint32_t *ring, uint32_t ring_mask, uint32_t *s_x) {
    using GR = Grp<G>;
    constexpr uint32_t PIECE = GR::PIECE;
    const uint32_t rk = GR::rank(), sh = (uint32_t)(start & 15u);
    const uint8_t *sbase = a.seq + (start - sh);
    const uint32_t Q = a.trim_quality, W = a.trim_window;
    uint32_t b = 0, e = L;
    bool empty = L == 0;
    if (L && Q && a.qual && (!a.has_qual || a.has_qual[r])) {
        const uint8_t *qbase = a.qual + (start - sh);
        const uint64_t n_pieces = ((uint64_t)sh + L + PIECE - 1) / PIECE;
        uint32_t carry = 0, bfound = NONE, s_before_b = 0, ebad = NONE;
        for (uint64_t pc = 0; pc < n_pieces; ++pc) {
            const uint64_t x = pc * PIECE + rk * 16u;
            const Chunk c = load_chunk(qbase, x, sh, L);
            uint32_t pre[16], loc = 0, first_good = NONE, before_good = 0;
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const uint32_t q = c.byte(k), p = (k >= c.lo && k < c.hi && q > 33u) ? q - 33u : 0u;
                if (k >= c.lo && k < c.hi && p >= Q && first_good == NONE) {
                    first_good = c.pos(k);
                    before_good = loc;
                }
                loc += p;
                pre[k] = loc;
            }
            uint32_t total;
            const uint32_t excl = carry + GR::scan(loc, total, s_x) - loc;  // the sum of p before this lane's bytes
            if (bfound == NONE) {
                const uint32_t m = GR::gmin(first_good, s_x);
                if (m != NONE) {
                    bfound = m;
                    s_before_b = GR::gsum(first_good == m ? excl + before_good : 0u, s_x);
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) ring[(uint32_t)(x + k) & ring_mask] = excl + pre[k];  // the sum up to and including this byte
            GR::ring_sync();
            if (bfound != NONE && L - bfound >= W) {  // (uniform in the group)
                uint32_t bad = NONE;
#pragma unroll
                for (uint32_t k = 0; k < 16; ++k) {
                    if (k < c.lo || k >= c.hi) continue;
                    const uint32_t j = c.pos(k);  // the window's last base
                    if (j + 1u < W) continue;
                    const uint32_t i = j + 1u - W;
                    if (i < bfound) continue;
                    const uint32_t before = i ? ring[(uint32_t)(x + k - W) & ring_mask] : 0u;
                    if (excl + pre[k] - before < Q * W) bad = min(bad, i);
                }
                const uint32_t m = GR::gmin(bad, s_x);
                if (m != NONE) {
                    ebad = m;
                    break;
                }
            }
            carry += total;
            GR::ring_sync();
        }
        if (bfound == NONE) {
            empty = true;
        } else {
            b = bfound;
            if (L - b < W) e = (carry - s_before_b < Q * (L - b)) ? b : L;  // one window of what is left (no break above: carry is the read's sum)
            else e = ebad != NONE ? ebad : L;
            if (e > b) {  // the last good base of [b, e): b itself is one
                const uint64_t pc_lo = ((uint64_t)sh + b) / PIECE;
                for (uint64_t pc = ((uint64_t)sh + e - 1u) / PIECE;; --pc) {
                    const Chunk c = load_chunk(qbase, pc * PIECE + rk * 16u, sh, L);
                    uint32_t last = 0;
#pragma unroll
                    for (uint32_t k = 0; k < 16; ++k) {
                        const uint32_t q = c.byte(k), j = c.pos(k);
                        if (k >= c.lo && k < c.hi && j >= b && j < e && q >= 33u + Q) last = j + 1u;
                    }
                    const uint32_t m = GR::gmax(last, s_x);
                    if (m) {
                        e = m;
                        break;
                    }
                    if (pc == pc_lo) break;
                }
            } else {
                empty = true;
            }
        }
    }
    if (a.poly_x && !empty && e > b) {
        const uint32_t cx = up(a.seq[start + e - 1u]);
        const uint64_t pc_lo = ((uint64_t)sh + b) / PIECE;
        uint32_t run = e - b;
        for (uint64_t pc = ((uint64_t)sh + e - 1u) / PIECE;; --pc) {
            const Chunk c = load_chunk(sbase, pc * PIECE + rk * 16u, sh, L);
            uint32_t last = 0;
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const uint32_t j = c.pos(k);
                if (k >= c.lo && k < c.hi && j >= b && j < e && up(c.byte(k)) != cx) last = j + 1u;
            }
            const uint32_t m = GR::gmax(last, s_x);
            if (m) {
                run = e - m;
                break;
            }
            if (pc == pc_lo) break;
        }
        if (run >= a.poly_x) e -= run;
    }
    uint32_t len = (empty || e <= b) ? 0u : e - b;
    if (!len) b = e = 0;
    uint32_t reason = 0;
    if (len < a.min_length) {
        reason = PREP_SHORT;
    } else if (len && (a.max_n != NONE || a.min_complexity)) {
        uint32_t n_cnt = 0, d_cnt = 0;
        const uint64_t pc_hi = ((uint64_t)sh + e - 1u) / PIECE;
        for (uint64_t pc = ((uint64_t)sh + b) / PIECE; pc <= pc_hi; ++pc) {
            const Chunk c = load_chunk(sbase, pc * PIECE + rk * 16u, sh, L);
            const uint32_t j15 = c.pos(15);
            // the base behind this lane's last one lies in the next lane's bytes
            const uint32_t after = (c.hi == 16u && j15 >= b && j15 + 1u < e) ? up(a.seq[start + j15 + 1u]) : 0u;
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const uint32_t j = c.pos(k);
                if (k < c.lo || k >= c.hi || j < b || j >= e) continue;
                const uint32_t u = up(c.byte(k));
                n_cnt += is_n(u) ? 1u : 0u;
                if (j + 1u < e) d_cnt += (k < 15 ? up(c.byte((k + 1u) & 15u)) : after) != u ? 1u : 0u;
            }
        }
        n_cnt = GR::gsum(n_cnt, s_x);
        d_cnt = GR::gsum(d_cnt, s_x);
        if (a.max_n != NONE && n_cnt > a.max_n) reason = PREP_N;
        else if (a.min_complexity && 100ull * d_cnt < (uint64_t)a.min_complexity * (len - 1u)) reason = PREP_COMPLEXITY;
    }
    if (rk == 0) {
        a.begin[r] = b;
        a.len[r] = len;
        a.reason[r] = reason;
    }
}

extern __shared__ uint32_t s_prep_rings[];  // a ring per group of the block

// CUT: the adapter step ran first and read r is s[0, min(L, cut[r])).  A build of its own, chosen on the host, so that the
// kernel without adapters stays the one it was.
template <int G, bool CUT>
__global__ void __launch_bounds__(256) k_prep_trim(PrepArgs a, uint32_t len_lo, uint32_t len_hi, uint32_t ring_words) {
    __shared__ uint32_t s_x[4];
    uint32_t *ring = s_prep_rings + (G == 256 ? 0u : (threadIdx.x / G) * ring_words);
    for_lengths<G>(a.off, a.n_reads, len_lo, len_hi, a.totals + PREP_TOT_ERR,
                   [&](uint64_t r, uint64_t start, uint32_t L) { prep_one<G>(a, r, start, CUT ? min(L, a.cut[r]) : L, ring, ring_words - 1u, s_x); });
}

// A thread per unit (a read; PFQ_PREP_PAIRED: a fragment): the mate rule, keep and klen per read, the totals.
__global__ void __launch_bounds__(256) k_prep_mark(PrepArgs a) {
    __shared__ unsigned long long s_t[4][PREP_TOT_ERR];
    unsigned long long t[PREP_TOT_ERR];
#pragma unroll
    for (uint32_t c = 0; c < PREP_TOT_ERR; ++c) t[c] = 0;
    const uint32_t per = a.paired ? 2u : 1u;
    const uint64_t n_units = a.n_reads / per;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t why[2];
        why[0] = a.reason[per * u];
        why[1] = a.paired ? a.reason[2u * u + 1u] : 0u;
        if (a.paired && (why[0] != 0u) != (why[1] != 0u)) {
            const uint32_t passed = why[0] ? 1u : 0u;  // the mate that passed on its own
            why[passed] = PREP_MATE;
            a.reason[2u * u + passed] = PREP_MATE;
        }
        for (uint32_t m = 0; m < per; ++m) {
            const uint64_t r = per * u + m;
            const uint64_t L = a.off[r + 1] - a.off[r];
            const uint32_t len = a.len[r], keep = why[m] == 0u ? 1u : 0u;
            a.keep[r] = keep;
            a.klen[r] = keep ? len : 0u;
#pragma unroll
            for (uint32_t c = 0; c < 5; ++c) t[PREP_TOT_REASON + c] += why[m] == c ? 1u : 0u;
            t[PREP_TOT_BASES_IN] += L;
            t[PREP_TOT_BASES_KEPT] += keep ? len : 0u;
            t[PREP_TOT_TRIMMED] += (keep && len < L) ? 1u : 0u;
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < PREP_TOT_ERR; ++c) {
        unsigned long long v = t[c];
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
        if (lane_id() == 0) s_t[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < PREP_TOT_ERR) {
        const unsigned long long v = s_t[0][threadIdx.x] + s_t[1][threadIdx.x] + s_t[2][threadIdx.x] + s_t[3][threadIdx.x];
        if (v) atomicAdd(a.totals + threadIdx.x, v);
    }
}

// kept[kpos[r]] = r and csr_off[kpos[r]] = koff[r] for the kept reads; csr_off[n_kept] = the kept bases.
__global__ void __launch_bounds__(256) k_prep_offsets(PrepArgs a) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_reads; r += (uint64_t)gridDim.x * blockDim.x) {
        if (a.keep[r]) {
            const unsigned long long j = a.kpos[r];
            a.kept[j] = (uint32_t)r;
            a.csr_off[j] = a.koff[r];
        }
        if (r + 1 == a.n_reads) a.csr_off[a.kpos[a.n_reads]] = a.koff[a.n_reads];
    }
}

// The kept interval of a read to its place, by a group.  As k_text_copy, 16 bytes wide: the destination is brought to a
// 16-byte boundary byte by byte, whole 16-byte vectors are stored from the five aligned source dwords that hold their bytes
// (joined with alignbyte; a shift of 0 passes the low word), then the last bytes.  The source dwords lie inside the input buffer:
// it begins aligned and ends 16 bytes late.
template <int G>
__device__ __forceinline__ void gather_one(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint32_t len) {
    const uint32_t rk = Grp<G>::rank();
    const uint32_t head = min(len, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    if (rk < head) dst[rk] = src[rk];
    const uint32_t nv = (len - head) >> 4, s = (uint32_t)((uintptr_t)(src + head) & 3u);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src + head - s);
    uint4 *dv = reinterpret_cast<uint4 *>(dst + head);
    for (uint32_t v = rk; v < nv; v += G) {
        const uint32_t *p = sw + 4u * (size_t)v;
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];
        uint4 o;
        o.x = __builtin_amdgcn_alignbyte(w1, w0, s);
        o.y = __builtin_amdgcn_alignbyte(w2, w1, s);
        o.z = __builtin_amdgcn_alignbyte(w3, w2, s);
        o.w = __builtin_amdgcn_alignbyte(w4, w3, s);
        dv[v] = o;
    }
    const uint32_t done = head + 16u * nv;
    if (rk < len - done) dst[done + rk] = src[done + rk];
}

template <int G>
__global__ void __launch_bounds__(256) k_prep_gather(PrepArgs a, uint32_t len_lo, uint32_t len_hi) {
    const uint64_t n_kept = a.kpos[a.n_reads];
    for_lengths<G>(a.csr_off, n_kept, len_lo, len_hi, nullptr, [&](uint64_t j, uint64_t dst, uint32_t len) {
        const uint32_t r = a.kept[j];
        gather_one<G>(a.seq + a.off[r] + a.begin[r], a.out + dst, len);
    });
}

static uint32_t pow2_at_least(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// The three builds' length ranges: [0, PREP_SHORT_MAX], (PREP_SHORT_MAX, PREP_WAVE_MAX], the rest.
void launch_prep_trim(const PrepArgs &a, hipStream_t st) {
    if (!a.n_reads) return;
    // a ring holds a piece and the W + 1 sums behind it; the sub-wave builds take blocks as small as their rings need (<= 32 KiB a block)
    const uint32_t ring16 = pow2_at_least(16u * 16u + a.trim_window + 1u), ring64 = pow2_at_least(64u * 16u + a.trim_window + 1u),
                   ring256 = pow2_at_least(256u * 16u + a.trim_window + 1u);
    const uint32_t t16 = std::max(64u, std::min(256u, (32768u / (ring16 * 4u)) * 16u / 64u * 64u)),
                   t64 = ring64 > 2048u ? 128u : 256u;
    if (a.cut) {
        hipLaunchKernelGGL((k_prep_trim<16, true>), dim3(prep_grid(a.n_reads, t16)), dim3(t16), (t16 / 16u) * ring16 * 4u, st, a, 0u, PREP_SHORT_MAX, ring16);
        hipLaunchKernelGGL((k_prep_trim<64, true>), dim3(prep_grid(a.n_reads, t64)), dim3(t64), (t64 / 64u) * ring64 * 4u, st, a, PREP_SHORT_MAX + 1u, PREP_WAVE_MAX, ring64);
        hipLaunchKernelGGL((k_prep_trim<256, true>), dim3(prep_grid(a.n_reads, 256)), dim3(256), ring256 * 4u, st, a, PREP_WAVE_MAX + 1u, 0xffffffffu, ring256);
        return;
    }
    hipLaunchKernelGGL((k_prep_trim<16, false>), dim3(prep_grid(a.n_reads, t16)), dim3(t16), (t16 / 16u) * ring16 * 4u, st, a, 0u, PREP_SHORT_MAX, ring16);
    hipLaunchKernelGGL((k_prep_trim<64, false>), dim3(prep_grid(a.n_reads, t64)), dim3(t64), (t64 / 64u) * ring64 * 4u, st, a, PREP_SHORT_MAX + 1u, PREP_WAVE_MAX, ring64);
    hipLaunchKernelGGL((k_prep_trim<256, false>), dim3(prep_grid(a.n_reads, 256)), dim3(256), ring256 * 4u, st, a, PREP_WAVE_MAX + 1u, 0xffffffffu, ring256);
}
void launch_prep_mark(const PrepArgs &a, hipStream_t st) {
    if (!a.n_reads) return;
    hipLaunchKernelGGL(k_prep_mark, dim3(prep_grid(a.n_reads / (a.paired ? 2u : 1u), 256)), dim3(256), 0, st, a);
}
void launch_prep_gather(const PrepArgs &a, hipStream_t st) {
    if (!a.n_reads) return;
    hipLaunchKernelGGL(k_prep_offsets, dim3(prep_grid(a.n_reads, 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_prep_gather<16>, dim3(prep_grid(a.n_reads, 256)), dim3(256), 0, st, a, 1u, PREP_SHORT_MAX);
    hipLaunchKernelGGL(k_prep_gather<64>, dim3(prep_grid(a.n_reads, 256)), dim3(256), 0, st, a, PREP_SHORT_MAX + 1u, PREP_WAVE_MAX);
    hipLaunchKernelGGL(k_prep_gather<256>, dim3(prep_grid(a.n_reads, 256)), dim3(256), 0, st, a, PREP_WAVE_MAX + 1u, 0xffffffffu);
}

}  // namespace pfq
