// pfq_overlap.hip — the mate overlap step of pfq_prep_reads: per fragment the insert length by the rule of pfq.h "mate overlap",
// and per read the cut that follows from it (DESIGN.md "Mate overlap").
//
//   k_prep_overlap   a wave per fragment.  The wave lays mate 1 down in LDS as two planes, a word of 2-bit codes and a word of
//                    not-ACGT bits per 16 bases, base 0 at bit 0 (planes_of on the lane's 16 aligned bytes, then a funnel shift
//                    by the mate's alignment), and mate 2 reverse-complemented: the pairs of every word reversed, the words in
//                    reverse order, code ^ 2, shifted so that base L2 - 1 comes to bit 0.  "The insert has I bases" is then the
//                    shift d = I - L2 between the two: XOR of the code planes, the pair bits folded, both not-ACGT planes ORed
//                    in, masked to the overlap, counted.  Lanes take the candidates in descending stripes of 64; the wave stops
//                    at the first stripe in which a lane matches, and a lane drops its candidate once mm exceeds the bound.
//
// Nothing per candidate touches global memory.  The totals and the histogram of the inserts gather in LDS and leave the block
// as one atomic per counter that is not zero.
//
// Mate correction (pfq.h "mate correction", DESIGN.md "Mate correction") is a second build of the kernel, chosen on the host:
// a fragment whose insert has mismatches recomputes the mismatch word of that one hypothesis from the planes still in LDS, and
// the lane of a word takes its set bits one by one: two quality bytes from global memory, the rule, a byte store each for the
// base and its quality.  Byte stores only: the bytes beside a mate are another wave's.
//   k_prep_patches   for calls that want the patch list: the overlap kernel then only counts a fragment's corrections, a scan
//                    gives every fragment its place in the list, and this kernel, a wave per fragment that has any, writes the
//                    patches from the reads as they came, ascending by (read, pos), and then corrects them.
#include "pfq_prep_groups.h"

namespace pfq {

constexpr uint32_t OVL_WORDS = OVL_LEN_MAX / 16u;   // words of a plane
constexpr uint32_t OVL_RAW = OVL_WORDS + 2u;        // the aligned span of a mate: 15 + 512 bytes are 33 lanes' 16, and a zero word
constexpr uint32_t OVL_PLANE = OVL_WORDS + 1u;      // a plane and the zero word behind it that the last funnel shift reads
// a wave's LDS: the raw words (code, not-ACGT), mate 1's planes, the planes of mate 2 reverse-complemented
constexpr uint32_t OVL_T = 0, OVL_A = 2u * OVL_RAW, OVL_R = OVL_A + 2u * OVL_PLANE, OVL_GROUP = OVL_R + 2u * OVL_PLANE;

using Wave = Grp<64>;

// The pairs of a word in reverse order.
__device__ __forceinline__ uint32_t reverse_pairs(uint32_t x) {
    x = __brev(x);
    return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
}

// A fragment as the wave holds it one trip ahead of its turn, so that the loads are under way while the fragment before is judged:
// the offsets and every lane's 16 aligned bytes of either mate.
struct Fragment {
    uint32_t sh1, sh2, L1, L2;  // the mates' first bytes in lane 0's 16, their lengths (2^32 - 1: that or more, which launch_prep_trim reports)
    Chunk c1, c2;
    __device__ __forceinline__ bool skipped() const { return L1 > OVL_LEN_MAX || L2 > OVL_LEN_MAX; }
};
__device__ __forceinline__ Fragment fetch(const OverlapArgs &a, uint64_t f) {
    Fragment x;
    const uint64_t s1 = a.off[2u * f], s2 = a.off[2u * f + 1u], end = a.off[2u * f + 2u];
    x.sh1 = (uint32_t)(s1 & 15u);
    x.sh2 = (uint32_t)(s2 & 15u);
    x.L1 = (uint32_t)min(s2 - s1, (uint64_t)NONE);
    x.L2 = (uint32_t)min(end - s2, (uint64_t)NONE);
    const bool load = !x.skipped();
    const uint32_t rk = Wave::rank();
    x.c1 = load_chunk(a.seq + (s1 - x.sh1), rk * 16u, x.sh1, load ? x.L1 : 0u);  // (nothing is loaded beyond the mate: lanes from 33 on hold zeros)
    x.c2 = load_chunk(a.seq + (s2 - x.sh2), rk * 16u, x.sh2, load ? x.L2 : 0u);
    return x;
}

// Lane rk < OVL_WORDS gets the word of each plane that holds bases 16 rk .. 16 rk + 15 of the read, zero beyond L (L <= OVL_LEN_MAX).
// ch: the lane's 16 aligned bytes, sh: the read's first byte in lane 0's.
__device__ __forceinline__ void read_words(const Chunk &ch, uint32_t sh, uint32_t L, uint32_t rk, uint32_t *p, uint32_t &wc, uint32_t &wn) {
    Wave::ring_sync();  // (the raw words of the read before have been read)
    if (rk < OVL_RAW) {
        uint32_t c, n;
        planes_of(ch, c, n);
        p[OVL_T + rk] = c;
        p[OVL_T + OVL_RAW + rk] = n;
    }
    Wave::ring_sync();
    wc = wn = 0;
    if (rk < OVL_WORDS) {
        const uint32_t m = overlap_mask(L, rk);
        wc = __builtin_amdgcn_alignbit(p[OVL_T + rk + 1u], p[OVL_T + rk], 2u * sh) & (3u * m);
        wn = __builtin_amdgcn_alignbit(p[OVL_T + OVL_RAW + rk + 1u], p[OVL_T + OVL_RAW + rk], 2u * sh) & m;
    }
}

// One fragment, by the wave: insert and mm(insert), or NONE and 0.  p: the wave's OVL_GROUP words.
__device__ __forceinline__ uint32_t overlap_one(const Fragment &x, uint32_t O, uint32_t E, uint32_t *p, uint32_t &mm_out) {
    const uint32_t rk = Wave::rank(), L1 = x.L1, L2 = x.L2;
    uint32_t wc, wn;
    read_words(x.c1, x.sh1, L1, rk, p, wc, wn);
    if (rk < OVL_PLANE) {  // (lane OVL_WORDS holds zeros)
        p[OVL_A + rk] = wc;
        p[OVL_A + OVL_PLANE + rk] = wn;
    }
    read_words(x.c2, x.sh2, L2, rk, p, wc, wn);
    Wave::ring_sync();
    // all 512 places reversed and complemented: place t holds comp(b[511 - t]), zero where there is no base
    if (rk < OVL_WORDS) {
        p[OVL_T + OVL_WORDS - 1u - rk] = reverse_pairs((wc ^ 0xAAAAAAAAu) & (3u * overlap_mask(L2, rk)));
        p[OVL_T + OVL_RAW + OVL_WORDS - 1u - rk] = reverse_pairs(wn);
    } else if (rk < OVL_RAW) {
        p[OVL_T + rk] = 0;
        p[OVL_T + OVL_RAW + rk] = 0;
    }
    Wave::ring_sync();
    if (rk < OVL_PLANE) {  // ... and moved down by 512 - L2 places, so that comp(b[L2 - 1]) is at place 0
        const uint32_t at = rk + ((OVL_LEN_MAX - L2) >> 4), by = 2u * ((OVL_LEN_MAX - L2) & 15u);
        const uint32_t c0 = at < OVL_RAW ? p[OVL_T + at] : 0u, c1 = at + 1u < OVL_RAW ? p[OVL_T + at + 1u] : 0u;
        const uint32_t n0 = at < OVL_RAW ? p[OVL_T + OVL_RAW + at] : 0u, n1 = at + 1u < OVL_RAW ? p[OVL_T + OVL_RAW + at + 1u] : 0u;
        p[OVL_R + rk] = __builtin_amdgcn_alignbit(c1, c0, by);
        p[OVL_R + OVL_PLANE + rk] = __builtin_amdgcn_alignbit(n1, n0, by);
    }
    Wave::ring_sync();
    mm_out = 0;
    if (L1 + L2 < 2u * O) return NONE;
    for (int32_t top = (int32_t)(L1 + L2 - O); top >= (int32_t)O; top -= 64) {  // (uniform in the wave)
        const int32_t I = top - (int32_t)rk;
        uint32_t hit = 0, mm = 0;
        if (I >= (int32_t)O) {
            // a[i] against r[i - d], d = I - L2: X is the plane read s = |d| places in, Y the one read from its place 0
            const int32_t d = I - (int32_t)L2;
            const uint32_t s = (uint32_t)(d >= 0 ? d : -d), x = d >= 0 ? OVL_A : OVL_R, y = d >= 0 ? OVL_R : OVL_A;
            const uint32_t o = min(d >= 0 ? L2 : L1, (d >= 0 ? L1 : L2) - s);
            if (o >= O) {
                const uint32_t bound = E * o / 100u, k = s >> 4, by = 2u * (s & 15u), nw = (o + 15u) >> 4;
                uint32_t c0 = p[x + k], n0 = p[x + OVL_PLANE + k];
                for (uint32_t w = 0; w < nw && mm <= bound; ++w) {
                    const uint32_t c1 = p[x + k + w + 1u], n1 = p[x + OVL_PLANE + k + w + 1u];
                    const uint32_t v = __builtin_amdgcn_alignbit(c1, c0, by) ^ p[y + w];
                    const uint32_t bad = v | (v >> 1) | __builtin_amdgcn_alignbit(n1, n0, by) | p[y + OVL_PLANE + w];
                    mm += (uint32_t)__popc(bad & overlap_mask(o, w));
                    c0 = c1;
                    n0 = n1;
                }
                if (mm <= bound) hit = (uint32_t)I;
            }
        }
        const uint32_t found = Wave::gmax(hit, nullptr);  // (I >= O >= 1: 0 is no match)
        if (found) {
            mm_out = Wave::gmax(hit == found ? mm : 0u, nullptr);
            return found;
        }
    }
    return NONE;
}

// The mismatching pairs of the hypothesis I, which overlap_one found: lane w gets the word bad & overlap_mask(o, w) of the
// candidate loop, read from the planes overlap_one left in p.  Bit 2 t of lane w is pair m = 16 w + t: (i, j) = (i0 + m, j0 - m).
__device__ __forceinline__ uint32_t mismatch_word(const Fragment &x, uint32_t I, const uint32_t *p, uint32_t &i0, uint32_t &j0) {
    const uint32_t w = Wave::rank(), L1 = x.L1, L2 = x.L2;
    const int32_t d = (int32_t)I - (int32_t)L2;
    const uint32_t s = (uint32_t)(d >= 0 ? d : -d), px = d >= 0 ? OVL_A : OVL_R, py = d >= 0 ? OVL_R : OVL_A;
    const uint32_t o = min(d >= 0 ? L2 : L1, (d >= 0 ? L1 : L2) - s);
    i0 = d >= 0 ? s : 0u;
    j0 = L2 - 1u - (d >= 0 ? 0u : s);
    const uint32_t k = s >> 4, by = 2u * (s & 15u), nw = (o + 15u) >> 4;
    if (w >= nw) return 0;
    const uint32_t v = __builtin_amdgcn_alignbit(p[px + k + w + 1u], p[px + k + w], by) ^ p[py + w];
    const uint32_t bad = v | (v >> 1) | __builtin_amdgcn_alignbit(p[px + OVL_PLANE + k + w + 1u], p[px + OVL_PLANE + k + w], by) | p[py + OVL_PLANE + w];
    return bad & overlap_mask(o, w);
}

__device__ __forceinline__ uint32_t comp_of(uint32_t u) { return u == 'A' ? 'T' : u == 'T' ? 'A' : u == 'C' ? 'G' : 'C'; }

// A mismatching pair by the rule: 1: mate 2's base becomes comp(up(ca)) with qa, 2: mate 1's becomes comp(up(cb)) with qb, 0: unresolved.
__device__ __forceinline__ uint32_t correct_pair(uint32_t ca, uint32_t cb, uint32_t qa, uint32_t qb, uint32_t high, uint32_t low) {
    const uint32_t pa = qa > 33u ? qa - 33u : 0u, pb = qb > 33u ? qb - 33u : 0u;
    if (!is_n(up(ca)) && pa >= high && pb <= low) return 1;
    if (!is_n(up(cb)) && pb >= high && pa <= low) return 2;
    return 0;
}

// (eight waves a SIMD: 64 VGPRs)
template <bool CORRECT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) k_prep_overlap(OverlapArgs a) {
    __shared__ uint32_t s_planes[4 * OVL_GROUP];
    __shared__ uint32_t s_hist[OVL_HIST];
    __shared__ unsigned long long s_tot[OVL_TOT_N + (CORRECT ? COR_TOT_N : 0u)];  // (the correction's behind the step's own)
    for (uint32_t i = threadIdx.x; i < OVL_HIST; i += 256u) s_hist[i] = 0;
    if (threadIdx.x < OVL_TOT_N + (CORRECT ? COR_TOT_N : 0u)) s_tot[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t g = threadIdx.x >> 6;
    const uint64_t n_frag = a.n_reads / 2u;
    const uint64_t first = (uint64_t)blockIdx.x * 4u + g, stride = (uint64_t)gridDim.x * 4u;
    Fragment next{};
    if (first < n_frag) next = fetch(a, first);
    for (uint64_t f = first; f < n_frag; f += stride) {  // (uniform in the wave)
        const Fragment x = next;
        if (f + stride < n_frag) next = fetch(a, f + stride);
        const bool skipped = x.skipped();
        uint32_t insert = NONE, mm = 0;
        if (!skipped) insert = overlap_one(x, a.min_overlap, a.max_error_percent, s_planes + g * OVL_GROUP, mm);
        if (CORRECT && mm) {  // (uniform in the wave; mm > 0: an insert was found)
            const bool has = a.cor_qual && (!a.has_qual || (a.has_qual[2u * f] && a.has_qual[2u * f + 1u]));
            uint32_t n1 = 0, n2 = 0, nu = 0;
            if (has) {
                uint32_t i0, j0;
                uint32_t word = mismatch_word(x, insert, s_planes + g * OVL_GROUP, i0, j0);
                const uint64_t at1 = a.off[2u * f] + i0 + 16u * Wave::rank(), at2 = a.off[2u * f + 1u] + j0 - 16u * Wave::rank();
                while (word) {  // (rare: a few bits a fragment)
                    const uint32_t t = (uint32_t)(__ffs((int)word) - 1) >> 1;
                    word &= word - 1u;
                    const uint64_t ia = at1 + t, jb = at2 - t;
                    const uint32_t ca = a.cor_seq[ia], cb = a.cor_seq[jb], qa = a.cor_qual[ia], qb = a.cor_qual[jb];
                    const uint32_t r = correct_pair(ca, cb, qa, qb, a.cor_high, a.cor_low);
                    if (r == 1) {
                        if (!a.cor_count) a.cor_seq[jb] = (uint8_t)comp_of(up(ca)), a.cor_qual[jb] = (uint8_t)qa;
                        ++n2;
                    } else if (r == 2) {
                        if (!a.cor_count) a.cor_seq[ia] = (uint8_t)comp_of(up(cb)), a.cor_qual[ia] = (uint8_t)qb;
                        ++n1;
                    } else {
                        ++nu;
                    }
                }
                const uint32_t all = Wave::gsum(n1 | (n2 << 10) | (nu << 20), nullptr);  // (each at most 512)
                n1 = all & 1023u, n2 = (all >> 10) & 1023u, nu = all >> 20;
            }
            if (Wave::rank() == 0) {
                if (!has) atomicAdd(s_tot + OVL_TOT_N + COR_TOT_NO_QUALITY, 1ull);
                if (n1 + n2) {
                    atomicAdd(s_tot + OVL_TOT_N + COR_TOT_FRAGMENTS, 1ull);
                    if (n1) atomicAdd(s_tot + OVL_TOT_N + COR_TOT_BASES, (unsigned long long)n1);
                    if (n2) atomicAdd(s_tot + OVL_TOT_N + COR_TOT_BASES + 1u, (unsigned long long)n2);
                    if (a.cor_count) a.cor_count[f] = n1 + n2;
                }
                if (nu) atomicAdd(s_tot + OVL_TOT_N + COR_TOT_UNRESOLVED, (unsigned long long)nu);
            }
        }
        if (Wave::rank() == 0) {
            const uint32_t L1 = x.L1, L2 = x.L2;
            const uint32_t c1 = min(L1, insert), c2 = min(L2, insert);
            a.insert[f] = insert;
            a.mismatches[f] = mm;
            a.cut[2u * f] = a.adapter_cut ? min(c1, a.adapter_cut[2u * f]) : c1;
            a.cut[2u * f + 1u] = a.adapter_cut ? min(c2, a.adapter_cut[2u * f + 1u]) : c2;
            atomicAdd(s_tot + (skipped ? OVL_TOT_SKIPPED : OVL_TOT_ANALYSED), 1ull);
            if (insert != NONE) {
                atomicAdd(s_tot + OVL_TOT_FOUND, 1ull);
                atomicAdd(s_hist + insert, 1u);
                if (insert < max(L1, L2)) atomicAdd(s_tot + OVL_TOT_THROUGH, 1ull);
                const uint32_t n_cut = (c1 < L1 ? 1u : 0u) + (c2 < L2 ? 1u : 0u);
                if (n_cut) {
                    atomicAdd(s_tot + OVL_TOT_READS, (unsigned long long)n_cut);
                    atomicAdd(s_tot + OVL_TOT_BASES, (unsigned long long)(L1 - c1) + (L2 - c2));
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < OVL_TOT_N) {  // one atomic per block and counter
        const unsigned long long v = s_tot[threadIdx.x];
        if (v) atomicAdd(a.totals + threadIdx.x, v);
    } else if (CORRECT && threadIdx.x < OVL_TOT_N + COR_TOT_N) {
        const unsigned long long v = s_tot[threadIdx.x];
        if (v) atomicAdd(a.cor_totals + (threadIdx.x - OVL_TOT_N), v);
    }
    for (uint32_t i = threadIdx.x; i < OVL_HIST; i += 256u) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(a.totals + OVL_TOT_N + i, (unsigned long long)v);
    }
}

void launch_prep_overlap(const OverlapArgs &a, hipStream_t st) {
    if (a.n_reads < 2) return;
    // eight blocks a CU: what a wave does for a fragment is a chain of short steps, and it is the other waves that fill its gaps
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(2u * PREP_GRID, (a.n_reads / 2u + 3u) / 4u));
    if (a.cor_high)
        hipLaunchKernelGGL(k_prep_overlap<true>, dim3(grid), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_prep_overlap<false>, dim3(grid), dim3(256), 0, st, a);
}

// One fragment with corrections, by the wave: the pairs of its insert once for mate 1's corrections, ascending in i, and once for
// mate 2's, ascending in j.  A pass corrects what it lists; the pairs it touches are not the other pass's (a pair corrects one side).
__device__ __forceinline__ void patch_one(const OverlapArgs &a, uint64_t f) {
    const uint32_t rk = Wave::rank();
    const uint64_t s1 = a.off[2u * f], s2 = a.off[2u * f + 1u];
    const uint32_t L1 = (uint32_t)(s2 - s1), L2 = (uint32_t)(a.off[2u * f + 2u] - s2), I = a.insert[f];
    const uint32_t lo = I > L2 ? I - L2 : 0u, hi = min(I, L1);
    unsigned long long at = a.cor_at[f];
    const unsigned long long end = a.cor_at[f + 1u];
    for (uint32_t side = 2; side >= 1; --side) {  // (2: mate 1 is corrected, then 1: mate 2)
        const uint32_t first = side == 2 ? lo : I - hi, last = side == 2 ? hi : I - lo;
        for (uint32_t base = first; base < last; base += 64u) {  // (uniform in the wave)
            const uint32_t z = base + rk, i = side == 2 ? z : I - 1u - z, j = I - 1u - i;
            bool fix = false;
            uint32_t ca = 0, cb = 0, qa = 0, qb = 0;
            if (z < last) {
                ca = a.cor_seq[s1 + i], cb = a.cor_seq[s2 + j];
                const uint32_t ua = up(ca), ub = up(cb);
                if (is_n(ua) || is_n(ub) || ua != comp_of(ub)) {
                    qa = a.cor_qual[s1 + i], qb = a.cor_qual[s2 + j];
                    fix = correct_pair(ca, cb, qa, qb, a.cor_high, a.cor_low) == side;
                }
            }
            const uint64_t m = ballot64(fix);
            if (fix) {
                CorPatch pt;
                pt.read = (uint32_t)(2u * f) + (side == 2 ? 0u : 1u);
                pt.pos = z;
                pt.base = (uint8_t)comp_of(up(side == 2 ? cb : ca));
                pt.qual = (uint8_t)(side == 2 ? qb : qa);
                pt.old_base = (uint8_t)(side == 2 ? ca : cb);
                pt.old_qual = (uint8_t)(side == 2 ? qa : qb);
                const unsigned long long slot = at + (uint32_t)__popcll(m & ((1ull << rk) - 1ull));
                if (slot < end) a.patches[slot] = pt;  // (always: the overlap kernel counted these very pairs)
                const uint64_t where = side == 2 ? s1 + i : s2 + j;
                a.cor_seq[where] = pt.base;
                a.cor_qual[where] = pt.qual;
            }
            at += (uint32_t)__popcll(m);
        }
        __threadfence_block();
    }
}

__global__ void __launch_bounds__(256) k_prep_patches(OverlapArgs a) {
    const uint64_t n_frag = a.n_reads / 2u;
    for (uint64_t base = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; base < n_frag; base += (uint64_t)gridDim.x * 256u) {  // (uniform in the wave)
        const uint64_t f = base + Wave::rank();
        uint64_t m = ballot64(f < n_frag && a.cor_count[f] != 0);
        while (m) {
            const uint32_t bit = (uint32_t)(__ffsll((unsigned long long)m) - 1);
            m &= m - 1;
            patch_one(a, base + bit);
        }
    }
}

void launch_prep_patches(const OverlapArgs &a, hipStream_t st) {
    if (a.n_reads < 2) return;
    // a block a CU: most waves only look through their 64 counts a trip and find nothing
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(PREP_GRID / 4u, (a.n_reads / 2u + 255u) / 256u));
    hipLaunchKernelGGL(k_prep_patches, dim3(grid), dim3(256), 0, st, a);
}

}  // namespace pfq
