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

// (eight waves a SIMD: 64 VGPRs)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) k_prep_overlap(OverlapArgs a) {
    __shared__ uint32_t s_planes[4 * OVL_GROUP];
    __shared__ uint32_t s_hist[OVL_HIST];
    __shared__ unsigned long long s_tot[OVL_TOT_N];
    for (uint32_t i = threadIdx.x; i < OVL_HIST; i += 256u) s_hist[i] = 0;
    if (threadIdx.x < OVL_TOT_N) s_tot[threadIdx.x] = 0;
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
    hipLaunchKernelGGL(k_prep_overlap, dim3(grid), dim3(256), 0, st, a);
}

}  // namespace pfq
