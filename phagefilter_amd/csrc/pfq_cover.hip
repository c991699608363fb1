// pfq_cover.hip — PFQ_WANT_COVERAGE: per leaf, a HyperLogLog sketch of the distinct k-mers its units matched, beside the number
// of units that list it and of k-mers matched (DESIGN.md "Coverage").  A post-stage on the CSR the call has built, like
// pfq_lca.hip and pfq_abund.hip: no kernel of pfq_kernels.hip is involved.
//
// For every unit (a read; a fragment: both mates) and every leaf l of its row, every canonical k-mer c of the unit whose
// num_hashes probed bits are all set in l's filter (the test PFQ_WANT_SCORES counts) is logged: matched[l] += 1 and
// R[l][j] = max(R[l][j], rho), with u = mix(h1(c)), j = u >> (64 - p), rho = min(clz64(u << p), 64 - p) + 1.
// A register file is a max-monoid and the counters are integer sums, so the state is a pure function of the multiset of logged
// (k-mer, leaf) pairs: it does not depend on launch shape, atomic order or how the units were cut into calls.
//
// R is u8[n_leaves << p], [leaf << p | j].  A byte is raised with a compare-and-swap on the aligned 32-bit word that holds it,
// after a plain load has shown that it is smaller than rho (a stale load can only show a smaller value than the byte holds: the
// swap loop then sees the real one).  Once a leaf's sketch has warmed up nearly every update ends at the load.
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

// splitmix64's finaliser: the seeded hash's low bits are weak (a rotate of a multiply), the register index and rho want all 64
__device__ __forceinline__ uint64_t cover_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// R[at] = max(R[at], rho).  Lanes of one wave may name the same word, or the same byte: every lane runs its own loop, and a
// lane whose swap lost looks at what the winner left.
__device__ __forceinline__ void cover_raise(uint8_t *regs, uint64_t at, uint32_t rho) {
    uint32_t *w = reinterpret_cast<uint32_t *>(regs + (at & ~3ull));
    const uint32_t sh = 8u * (uint32_t)(at & 3ull);
    uint32_t old = __atomic_load_n(w, __ATOMIC_RELAXED);
    while (((old >> sh) & 0xffu) < rho) {
        const uint32_t want = (old & ~(0xffu << sh)) | (rho << sh);
        const uint32_t seen = atomicCAS(w, old, want);
        if (seen == old) break;
        old = seen;
    }
}

// One read of a unit against the (up to 64) leaves of a chunk of its row: lane j holds leaf j (my_leaf, filter row my_row;
// lanes j >= nh: none) and returns how many of the read's k-mers leaf j matched.  Window by window, every lane hashes its
// k-mer once.  ALL: every k-mer of the read is contained in every listed leaf, so every valid lane raises a register of every
// leaf: the byte loads of eight leaves are issued before any is looked at.  Otherwise the filters are probed as score_chunk
// does, eight loads in flight, unless `all` says the same of this read (then only the probing is left out).
template <bool ALL>
__device__ __forceinline__ uint32_t cover_chunk(BlockLds &lds, uint32_t wave, uint32_t lane, const HashParams &hp, const uint8_t *read, uint64_t n,
                                                bool all, uint32_t my_leaf, uint32_t my_row, uint32_t nh, const uint64_t *__restrict__ bits,
                                                uint64_t n_words, uint8_t *regs, uint32_t p) {
    const uint32_t H = hp.num_hashes;
    uint32_t acc = 0;
    for (uint64_t base = 0; base < n; base += WIN_KMERS) {
        const uint32_t cnt = (uint32_t)min<uint64_t>(n - base, WIN_KMERS);
        stage_window(lds, wave, read, base, cnt, hp.k);
        const bool valid = lane < cnt;
        uint64_t kh1, kh2;
        kmer_hashes(lds, wave, lane, cnt, valid, hp, kh1, kh2);
        const uint64_t u = cover_mix(kh1), w = u << p;
        const uint32_t reg = (uint32_t)(u >> (64u - p));
        const uint32_t rho = min(w ? (uint32_t)__builtin_clzll(w) : 64u, 64u - p) + 1u;
        if (ALL) {
            for (uint32_t j0 = 0; j0 < nh; j0 += 8) {
                uint32_t held[8];
#pragma unroll
                for (uint32_t b = 0; b < 8; ++b) {
                    const uint32_t leaf = bcast_u32(my_leaf, (int)min(j0 + b, nh - 1u));
                    held[b] = (valid && j0 + b < nh) ? regs[((uint64_t)leaf << p) | reg] : 0xffu;
                }
#pragma unroll
                for (uint32_t b = 0; b < 8; ++b)
                    if (held[b] < rho) cover_raise(regs, ((uint64_t)bcast_u32(my_leaf, (int)min(j0 + b, nh - 1u)) << p) | reg, rho);
            }
            acc += lane < nh ? cnt : 0u;
        } else {
            for (uint32_t j = 0; j < nh; ++j) {
                const uint64_t *f = bits + (uint64_t)bcast_u32(my_row, (int)j) * n_words;
                ProbeIter it;
                it.init(kh1, kh2, hp);
                bool in = valid;
                for (uint32_t i = 0; i < H && !all && ballot64(in) != 0; i += 8) {  // (i and all are wave-uniform)
                    uint32_t idx[8];
                    uint64_t fw[8];
#pragma unroll
                    for (uint32_t b = 0; b < 8; ++b) {
                        const uint32_t q = i + b;
                        idx[b] = q == 0 ? it.i0 : q == 1 ? it.g : q == 2 ? it.x : (q < H ? it.step(hp) : 0u);
                        fw[b] = (in && q < H) ? f[idx[b] >> 6] : ~0ull;
                    }
#pragma unroll
                    for (uint32_t b = 0; b < 8; ++b) in = in && ((fw[b] >> (idx[b] & 63u)) & 1ull);
                }
                const uint32_t c = (uint32_t)__popcll(ballot64(in));
                acc += lane == j ? c : 0u;
                if (in) {
                    const uint64_t at = ((uint64_t)bcast_u32(my_leaf, (int)j) << p) | reg;
                    if (regs[at] < rho) cover_raise(regs, at, rho);
                }
            }
        }
    }
    return acc;
}

// One wave per unit with a non-empty row; the row's leaves 64 at a time (lane j owns leaf j of the chunk: one atomic add to
// units and one to matched per (unit, leaf)).  PAIR: unit f is reads 2f and 2f + 1, both tested against every listed leaf
// whichever mate caused the listing (k_pair_scores).  An unpaired read whose need is at least its k-mer count, and in `both`
// mode such a mate, contains every k-mer in every listed leaf.  ALL: the host knows that of every read of the call (threshold
// >= 1, no `either` fragments): this instantiation holds no probing code, its registers go to the loads in flight.
template <bool PAIR, bool ALL>
__global__ void __launch_bounds__(256) k_cover_sketch(HashParams hp, const uint8_t *__restrict__ seq, const uint64_t *__restrict__ off, uint64_t n_units,
                                                      float threshold, int both, const unsigned long long *__restrict__ row_off,
                                                      const uint32_t *__restrict__ row_leaves, const uint32_t *__restrict__ col_row,
                                                      const uint64_t *__restrict__ bits, uint64_t n_words, CoverArgs cv) {
    __shared__ BlockLds lds;
    fill_complement(lds.comp);
    __syncthreads();
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    seq = in_vgpr(seq);
    off = in_vgpr(off);
    row_off = in_vgpr(row_off);
    row_leaves = in_vgpr(row_leaves);
    col_row = in_vgpr(col_row);
    unsigned long long *const units = in_vgpr(cv.units), *const matched = in_vgpr(cv.matched);
    for (uint64_t u = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; u < n_units; u += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t h0 = uniform64(row_off[u]), h1 = uniform64(row_off[u + 1]);
        if (h0 == h1) continue;
        for (uint64_t c0 = h0; c0 < h1; c0 += 64) {
            const uint32_t nh = (uint32_t)min<uint64_t>(h1 - c0, 64);
            const bool mine = lane < nh;
            const uint32_t my_leaf = mine ? row_leaves[c0 + lane] : 0u;
            // (rows hold leaf columns only; a chunk with anything else would be left out rather than written out of bounds)
            if (ballot64(my_leaf >= cv.n_leaves) != 0) continue;
            const uint32_t my_row = ALL ? 0u : col_row[my_leaf];
            uint32_t acc = 0;
            for (uint32_t mate = 0; mate < (PAIR ? 2u : 1u); ++mate) {
                const uint64_t r = PAIR ? 2 * u + mate : u;
                const uint64_t o = uniform64(off[r]), len = uniform64(off[r + 1]) - o;
                const uint64_t n = len >= hp.k ? len - hp.k + 1 : 0;
                const bool all = ALL || ((!PAIR || both) && need_kmers(threshold, n) >= n);
                acc += cover_chunk<ALL>(lds, wave, lane, hp, seq + o, n, all, my_leaf, my_row, nh, bits, n_words, cv.registers, cv.precision);
            }
            if (mine) atomicAdd(&units[my_leaf], 1ull);
            if (mine && acc) atomicAdd(&matched[my_leaf], (unsigned long long)acc);
        }
    }
}

void launch_cover_sketch(const HashParams &hp, const uint8_t *d_seq, const uint64_t *d_off, uint64_t n_units, float threshold, int pair_mode,
                         const unsigned long long *d_row_off, const uint32_t *d_row_leaves, const uint32_t *d_col_row, const uint64_t *d_bits,
                         uint64_t n_words, const CoverArgs &cv, uint32_t blocks, hipStream_t st) {
    if (!n_units || !cv.n_leaves) return;
    if (!blocks) blocks = (uint32_t)std::min<uint64_t>((n_units + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 8192);
    // threshold >= 1: need_kmers(threshold, n) >= n for every n (the f32 product is rounded monotonically and n * 1.0f = (float)n)
    const bool all = threshold >= 1.0f && pair_mode != 1;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, hp, d_seq, d_off, n_units, threshold, pair_mode == 2 ? 1 : 0, d_row_off, d_row_leaves,
                           d_col_row, d_bits, n_words, cv);
    };
    if (pair_mode) all ? go(k_cover_sketch<true, true>) : go(k_cover_sketch<true, false>);
    else all ? go(k_cover_sketch<false, true>) : go(k_cover_sketch<false, false>);
}

}  // namespace pfq
