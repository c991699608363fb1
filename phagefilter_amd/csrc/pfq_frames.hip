// pfq_frames.hip — pfq_query_frames: long sequences classified in overlapping frames, runs of frames merged into segments and
// every segment refined to k-mer resolution (DESIGN.md "Frames and segments").  The shape of PFQ_PAIRED: the inner units (here
// the frames) are classified by the ordinary query path into a count sink, and a post-stage on their CSR combines them.  Like
// pfq_lca.hip, pfq_abund.hip and pfq_cover.hip: no kernel of pfq_kernels.hip is involved beyond the scan behind launch_scan_u32.
//
//   before the classification   k_frame_count -> scans -> k_frame_table -> k_frame_copy   (the frames' own CSR byte buffer)
//   after it                    k_seg_count -> scan -> k_seq_seg_off | k_seg_fill -> k_seg_walk -> k_seq_counts
//                               k_piece_count -> scan -> k_seg_refine -> k_seg_combine
//
// Every result is a pure function of the frames' rows: segments are found in CSR order (sequence, frame, leaf), which is the
// order they are delivered in, and the partial results of the refinement form a monoid that is folded in piece order.
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

// ---- frame table and cut ------------------------------------------------------------------------------------------------

// Frames of a sequence of L bases: one if L <= F, else ceil((L - F) / S) + 1 (the last one flush with the end).  deficit = what a
// lone frame is shorter than F: frame f's bytes then start at F * f - (the deficits of the sequences before its own).
__global__ void __launch_bounds__(256) k_frame_count(const uint64_t *__restrict__ off, uint64_t n_seqs, uint32_t F, uint32_t S, uint32_t *__restrict__ cnt,
                                                     uint32_t *__restrict__ deficit, unsigned long long *__restrict__ err) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_seqs; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t L = off[i + 1] - off[i];
        if (L >> 32) {  // (offsets that run backwards land here as well)
            atomicOr(err, 1ull);
            L = 0;
        }
        cnt[i] = L <= F ? 1u : (uint32_t)((L - F + S - 1) / S + 1);
        deficit[i] = L <= F ? F - (uint32_t)L : 0u;
    }
}

// the sequence of frame f: the last i with seq_frame0[i] <= f (every sequence has a frame: strictly ascending)
__device__ __forceinline__ uint64_t frame_owner(const unsigned long long *__restrict__ seq_frame0, uint64_t n_seqs, uint64_t f) {
    uint64_t lo = 0, hi = n_seqs;  // seq_frame0[lo] <= f < seq_frame0[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (seq_frame0[mid] <= f) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) k_frame_table(FrameArgs fa) {
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < fa.n_frames; f += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = frame_owner(fa.seq_frame0, fa.n_seqs, f);
        const uint64_t j = f - fa.seq_frame0[i], L = fa.seq_off[i + 1] - fa.seq_off[i];
        fa.frame_seq[f] = (uint32_t)i;
        fa.frame_start[f] = L <= fa.frame ? 0u : (uint32_t)min<uint64_t>(j * fa.step, L - fa.frame);
        fa.frame_off[f] = (uint64_t)fa.frame * f - fa.seq_deficit[i];
        if (f + 1 == fa.n_frames) fa.frame_off[f + 1] = (uint64_t)fa.frame * fa.n_frames - fa.seq_deficit[fa.n_seqs];
    }
}

// One wave per frame.  The destination is brought to a dword boundary byte by byte, then whole dwords are stored; the source
// is read as the aligned dwords that hold those bytes (two per store, joined with alignbyte, when the two are not aligned
// alike: both hold bytes of the frame, so nothing outside the sequence's own dwords is touched), then the last bytes.
__global__ void __launch_bounds__(256) k_frame_copy(FrameArgs fa, const uint8_t *__restrict__ seq, uint8_t *__restrict__ out) {
    const uint32_t lane = lane_id();
    const uint64_t wave0 = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    for (uint64_t f = wave0; f < fa.n_frames; f += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t o = fa.frame_off[f];
        const uint32_t len = (uint32_t)(fa.frame_off[f + 1] - o);
        const uint8_t *src = seq + fa.seq_off[fa.frame_seq[f]] + fa.frame_start[f];
        uint8_t *dst = out + o;
        const uint32_t head = min(len, (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
        if (lane < head) dst[lane] = src[lane];
        const uint32_t nd = (len - head) >> 2, sh = (uint32_t)((uintptr_t)(src + head) & 3u);
        const uint32_t *sw = reinterpret_cast<const uint32_t *>(src + head - sh);
        uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
        if (sh == 0) {  // (wave-uniform)
            for (uint32_t d = lane; d < nd; d += 64) dw[d] = sw[d];
        } else {
            for (uint32_t d = lane; d < nd; d += 64) dw[d] = __builtin_amdgcn_alignbyte(sw[d + 1], sw[d], sh);
        }
        const uint32_t done = head + 4u * nd;
        if (lane < len - done) dst[done + lane] = src[done + lane];
    }
}

void launch_frame_count(const uint64_t *d_seq_off, uint64_t n_seqs, uint32_t frame, uint32_t step, uint32_t *d_cnt, uint32_t *d_deficit,
                        unsigned long long *d_err, hipStream_t st) {
    if (!n_seqs) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_seqs + 255) / 256, 4096);
    hipLaunchKernelGGL(k_frame_count, dim3(blocks), dim3(256), 0, st, d_seq_off, n_seqs, frame, step, d_cnt, d_deficit, d_err);
}
void launch_frame_cut(const FrameArgs &fa, const uint8_t *d_seq, uint8_t *d_out, hipStream_t st) {
    if (!fa.n_frames) return;
    hipLaunchKernelGGL(k_frame_table, dim3((uint32_t)std::min<uint64_t>((fa.n_frames + 255) / 256, 4096)), dim3(256), 0, st, fa);
    hipLaunchKernelGGL(k_frame_copy, dim3((uint32_t)std::min<uint64_t>((fa.n_frames + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 16384)), dim3(256), 0, st, fa,
                       d_seq, d_out);
}

// ---- segments -----------------------------------------------------------------------------------------------------------

// l in the ascending leaves[a, b)?
__device__ __forceinline__ bool row_has(const uint32_t *__restrict__ leaves, uint64_t a, uint64_t b, uint32_t l) {
    while (a < b) {
        const uint64_t mid = a + (b - a) / 2;
        const uint32_t v = leaves[mid];
        if (v == l) return true;
        if (v < l) a = mid + 1;
        else b = mid;
    }
    return false;
}

// One wave per frame; its row 64 entries at a time.  Entry (j, l) opens a segment iff j is its sequence's first frame or l is
// not in the row before.  FILL = false: open_cnt[f] = the frame's opening entries.  FILL = true: seg_pos[f] (their scan) is
// where the frame's segments go, in row order — sequence, first frame, leaf: the order of delivery.  An opening lane writes
// leaf, first_frame and begin, walks up to SEG_WALK rows forward, and queues the segment for k_seg_walk if it is still open
// then.  The entries of a one-frame sequence are its leaf set: they are counted here.
constexpr uint32_t SEG_WALK = 8;
__device__ __forceinline__ void seg_close(const SegArgs &sa, uint64_t p, uint64_t f0, uint64_t g) {  // the run is frames [f0, g)
    sa.seg[p].n_frames = (uint32_t)(g - f0);
    sa.seg[p].end = sa.frame_start[g - 1] + (uint32_t)(sa.frame_off[g] - sa.frame_off[g - 1]);
}
template <bool FILL>
__global__ void __launch_bounds__(256) k_seg_open(SegArgs sa) {
    const uint32_t lane = lane_id();
    const uint64_t wave0 = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    for (uint64_t f = wave0; f < sa.n_frames; f += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t r0 = sa.row_off[f], r1 = sa.row_off[f + 1];
        if (r0 == r1) {
            if (!FILL && lane == 0) sa.open_cnt[f] = 0;
            continue;
        }
        const uint32_t i = sa.frame_seq[f];
        const uint64_t f_first = sa.seq_frame0[i], f_end = sa.seq_frame0[i + 1];
        const bool first = f == f_first;
        const uint64_t p0 = first ? r0 : sa.row_off[f - 1];
        uint64_t run = FILL ? sa.seg_pos[f] : 0;
        for (uint64_t c = r0; c < r1; c += 64) {
            const uint64_t e = c + lane;
            const uint32_t l = e < r1 ? sa.row_leaves[e] : 0u;
            const bool opens = e < r1 && l < sa.n_leaves && (first || !row_has(sa.row_leaves, p0, r0, l));
            const uint64_t m = ballot64(opens);
            if (FILL && opens) {
                const uint64_t p = run + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
                Segment &s = sa.seg[p];
                s.leaf = l;
                s.first_frame = (uint32_t)(f - f_first);
                s.begin = sa.frame_start[f];
                sa.seg_seq[p] = i;
                if (f_end - f_first == 1) atomicAdd(&sa.counts[l], 1ull);
                uint64_t g = f + 1;
                bool open = g < f_end;
                for (uint32_t w = 0; open && w < SEG_WALK; ++w) {
                    if (!row_has(sa.row_leaves, sa.row_off[g], sa.row_off[g + 1], l)) open = false;
                    else open = ++g < f_end;
                }
                if (open) {  // still open after SEG_WALK rows: a wave takes over at row g
                    s.n_frames = (uint32_t)(g - f);
                    sa.queue[atomicAdd(sa.n_queued, 1ull)] = (uint32_t)p;
                } else seg_close(sa, p, f, g);
            }
            run += (uint64_t)__popcll(m);
        }
        if (!FILL && lane == 0) sa.open_cnt[f] = (uint32_t)run;
    }
}

// One wave per queued segment: 64 following rows a pass, lane t looks for the leaf in row g + t; the first row without it
// ends the run.  A segment of n frames costs n / 64 passes of one binary search each.
__global__ void __launch_bounds__(256) k_seg_walk(SegArgs sa) {
    const uint32_t lane = lane_id();
    const uint64_t n_q = *sa.n_queued;
    for (uint64_t q = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6); q < n_q; q += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint32_t p = sa.queue[q];
        const uint32_t i = sa.seg_seq[p], l = sa.seg[p].leaf;
        const uint64_t f0 = sa.seq_frame0[i] + sa.seg[p].first_frame, f_end = sa.seq_frame0[i + 1];
        uint64_t g = f0 + sa.seg[p].n_frames;
        while (g < f_end) {
            const uint32_t nv = (uint32_t)min<uint64_t>(64, f_end - g);
            const bool has = lane < nv && row_has(sa.row_leaves, sa.row_off[g + lane], sa.row_off[g + lane + 1], l);
            const uint64_t miss = ~ballot64(has) & (nv == 64 ? ~0ull : (1ull << nv) - 1ull);
            if (miss) {
                g += (uint32_t)__builtin_ctzll(miss);
                break;
            }
            g += nv;
        }
        if (lane == 0) seg_close(sa, p, f0, g);
    }
}

// seq_seg_off[i] = the first segment of sequence i = where its first frame's segments go
__global__ void __launch_bounds__(256) k_seq_seg_off(const unsigned long long *__restrict__ seq_frame0, const unsigned long long *__restrict__ seg_pos,
                                                     uint64_t n_seqs, unsigned long long *__restrict__ seq_seg_off) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_seqs; i += (uint64_t)gridDim.x * blockDim.x)
        seq_seg_off[i] = seg_pos[seq_frame0[i]];
}

// Leaf counters of the sequences of several frames: += 1 per distinct leaf among a sequence's segments.  One block per
// sequence keeps a bitmap of the leaves in LDS; the old value of atomicOr says who set a bit first, and that thread counts.
// SEQ_BITMAP_LEAVES leaves fit (16 KiB); a wider tree is taken in ranges of that many, one pass over the segments per range.
constexpr uint32_t SEQ_BITMAP_LEAVES = 131072;
__global__ void __launch_bounds__(256) k_seq_counts(SegArgs sa, const unsigned long long *__restrict__ seq_seg_off, uint64_t n_seqs) {
    __shared__ uint32_t s_seen[SEQ_BITMAP_LEAVES / 32];
    for (uint64_t i = blockIdx.x; i < n_seqs; i += gridDim.x) {
        if (sa.seq_frame0[i + 1] - sa.seq_frame0[i] == 1) continue;  // (counted by k_seg_open; uniform over the block)
        const uint64_t s0 = seq_seg_off[i], s1 = seq_seg_off[i + 1];
        if (s1 - s0 == 1) {
            if (threadIdx.x == 0) atomicAdd(&sa.counts[sa.seg[s0].leaf], 1ull);
            continue;
        }
        if (s0 == s1) continue;
        for (uint32_t base = 0; base < sa.n_leaves; base += SEQ_BITMAP_LEAVES) {
            const uint32_t span = min(sa.n_leaves - base, SEQ_BITMAP_LEAVES);
            __syncthreads();
            for (uint32_t w = threadIdx.x; w < (span + 31) / 32; w += blockDim.x) s_seen[w] = 0;
            __syncthreads();
            for (uint64_t s = s0 + threadIdx.x; s < s1; s += blockDim.x) {
                const uint32_t l = sa.seg[s].leaf - base;  // (below base: wraps past span)
                if (l < span && !((atomicOr(&s_seen[l >> 5], 1u << (l & 31u)) >> (l & 31u)) & 1u)) atomicAdd(&sa.counts[base + l], 1ull);
            }
        }
    }
}

void launch_seg_count(const SegArgs &sa, hipStream_t st) {
    if (!sa.n_frames) return;
    hipLaunchKernelGGL(k_seg_open<false>, dim3((uint32_t)std::min<uint64_t>((sa.n_frames + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 16384)), dim3(256), 0, st, sa);
}
void launch_seq_seg_off(const unsigned long long *d_seq_frame0, const unsigned long long *d_seg_pos, uint64_t n_seqs, unsigned long long *d_seq_seg_off,
                        hipStream_t st) {
    hipLaunchKernelGGL(k_seq_seg_off, dim3((uint32_t)std::min<uint64_t>((n_seqs + 256) / 256, 4096)), dim3(256), 0, st, d_seq_frame0, d_seg_pos, n_seqs,
                       d_seq_seg_off);
}
void launch_seg_fill(const SegArgs &sa, const unsigned long long *d_seq_seg_off, uint64_t n_seqs, uint64_t n_segs, hipStream_t st) {
    if (!sa.n_frames || !n_segs) return;
    hipLaunchKernelGGL(k_seg_open<true>, dim3((uint32_t)std::min<uint64_t>((sa.n_frames + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 16384)), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_seg_walk, dim3((uint32_t)std::min<uint64_t>((n_segs + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 2048)), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_seq_counts, dim3((uint32_t)std::min<uint64_t>(n_seqs, 4096)), dim3(256), 0, st, sa, d_seq_seg_off, n_seqs);
}

// ---- refinement ---------------------------------------------------------------------------------------------------------

// The match mask of a stretch of k-mer positions, reduced: a monoid under part_join (associative, part_unit its unit), so a
// segment's result does not depend on how its positions are cut into pieces.  first / last: positions of the first and last
// match within the stretch (meaningless while matched == 0); pre / suf: matches at its start / end; best: the longest run.
__host__ __device__ __forceinline__ FramePart part_join(const FramePart &a, const FramePart &b) {
    FramePart r;
    r.len = a.len + b.len;
    r.matched = a.matched + b.matched;
    r.first = a.matched ? a.first : a.len + b.first;
    r.last = b.matched ? a.len + b.last : a.last;
    r.pre = a.pre == a.len ? a.len + b.pre : a.pre;
    r.suf = b.suf == b.len ? b.len + a.suf : b.suf;
    r.best = max(max(a.best, b.best), a.suf + b.pre);
    r.pad_ = 0;
    return r;
}
// the part of one pass: bit q of m = position q matches, cnt (1..64) positions, no bit set beyond them
__device__ __forceinline__ FramePart part_of_mask(uint64_t m, uint32_t cnt) {
    FramePart r;
    r.len = cnt;
    r.matched = (uint32_t)__popcll(m);
    r.first = m ? (uint32_t)__builtin_ctzll(m) : 0u;
    r.last = m ? 63u - (uint32_t)__builtin_clzll(m) : 0u;
    const uint64_t holes = ~m;                 // (bit cnt, if there is one, is a hole: ctz <= cnt)
    r.pre = holes ? (uint32_t)__builtin_ctzll(holes) : 64u;
    const uint64_t top = ~(m << (64u - cnt));  // position cnt - 1 at bit 63, holes below position 0: clz <= cnt
    r.suf = top ? (uint32_t)__builtin_clzll(top) : 64u;
    uint32_t best = 0;
    for (uint64_t x = m; x; x &= x << 1) ++best;
    r.best = best;
    r.pad_ = 0;
    return r;
}

__global__ void __launch_bounds__(256) k_piece_count(const Segment *__restrict__ seg, uint64_t n_segs, uint32_t k, uint32_t piece, uint32_t *__restrict__ cnt) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_segs; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t len = seg[p].end - seg[p].begin;
        const uint32_t kmers = len >= k ? len - k + 1 : 0u;
        cnt[p] = kmers / piece + (kmers % piece ? 1u : 0u);
    }
}

// One wave per piece of at most `piece` k-mer positions of one segment, on the sequence itself (not on the frames' copy): every
// lane hashes its k-mer of a window once and probes the segment's leaf's own filter, eight loads in flight, as score_chunk
// does; the ballot is the window's match mask.  Cold pointers wait in vector registers (in_vgpr), what is loaded through them
// is wave-uniform (uniform64).
__global__ void __launch_bounds__(256) k_seg_refine(HashParams hp, const uint8_t *__restrict__ seq, const uint64_t *__restrict__ seq_off,
                                                    const Segment *__restrict__ seg, const uint32_t *__restrict__ seg_seq,
                                                    const unsigned long long *__restrict__ piece_off, uint64_t n_segs, uint64_t n_pieces, uint32_t piece,
                                                    const uint32_t *__restrict__ col_row, const uint64_t *__restrict__ bits, uint64_t n_words,
                                                    FramePart *__restrict__ parts) {
    __shared__ BlockLds lds;
    fill_complement(lds.comp);
    __syncthreads();
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6, H = hp.num_hashes;
    seq = in_vgpr(seq);
    seq_off = in_vgpr(seq_off);
    seg = in_vgpr(seg);
    seg_seq = in_vgpr(seg_seq);
    piece_off = in_vgpr(piece_off);
    col_row = in_vgpr(col_row);
    parts = in_vgpr(parts);
    for (uint64_t q = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; q < n_pieces; q += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        uint64_t lo = 0, hi = n_segs;  // the last segment with piece_off[p] <= q (it has pieces: piece_off[p + 1] > q)
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (uniform64(piece_off[mid]) <= q) lo = mid;
            else hi = mid;
        }
        const uint64_t p = lo;
        const uint32_t s_begin = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[p].begin), s_end = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[p].end);
        const uint32_t leaf = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[p].leaf), si = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg_seq[p]);
        const uint32_t kmers = s_end - s_begin - hp.k + 1;  // (a segment with pieces has k-mers)
        const uint32_t k0 = (uint32_t)(q - uniform64(piece_off[p])) * piece;
        const uint32_t n = min(piece, kmers - k0);
        const uint8_t *read = seq + uniform64(seq_off[si]) + s_begin + k0;
        const uint64_t *f = bits + (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)col_row[leaf]) * n_words;
        FramePart acc{0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t base = 0; base < n; base += WIN_KMERS) {
            const uint32_t cnt = min(n - base, WIN_KMERS);
            stage_window(lds, wave, read, base, cnt, hp.k);
            const bool valid = lane < cnt;
            uint64_t kh1, kh2;
            kmer_hashes(lds, wave, lane, cnt, valid, hp, kh1, kh2);
            ProbeIter it;
            it.init(kh1, kh2, hp);
            bool in = valid;
            for (uint32_t i = 0; i < H && ballot64(in) != 0; i += 8) {  // (i is wave-uniform)
                uint32_t idx[8];
                uint64_t w[8];
#pragma unroll
                for (uint32_t b = 0; b < 8; ++b) {
                    const uint32_t pr = i + b;
                    idx[b] = pr == 0 ? it.i0 : pr == 1 ? it.g : pr == 2 ? it.x : (pr < H ? it.step(hp) : 0u);
                    w[b] = (in && pr < H) ? f[idx[b] >> 6] : ~0ull;
                }
#pragma unroll
                for (uint32_t b = 0; b < 8; ++b) in = in && ((w[b] >> (idx[b] & 63u)) & 1ull);
            }
            acc = part_join(acc, part_of_mask(ballot64(in), cnt));
        }
        if (lane == 0) parts[q] = acc;
    }
}

// the pieces of a segment folded in order
__global__ void __launch_bounds__(256) k_seg_combine(Segment *__restrict__ seg, uint64_t n_segs, uint32_t k, const unsigned long long *__restrict__ piece_off,
                                                     const FramePart *__restrict__ parts) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_segs; p += (uint64_t)gridDim.x * blockDim.x) {
        FramePart acc{0, 0, 0, 0, 0, 0, 0, 0};
        for (uint64_t q = piece_off[p]; q < piece_off[p + 1]; ++q) acc = part_join(acc, parts[q]);
        Segment &s = seg[p];
        s.kmers = acc.len;
        s.matched = acc.matched;
        s.match_begin = acc.matched ? s.begin + acc.first : s.begin;
        s.match_end = acc.matched ? s.begin + acc.last + k : s.begin;
        s.longest_run = acc.best;
    }
}

void launch_piece_count(const Segment *d_seg, uint64_t n_segs, uint32_t k, uint32_t piece, uint32_t *d_cnt, hipStream_t st) {
    if (!n_segs) return;
    hipLaunchKernelGGL(k_piece_count, dim3((uint32_t)std::min<uint64_t>((n_segs + 255) / 256, 4096)), dim3(256), 0, st, d_seg, n_segs, k, piece, d_cnt);
}
void launch_seg_refine(const HashParams &hp, const uint8_t *d_seq, const uint64_t *d_seq_off, Segment *d_seg, const uint32_t *d_seg_seq,
                       const unsigned long long *d_piece_off, uint64_t n_segs, uint64_t n_pieces, uint32_t piece, const uint32_t *d_col_row,
                       const uint64_t *d_bits, uint64_t n_words, FramePart *d_parts, hipStream_t st) {
    if (!n_segs) return;
    if (n_pieces)
        hipLaunchKernelGGL(k_seg_refine, dim3((uint32_t)std::min<uint64_t>((n_pieces + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 8192)), dim3(256), 0, st, hp, d_seq,
                           d_seq_off, d_seg, d_seg_seq, d_piece_off, n_segs, n_pieces, piece, d_col_row, d_bits, n_words, d_parts);
    hipLaunchKernelGGL(k_seg_combine, dim3((uint32_t)std::min<uint64_t>((n_segs + 255) / 256, 4096)), dim3(256), 0, st, d_seg, n_segs, hp.k, d_piece_off, d_parts);
}

}  // namespace pfq
