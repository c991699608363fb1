// pfq_emit.hip — pfq_text_format: the POS / NEG records of a device-parsed block formatted on the device (DESIGN.md "Device-side
// output", the rules are pfq.h "text output").  Everything is read where pfq_text_parse and pfq_text_query left it: the text
// and its line table, the gathered sequences, the ascending hit rows.
//
//   k_fmt_ids                       per record: where its id lies in the text, a 64-bit hash of it
//   k_fmt_blocks                    per whole result block: the (hash, index) keys sorted in LDS, equal hashes settled by
//                                   comparing the bytes; state[b] = 1 if two records of the block share an id
//   k_fmt_sizes [k_fmt_sizes_long]  pos_len / neg_len per record (0: not emitted); rows of more than 64 names by a wave each
//   two scans, k_fmt_bounds         every record's place in its stream; the places of the block boundaries and the totals
//   k_fmt_emit                      a wave per record: marker, id, names, sequence (letters raised), quality
//
// Every index into the text is 32 bits wide (pfq_text_parse refuses 2^31 bytes or more).  The text buffer and the sequence
// buffer begin 16-byte aligned and end at least 16 bytes late, so the aligned dword reads of wave_copy stay inside them.
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

constexpr uint32_t FMT_IDX_BITS = 13;  // a record's index in its result block
static_assert((1u << FMT_IDX_BITS) == FMT_BLOCK_MAX, "the keys of k_fmt_blocks hold an index below FMT_BLOCK_MAX");

__device__ __forceinline__ bool fmt_blank(uint32_t c) { return c == ' ' || (c >= 9u && c <= 13u); }  // ' ', \t \n \v \f \r
__device__ __forceinline__ uint32_t fmt_trimmed(const uint8_t *__restrict__ text, uint32_t s, uint32_t e) {
    while (e > s && fmt_blank(text[e - 1u])) --e;
    return e - s;
}
__device__ __forceinline__ uint32_t fmt_header_line(const FmtArgs &a, uint32_t r) { return a.fastq ? 4u * r : a.rec_line[r]; }
__device__ __forceinline__ bool fmt_in_whole(const FmtArgs &a, uint32_t r) { return r >= a.head && r - a.head < a.n_whole * a.block; }

// id(r): the header line trimmed, from its second byte to the first separator (FASTQ: ' '; FASTA: any blank) — Batch::push_id.
__global__ void __launch_bounds__(256) k_fmt_ids(FmtArgs a) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += gridDim.x * blockDim.x) {
        const uint32_t hl = fmt_header_line(a, r), s = a.line_start[hl], e = a.line_start[hl + 1u] - 1u;
        const uint32_t te = s + fmt_trimmed(a.text, s, e);
        uint32_t i = s + 1u;
        uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a, then mixed: the keys of k_fmt_blocks keep its low bits
        while (i < te) {
            const uint32_t c = a.text[i];
            if (a.fastq ? c == ' ' : fmt_blank(c)) break;
            h = (h ^ c) * 0x100000001b3ull;
            ++i;
        }
        h = splitmix64(h);
        if (a.hash_bits < 64u) h &= (1ull << a.hash_bits) - 1ull;
        a.id_beg[r] = s + 1u;
        a.id_len[r] = i > s + 1u ? i - (s + 1u) : 0u;
        a.hash[r] = h;
    }
}

__device__ __forceinline__ bool fmt_same_id(const FmtArgs &a, uint32_t x, uint32_t y) {
    const uint32_t n = a.id_len[x];
    if (n != a.id_len[y]) return false;
    const uint8_t *p = a.text + a.id_beg[x], *q = a.text + a.id_beg[y];
    for (uint32_t i = 0; i < n; ++i)
        if (p[i] != q[i]) return false;
    return true;
}

// One workgroup per whole result block: keys (hash << 13 | index in the block) of `pad` slots (a power of two >= block; the
// slots beyond the block hold keys with an index >= block, which sort behind every record of the same hash) sorted in LDS by
// a bitonic network; then every record looks at the records behind it with the same 51 hash bits and compares the bytes.
// state[b] is zero when the kernel starts; every thread that finds a repeated id writes the same 1.
__global__ void __launch_bounds__(1024) k_fmt_blocks(FmtArgs a, uint32_t pad) {
    extern __shared__ unsigned long long s_key[];
    const uint32_t idx_mask = FMT_BLOCK_MAX - 1u;
    for (uint32_t b = blockIdx.x; b < a.n_whole; b += gridDim.x) {  // (uniform: every thread meets the barriers)
        const uint32_t r0 = a.head + b * a.block;
        for (uint32_t i = threadIdx.x; i < pad; i += blockDim.x)
            s_key[i] = ((i < a.block ? a.hash[r0 + i] : ~0ull) << FMT_IDX_BITS) | i;
        __syncthreads();
        for (uint32_t k = 2; k <= pad; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = threadIdx.x; i < pad; i += blockDim.x) {
                    const uint32_t p = i ^ j;
                    if (p > i) {
                        const unsigned long long x = s_key[i], y = s_key[p];
                        if ((x > y) == ((i & k) == 0u)) {
                            s_key[i] = y;
                            s_key[p] = x;
                        }
                    }
                }
                __syncthreads();
            }
        for (uint32_t i = threadIdx.x; i < pad; i += blockDim.x) {
            const unsigned long long x = s_key[i];
            const uint32_t xi = (uint32_t)x & idx_mask;
            if (xi >= a.block) continue;
            for (uint32_t j = i + 1u; j < pad; ++j) {
                const unsigned long long y = s_key[j];
                const uint32_t yi = (uint32_t)y & idx_mask;
                if ((y >> FMT_IDX_BITS) != (x >> FMT_IDX_BITS) || yi >= a.block) break;
                if (fmt_same_id(a, r0 + xi, r0 + yi)) {
                    a.state[b] = 1u;
                    break;
                }
            }
        }
        __syncthreads();  // (the next block's keys overwrite these)
    }
}

__device__ __forceinline__ uint32_t fmt_name_len(const FmtArgs &a, uint32_t leaf) { return a.name_off[leaf + 1u] - a.name_off[leaf]; }

// pos_len[r] / neg_len[r]: the bytes record r adds to its stream — 0 unless it lies in a whole plain block and its stream is
// asked for.  A row of more than 64 names: the length without the names, and r goes to long_list for k_fmt_sizes_long.
__global__ void __launch_bounds__(256) k_fmt_sizes(FmtArgs a) {
    uint32_t n_pos = 0, n_neg = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += gridDim.x * blockDim.x) {
        uint32_t pos = 0, neg = 0;
        if (fmt_in_whole(a, r) && a.state[(r - a.head) / a.block] == 0u) {
            const unsigned long long cnt = a.row_off[r + 1u] - a.row_off[r];
            const bool mapped = cnt != 0;
            if (a.flags & (mapped ? FMT_POS : FMT_NEG)) {
                unsigned long long len = 1ull + a.id_len[r] + 1ull + (a.seq_off[r + 1u] - a.seq_off[r]) + 1ull;
                if (a.fastq) {
                    const uint32_t ql = 4u * r + 3u, s = a.line_start[ql], e = a.line_start[ql + 1u] - 1u;
                    len += 2ull + fmt_trimmed(a.text, s, e) + 1ull;
                }
                if (mapped) {
                    len += 2ull + (cnt - 1ull);
                    if (cnt <= 64ull) {
                        const uint32_t *row = a.row_leaves + a.row_off[r];
                        for (uint32_t j = 0; j < (uint32_t)cnt; ++j) len += fmt_name_len(a, row[j]);
                    } else if (len < (1ull << 32)) {
                        a.long_list[atomicAdd(a.res + FMT_RES_LONG, 1ull)] = r;
                    }
                }
                if (len >= (1ull << 32)) {
                    atomicOr(a.res + FMT_RES_ERR, 1ull);
                    len = 0;
                }
                if (mapped) pos = (uint32_t)len, n_pos += len != 0;
                else neg = (uint32_t)len, n_neg += len != 0;
            }
        }
        a.len[0][r] = pos;
        a.len[1][r] = neg;
    }
    for (int d = 32; d > 0; d >>= 1) {
        n_pos += __shfl_down(n_pos, d);
        n_neg += __shfl_down(n_neg, d);
    }
    if (lane_id() == 0) {
        if (n_pos) atomicAdd(a.res + FMT_RES_POS_RECORDS, (unsigned long long)n_pos);
        if (n_neg) atomicAdd(a.res + FMT_RES_NEG_RECORDS, (unsigned long long)n_neg);
    }
}

// A wave per listed record adds the lengths of its row's names (as k_tax_long takes the long rows of its stage).
__global__ void __launch_bounds__(256) k_fmt_sizes_long(FmtArgs a) {
    const uint32_t lane = lane_id(), wpb = blockDim.x >> 6;
    const unsigned long long n_long = a.res[FMT_RES_LONG];
    for (unsigned long long q = (unsigned long long)blockIdx.x * wpb + (threadIdx.x >> 6); q < n_long; q += (unsigned long long)gridDim.x * wpb) {
        const uint32_t r = a.long_list[q];
        const unsigned long long o0 = a.row_off[r], o1 = a.row_off[r + 1u];
        unsigned long long sum = 0;
        for (unsigned long long j = o0 + lane; j < o1; j += 64) sum += fmt_name_len(a, a.row_leaves[j]);
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
        if (lane == 0) {
            const unsigned long long len = a.len[0][r] + sum;  // (a mapped record: the POS stream)
            if (len >= (1ull << 32)) {
                atomicOr(a.res + FMT_RES_ERR, 1ull);
                atomicAdd(a.res + FMT_RES_POS_RECORDS, ~0ull);  // (-1: the record is not emitted)
                a.len[0][r] = 0;
            } else a.len[0][r] = (uint32_t)len;
        }
    }
}

// bounds[2 i + s]: where in stream s the records from head + i * block on belong, i <= n_whole; bounds[2 (n_whole + 1) + s]: the
// stream's total.
__global__ void __launch_bounds__(256) k_fmt_bounds(FmtArgs a) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= a.n_whole + 1u; i += gridDim.x * blockDim.x) {
        const uint32_t r = i <= a.n_whole ? a.head + i * a.block : a.n;
        a.bounds[2u * i] = a.dst[0][r];
        a.bounds[2u * i + 1u] = a.dst[1][r];
    }
}

// only 'a' .. 'z' lowered by 32, four bytes at a time; bytes of 0x80 and above stay
__device__ __forceinline__ uint32_t fmt_upper4(uint32_t w) {
    const uint32_t x = w & 0x7f7f7f7fu;
    const uint32_t m = (x + 0x1f1f1f1fu) & ~(x + 0x05050505u) & ~w & 0x80808080u;  // 0x80 where 0x61 <= byte <= 0x7a
    return w - (m >> 2);
}
__device__ __forceinline__ uint8_t fmt_upper1(uint32_t c, bool upper) { return (uint8_t)((upper && c >= 'a' && c <= 'z') ? c - 32u : c); }

// The wave copies src[0, len) to dst, a piece of any length, by k_text_copy's scheme: bytes up to the destination's dword
// boundary, whole dwords from the aligned source dwords that hold their bytes (two joined with alignbyte where source and
// destination are not aligned alike), then the last bytes.  The source dwords may reach 3 bytes beyond src + len.
__device__ __forceinline__ void wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t len, bool upper, uint32_t lane) {
    if (!len) return;  // (wave-uniform)
    const uint32_t head = min(len, (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
    if (lane < head) dst[lane] = fmt_upper1(src[lane], upper);
    const uint32_t nd = (len - head) >> 2, sh = (uint32_t)((uintptr_t)(src + head) & 3u);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src + head - sh);
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t d = lane; d < nd; d += 64) {
        const uint32_t w = sh ? __builtin_amdgcn_alignbyte(sw[d + 1], sw[d], sh) : sw[d];
        dw[d] = upper ? fmt_upper4(w) : w;
    }
    const uint32_t done = head + 4u * nd;
    if (lane < len - done) dst[done + lane] = fmt_upper1(src[done + lane], upper);
}

// A wave per emitted record, the bytes of put_record: marker, id, [" |" names joined by ','], '\n', sequence, '\n',
// FASTQ: "+\n", quality, '\n'.
__global__ void __launch_bounds__(256) k_fmt_emit(FmtArgs a) {
    const uint32_t lane = lane_id(), wpb = blockDim.x >> 6;
    for (uint32_t r = blockIdx.x * wpb + (threadIdx.x >> 6); r < a.n; r += gridDim.x * wpb) {
        const uint32_t s = a.len[0][r] ? 0u : 1u;
        if (!a.len[s][r]) continue;  // (wave-uniform)
        uint8_t *dst = a.out[s] + a.dst[s][r];
        const uint32_t id_len = a.id_len[r];
        if (lane == 0) dst[0] = a.fastq ? '@' : '>';
        wave_copy(dst + 1, a.text + a.id_beg[r], id_len, false, lane);
        unsigned long long p = 1ull + id_len;
        const unsigned long long o0 = a.row_off[r], cnt = a.row_off[r + 1u] - o0;
        if (cnt) {
            if (lane == 0) dst[p] = ' ', dst[p + 1] = '|';
            p += 2;
            for (unsigned long long base = 0; base < cnt; base += 64) {
                const unsigned long long j = base + lane;
                const uint32_t leaf = j < cnt ? a.row_leaves[o0 + j] : 0u;
                const uint32_t nlen = j < cnt ? fmt_name_len(a, leaf) : 0u, mine = j < cnt ? nlen + (j ? 1u : 0u) : 0u;
                uint32_t incl = mine;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(incl, d);
                    if ((int)lane >= d) incl += up;
                }
                if (j < cnt) {
                    uint8_t *q = dst + p + (incl - mine);
                    if (j) *q++ = ',';
                    const uint8_t *nm = a.names + a.name_off[leaf];
                    for (uint32_t i = 0; i < nlen; ++i) q[i] = nm[i];
                }
                p += bcast_u32(incl, 63);
            }
        }
        const unsigned long long s0 = a.seq_off[r];
        const uint32_t slen = (uint32_t)(a.seq_off[r + 1u] - s0);
        if (lane == 0) dst[p] = '\n', dst[p + 1 + slen] = '\n';
        wave_copy(dst + p + 1, a.seq + s0, slen, true, lane);
        p += 2ull + slen;
        if (a.fastq) {
            const uint32_t ql = 4u * r + 3u, qs = a.line_start[ql], qlen = fmt_trimmed(a.text, qs, a.line_start[ql + 1u] - 1u);
            if (lane == 0) dst[p] = '+', dst[p + 1] = '\n', dst[p + 2 + qlen] = '\n';
            wave_copy(dst + p + 2, a.text + qs, qlen, false, lane);
        }
    }
}

static uint32_t fmt_grid(const FmtArgs &a, uint64_t n, uint32_t per_block, uint32_t most) {
    const uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>(most, (n + per_block - 1) / per_block));
    return (uint32_t)(a.grid ? std::min<uint64_t>(g, a.grid) : g);
}
void launch_fmt_ids(const FmtArgs &a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_fmt_ids, dim3(fmt_grid(a, a.n, 256, 8192)), dim3(256), 0, st, a);
    if (a.n_whole) {
        uint32_t pad = 1;
        while (pad < a.block) pad <<= 1;
        hipLaunchKernelGGL(k_fmt_blocks, dim3(fmt_grid(a, a.n_whole, 1, 65535)), dim3(std::min(1024u, std::max(64u, pad / 2u))), (size_t)pad * 8, st, a, pad);
    }
}
void launch_fmt_sizes(const FmtArgs &a, bool long_rows, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_fmt_sizes, dim3(fmt_grid(a, a.n, 256, 8192)), dim3(256), 0, st, a);
    if (long_rows) hipLaunchKernelGGL(k_fmt_sizes_long, dim3(fmt_grid(a, a.n, 4, 1024)), dim3(256), 0, st, a);
}
void launch_fmt_bounds(const FmtArgs &a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_fmt_bounds, dim3(fmt_grid(a, (uint64_t)a.n_whole + 2, 256, 8192)), dim3(256), 0, st, a);
}
void launch_fmt_emit(const FmtArgs &a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_fmt_emit, dim3(fmt_grid(a, a.n, 4, 16384)), dim3(256), 0, st, a);
}

}  // namespace pfq
