// pfq_text.hip — pfq_text_parse: plain FASTA / FASTQ text parsed on the device (DESIGN.md "Device-side parsing").  One
// line-parallel pipeline serves both formats; nothing of pfq_kernels.hip is involved beyond the scan behind launch_scan_u32.
//
//   k_text_count -> scan -> k_text_lines          newline masks, 16 bytes a lane; the start of every line
//   k_text_roles                                  per line: its role, its trimmed length if it is a sequence line; FASTQ:
//                                                 the first record that is not plain (one atomicMin, only on failure)
//   scan of the lengths                           every line's destination in the CSR
//   FASTA: scan of the header flags -> k_text_rec_lines   the header line of every record
//   k_text_finish                                 one thread: records taken, consumed, stop, bases (read back in one copy)
//   k_text_offsets | k_text_copy                  the CSR offsets (and rec_begin); the sequence lines moved to their places
//
// Every index is 32 bits wide: the host refuses texts of 2^31 bytes or more.  The text buffer is 16-byte aligned and holds 16
// bytes beyond the text rounded up to 16, so aligned 16-byte loads and the dword over-reads of the copy stay inside it.
#include "pfq_kernels.h"

#include <algorithm>

namespace pfq {

constexpr uint32_t TEXT_THREADS = 256, TEXT_STEP = TEXT_THREADS * 16;  // bytes a block looks at per step, 16 a lane

// bit j: byte pos + j is '\n' (pos: a multiple of 16; bytes at or beyond len never count)
__device__ __forceinline__ uint32_t newline_mask(const uint8_t *__restrict__ text, uint32_t pos, uint32_t len) {
    if (pos >= len) return 0u;
    const uint4 v = *reinterpret_cast<const uint4 *>(text + pos);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t x = w[j] ^ 0x0a0a0a0au;  // a zero byte where the newlines are
        const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);  // 0x80 in exactly those bytes
        mask |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4u * j);
    }
    const uint32_t left = len - pos;
    return left >= 16u ? mask : mask & ((1u << left) - 1u);
}

// Block b looks at text[b * tile, (b + 1) * tile): blk_cnt[b] = its newlines.
__global__ void __launch_bounds__(TEXT_THREADS) k_text_count(const uint8_t *__restrict__ text, uint32_t len, uint32_t tile, uint32_t *__restrict__ blk_cnt) {
    __shared__ uint32_t s_w[TEXT_THREADS / 64];
    const uint32_t base = blockIdx.x * tile;
    uint32_t c = 0;
    for (uint32_t o = threadIdx.x * 16u; o < tile; o += TEXT_STEP) c += __popc(newline_mask(text, base + o, len));
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if (lane_id() == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < TEXT_THREADS / 64; ++w) t += s_w[w];
        blk_cnt[blockIdx.x] = t;
    }
}

// line_start[0] = 0 and line_start[j + 1] = the byte behind the j-th newline: line i is text[line_start[i], line_start[i + 1] - 1).
// unterminated (the last run counts as a line, PFQ_TEXT_FINAL): line_start[n_lines] = len + 1, as if a newline ended the text.
__global__ void __launch_bounds__(TEXT_THREADS) k_text_lines(const uint8_t *__restrict__ text, uint32_t len, uint32_t tile,
                                                             const unsigned long long *__restrict__ blk_off, uint32_t *__restrict__ line_start,
                                                             uint32_t n_lines, uint32_t unterminated) {
    __shared__ uint32_t s_w[TEXT_THREADS / 64];
    const uint32_t base = blockIdx.x * tile, lane = lane_id(), wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        line_start[0] = 0;
        if (unterminated) line_start[n_lines] = len + 1u;
    }
    uint32_t run = (uint32_t)blk_off[blockIdx.x];  // newlines before this step
    for (uint32_t o0 = 0; o0 < tile; o0 += TEXT_STEP) {  // (uniform: every thread meets the barriers)
        const uint32_t o = o0 + threadIdx.x * 16u, pos = base + o;
        uint32_t m = o < tile ? newline_mask(text, pos, len) : 0u;
        const uint32_t c = __popc(m);
        uint32_t incl = c;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if ((int)lane >= d) incl += up;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t rank = run + incl - c, all = 0;
        for (uint32_t w = 0; w < TEXT_THREADS / 64; ++w) {
            if (w < wave) rank += s_w[w];
            all += s_w[w];
        }
        while (m) {
            const uint32_t j = __ffs(m) - 1u;
            m &= m - 1u;
            line_start[++rank] = pos + j + 1u;
        }
        run += all;
        __syncthreads();
    }
}

__device__ __forceinline__ bool text_blank(uint32_t c) { return c == ' ' || (c >= 9u && c <= 13u); }  // ' ', \t \n \v \f \r
__device__ __forceinline__ uint32_t trimmed_len(const uint8_t *__restrict__ text, uint32_t s, uint32_t e) {
    while (e > s && text_blank(text[e - 1u])) --e;
    return e - s;
}

// Per line: line_len = the trimmed length of a sequence line, 0 of any other.  FASTQ: line i has role i mod 4 and the lines
// below n_check (whole records) are tested for "plain"; FASTA: is_header says which lines begin with '>'.
__global__ void __launch_bounds__(256) k_text_roles(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_start, uint32_t n_lines,
                                                    uint32_t n_check, int fastq, uint32_t *__restrict__ line_len, uint32_t *__restrict__ is_header,
                                                    uint32_t *__restrict__ first_bad) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += gridDim.x * blockDim.x) {
        const uint32_t s = line_start[i], e = line_start[i + 1u] - 1u;
        const uint32_t first = s < e ? text[s] : 0x100u;  // (an empty line begins with nothing)
        if (fastq) {
            const uint32_t role = i & 3u;
            const uint32_t tl = (role == 1u || role == 3u) ? trimmed_len(text, s, e) : 0u;
            line_len[i] = role == 1u ? tl : 0u;
            const bool bad = role == 0u ? first != '@' : role == 1u ? first == '+' : role == 2u ? first != '+' : tl == 0u;
            if (bad && i < n_check) atomicMin(first_bad, i >> 2);
        } else {
            const bool hdr = first == '>';
            is_header[i] = hdr ? 1u : 0u;
            line_len[i] = hdr ? 0u : trimmed_len(text, s, e);
        }
    }
}

__global__ void __launch_bounds__(256) k_text_rec_lines(const uint32_t *__restrict__ is_header, const unsigned long long *__restrict__ rec_idx,
                                                        uint32_t n_lines, uint32_t *__restrict__ rec_line) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += gridDim.x * blockDim.x)
        if (is_header[i]) rec_line[rec_idx[i]] = i;
}

// The begin of line i; behind the considered lines, where they end (an unterminated last line ends with the text).
__device__ __forceinline__ uint32_t line_begin(const TextArgs &a, uint32_t i) { return i < a.n_lines ? a.line_start[i] : min(a.line_start[a.n_lines], a.len); }

// One thread: the rules of pfq.h "pfq_text_parse" from what the kernels before left.  The begins of the records ascend, so
// the first record at or beyond the limit is found by bisection.
__global__ void k_text_finish(TextArgs a) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t taken, lines_taken, stop;
    uint64_t consumed;
    if (a.fastq) {
        const uint32_t n_full = a.n_lines >> 2;
        uint32_t lo = 0, hi = n_full + 1u;  // the first r <= n_full whose begin is at or beyond the limit (none: n_full + 1)
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if ((uint64_t)line_begin(a, 4u * mid) >= a.limit) hi = mid;
            else lo = mid + 1u;
        }
        taken = min(min(*a.first_bad, n_full), lo);
        lines_taken = 4u * taken;
        const uint32_t b = line_begin(a, lines_taken);
        consumed = b;
        if (b == a.len) stop = PFQ_TEXT_STOP_END;
        else if (lines_taken == a.n_lines) stop = PFQ_TEXT_STOP_MORE;
        else if ((uint64_t)b >= a.limit) stop = PFQ_TEXT_STOP_LIMIT;
        else if (a.n_lines - lines_taken < 4u) stop = a.final ? PFQ_TEXT_STOP_SLOW : PFQ_TEXT_STOP_MORE;
        else stop = PFQ_TEXT_STOP_SLOW;
    } else {  // (line 0 is a header: the host answers every other text itself)
        const uint32_t n_hdr = (uint32_t)a.rec_idx[a.n_lines], n_complete = a.final ? n_hdr : n_hdr - 1u;
        uint32_t lo = 0, hi = n_hdr;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if ((uint64_t)a.line_start[a.rec_line[mid]] >= a.limit) hi = mid;
            else lo = mid + 1u;
        }
        taken = min(lo, n_complete);
        if (taken == n_hdr) {
            lines_taken = a.n_lines;
            consumed = a.len;
            stop = PFQ_TEXT_STOP_END;
        } else {
            lines_taken = a.rec_line[taken];
            consumed = a.line_start[lines_taken];
            stop = consumed >= a.limit ? PFQ_TEXT_STOP_LIMIT : PFQ_TEXT_STOP_MORE;
        }
    }
    a.result[TEXT_RES_RECORDS] = taken;
    a.result[TEXT_RES_CONSUMED] = consumed;
    a.result[TEXT_RES_BASES] = a.dst[lines_taken];
    a.result[TEXT_RES_STOP] = stop;
    a.result[TEXT_RES_LINES] = lines_taken;
}

// csr_off[j] = where record j's bases begin, j <= taken; rec_begin[j] = its header line's byte offset, then consumed.
__global__ void __launch_bounds__(256) k_text_offsets(TextArgs a, uint64_t *__restrict__ csr_off, uint64_t *__restrict__ rec_begin) {
    const uint32_t taken = (uint32_t)a.result[TEXT_RES_RECORDS], lines_taken = (uint32_t)a.result[TEXT_RES_LINES];
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j <= taken; j += gridDim.x * blockDim.x) {
        const uint32_t line = j == taken ? lines_taken : a.fastq ? 4u * j : a.rec_line[j];
        csr_off[j] = a.dst[line];
        if (rec_begin) rec_begin[j] = j == taken ? a.result[TEXT_RES_CONSUMED] : (uint64_t)a.line_start[line];
    }
}

// One wave per sequence line of the records taken (FASTQ: line 4r + 1; FASTA: every line, headers have length 0), whatever its
// length: the lanes loop over it.  As k_frame_copy: the destination is brought to a dword boundary byte by byte, whole dwords
// are stored from the aligned source dwords that hold their bytes (two joined with alignbyte where the two are not aligned
// alike), then the last bytes.  The source dwords lie inside the text buffer: it begins aligned and ends 16 bytes late.
__global__ void __launch_bounds__(256) k_text_copy(TextArgs a, uint8_t *__restrict__ out) {
    const uint32_t lane = lane_id();
    const uint32_t n_units = a.fastq ? (uint32_t)a.result[TEXT_RES_RECORDS] : (uint32_t)a.result[TEXT_RES_LINES];
    for (uint32_t u = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); u < n_units; u += gridDim.x * (blockDim.x >> 6)) {
        const uint32_t line = a.fastq ? 4u * u + 1u : u;
        const uint32_t len = a.line_len[line];
        if (!len) continue;  // (wave-uniform)
        const uint8_t *src = a.text + a.line_start[line];
        uint8_t *dst = out + a.dst[line];
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

void launch_text_count(const uint8_t *d_text, uint32_t len, uint32_t tile, uint32_t *d_blk_cnt, hipStream_t st) {
    const uint32_t n_tiles = (len + tile - 1) / tile;
    if (n_tiles) hipLaunchKernelGGL(k_text_count, dim3(n_tiles), dim3(TEXT_THREADS), 0, st, d_text, len, tile, d_blk_cnt);
}
void launch_text_lines(const uint8_t *d_text, uint32_t len, uint32_t tile, const unsigned long long *d_blk_off, uint32_t *d_line_start, uint32_t n_lines,
                       bool unterminated, hipStream_t st) {
    const uint32_t n_tiles = (len + tile - 1) / tile;
    if (n_tiles) hipLaunchKernelGGL(k_text_lines, dim3(n_tiles), dim3(TEXT_THREADS), 0, st, d_text, len, tile, d_blk_off, d_line_start, n_lines, unterminated ? 1u : 0u);
}
static uint32_t text_grid(uint32_t n, uint32_t per_block) { return std::max(1u, std::min(8192u, (n + per_block - 1) / per_block)); }
void launch_text_roles(const TextArgs &a, uint32_t *d_is_header, hipStream_t st) {
    const uint32_t n_check = a.fastq ? (a.n_lines & ~3u) : 0u;
    hipLaunchKernelGGL(k_text_roles, dim3(text_grid(a.n_lines, 256)), dim3(256), 0, st, a.text, a.line_start, a.n_lines, n_check, a.fastq, a.line_len, d_is_header,
                       a.first_bad);
}
void launch_text_rec_lines(const uint32_t *d_is_header, const unsigned long long *d_rec_idx, uint32_t n_lines, uint32_t *d_rec_line, hipStream_t st) {
    hipLaunchKernelGGL(k_text_rec_lines, dim3(text_grid(n_lines, 256)), dim3(256), 0, st, d_is_header, d_rec_idx, n_lines, d_rec_line);
}
void launch_text_finish(const TextArgs &a, uint8_t *d_csr_seq, uint64_t *d_csr_off, uint64_t *d_rec_begin, hipStream_t st) {
    hipLaunchKernelGGL(k_text_finish, dim3(1), dim3(64), 0, st, a);
    const uint32_t max_records = a.fastq ? a.n_lines >> 2 : a.n_lines;
    hipLaunchKernelGGL(k_text_offsets, dim3(text_grid(max_records + 1u, 256)), dim3(256), 0, st, a, d_csr_off, d_rec_begin);
    hipLaunchKernelGGL(k_text_copy, dim3(text_grid(max_records, 4)), dim3(256), 0, st, a, d_csr_seq);
}

}  // namespace pfq
