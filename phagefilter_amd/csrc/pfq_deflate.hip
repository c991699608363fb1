// pfq_bgzf_deflate / pfq_text_format_gz: text cut into members of blocked gzip (BGZF) and deflated on the device, one workgroup a
// member ("Device-side deflate").  The rules — which match a position gets, which the parse takes, how the codes are
// built — are pfq_deflate_core.h, the text the host program tools/deflate_host.cpp compiles too; this file is how 256 lanes follow
// them so that the bytes are the host program's: nothing here depends on the order in which lanes run.
//
//   pass 1, a tile of 256 positions at a time: a lane a position looks up last[hash], measures its two candidates a dword at a time
//     and makes its choice; pointer doubling over "where the parse goes from here" marks the positions the greedy parse visits;
//     those write their token to the workgroup's slab in global memory and count it (LDS atomics); then the tile's positions enter
//     last[] by atomic max.
//   thread 0: the core's plan() — code lengths, codes, the header's run symbols — in LDS.
//   pass 2: the text's LDS becomes the bit buffer; a lane a position again, its token's bits OR-ed in at the offset an exclusive
//     scan of the bit counts gives; the buffer leaves for the member's slot as dwords.
// The tokens are kept (4 bytes a position, a slab of BGZF_TOKENS words a workgroup, written and re-read by the same lane) and
// not made twice: the second pass then needs neither the text nor last[], and the text's 64 KiB can hold the bits.
#include <hip/hip_runtime.h>

#include "pfq_deflate_core.h"
#include "pfq_kernels.h"

namespace pfq {
namespace {

namespace pd = pfq_deflate;
namespace pi = pfq_inflate;

constexpr uint32_t DF_THREADS = pd::TILE, DF_WAVES = DF_THREADS / 64, DF_ROUNDS = 8;
static_assert(DF_THREADS == 256 && (1u << DF_ROUNDS) == pd::TILE, "a lane a position of the tile; doubling rounds that cover it");
static_assert(BGZF_SLOT == pd::SLOT && BGZF_TOKENS == pd::MEMBER_TEXT, "pfq_kernels.h and the core agree");

struct DfLds {
    // the member's text from byte (text_begin & 15) on, up to 15 + 65280 bytes, read up to 7 bytes further; later the member itself
    uint8_t buf[pd::SLOT];
    uint32_t last[1u << pd::HASH_BITS];  // position + 1 of the last 4-gram with this hash below the tile, 0: none
    pd::Work work;
    uint32_t crc_table[256];
    uint32_t jump[DF_THREADS], mark[DF_THREADS];
    uint32_t wave_bits[DF_WAVES];
    uint32_t crc, block_bits, header_end;
    uint8_t fixed[32];  // of a stored member: header 18, block head 5, -, trailer 8 at 24
};
static_assert(sizeof(DfLds) <= 160 * 1024, "one workgroup a CU");

// text[a .. a + 4) of the LDS image, little-endian, from the two aligned dwords that hold it
__device__ __forceinline__ uint32_t ld4(const uint32_t *words, uint32_t a) {
    return __builtin_amdgcn_alignbyte(words[(a >> 2) + 1], words[a >> 2], a & 3u);
}
// The common prefix of the text at a and at b, at most `most` (a + most <= the text's end).
__device__ __forceinline__ uint32_t prefix(const uint32_t *words, uint32_t a, uint32_t b, uint32_t most) {
    uint32_t k = 0;
    while (k < most) {
        const uint32_t x = ld4(words, a + k) ^ ld4(words, b + k);
        if (x) {
            k += (uint32_t)(__ffs((int)x) - 1) >> 3;
            break;
        }
        k += 4;
    }
    return k < most ? k : most;
}

__global__ __launch_bounds__(DF_THREADS) void k_bgzf_deflate(const uint8_t *__restrict__ text, const BgzfMember *__restrict__ members, uint64_t n_members,
                                                             uint32_t *__restrict__ tokens, uint8_t *__restrict__ slots, uint32_t *__restrict__ sizes) {
    __shared__ __attribute__((aligned(16))) DfLds s;
    const uint32_t tid = threadIdx.x;
    s.crc_table[tid] = pi::crc_table_entry(tid);
    uint32_t *my_tokens = tokens + (size_t)blockIdx.x * BGZF_TOKENS;
    uint32_t *words = reinterpret_cast<uint32_t *>(s.buf);
    for (uint64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
        __syncthreads();  // (the last member has left the buffer; the CRC table stands)
        const BgzfMember mem = members[m];
        const uint32_t n = mem.text_len <= pd::MEMBER_TEXT ? mem.text_len : pd::MEMBER_TEXT;
        const uint32_t sh = (uint32_t)(mem.text_begin & 15u);
        {  // the text: aligned 16-byte loads (the source buffer begins aligned and ends 16 bytes late)
            const uint4 *src = reinterpret_cast<const uint4 *>(text + (mem.text_begin - sh));
            uint4 *dst = reinterpret_cast<uint4 *>(s.buf);
            const uint32_t n16 = (sh + n + 15) / 16;
            for (uint32_t i = tid; i < n16; i += DF_THREADS) dst[i] = src[i];
        }
        for (uint32_t i = tid; i < (1u << pd::HASH_BITS); i += DF_THREADS) s.last[i] = 0;
        for (uint32_t i = tid; i < pd::N_LIT + 2; i += DF_THREADS) s.work.lit_count[i] = 0;
        if (tid < pd::N_DIST + 2) s.work.dist_count[tid] = 0;
        __syncthreads();
        if (tid < 64) {  // the CRC of the text, by the first wave (no barrier inside: the others go on to the tiles)
            const uint8_t *win = s.buf + sh;
            uint32_t crc = pi::crc_piece(win, s.crc_table, n, tid);
            for (uint32_t d = 1; d < 64; d <<= 1) crc ^= __shfl_xor(crc, d, 64);
            if (tid == 0) s.crc = ~crc;
        }
        // ---- pass 1
        uint32_t entry = 0;  // where the parse enters the tile, or a position beyond it
        for (uint32_t t0 = 0; t0 < n; t0 += pd::TILE) {
            const uint32_t p = t0 + tid, t_end = t0 + pd::TILE;
            uint32_t choice = 0, h = 0;
            const bool hashed = p + 4 <= n;
            if (p < n) {
                const uint32_t most = n - p < pd::MAX_MATCH ? n - p : pd::MAX_MATCH;
                uint32_t len_a = 0, dist_a = 0, len_b = 0;
                if (hashed) {
                    h = pd::hash4(ld4(words, sh + p));
                    const uint32_t q1 = s.last[h];
                    if (q1 && p - (q1 - 1) <= pd::MAX_DIST) dist_a = p - (q1 - 1), len_a = prefix(words, sh + p, sh + q1 - 1, most);
                }
                if (p) len_b = prefix(words, sh + p, sh + p - 1, most);
                choice = pd::choose(len_a, dist_a, len_b);
            }
            s.jump[tid] = p < n ? p + pd::choice_len(choice) : t_end;
            s.mark[tid] = p == entry;
            __syncthreads();
            // after round r the positions up to 2^(r + 1) - 1 steps behind `entry` are marked, and jump is 2^(r + 1) steps
            for (uint32_t r = 0; r < DF_ROUNDS; r++) {
                const uint32_t mk = s.mark[tid], j = s.jump[tid], jj = j < t_end ? s.jump[j - t0] : j;
                __syncthreads();
                if (mk && j < t_end) s.mark[j - t0] = 1;
                s.jump[tid] = jj;
                __syncthreads();
            }
            const uint32_t next_entry = entry < t_end ? s.jump[entry - t0] : entry;
            if (p < n) {
                uint32_t tok = 0;
                if (s.mark[tid]) {
                    tok = choice ? choice : pd::TOK_LIT | s.buf[sh + p];
                    if (choice) {
                        atomicAdd(&s.work.lit_count[pd::length_sym(pd::choice_len(choice)).sym], 1u);
                        atomicAdd(&s.work.dist_count[pd::dist_sym((choice & 0x7fffu) + 1).sym], 1u);
                    } else {
                        atomicAdd(&s.work.lit_count[tok & 0xffu], 1u);
                    }
                }
                my_tokens[p] = tok;
            }
            if (hashed) atomicMax(&s.last[h], p + 1);
            __syncthreads();  // (last[] is complete for the next tile; jump and mark have been read)
            entry = next_entry;
        }
        if (tid == 0) {
            s.work.lit_count[pd::EOB]++;
            s.block_bits = pd::plan(s.work);
        }
        __syncthreads();
        const uint32_t block_bytes = (s.block_bits + 7) / 8;
        const bool stored = block_bytes >= n;
        const uint32_t payload = stored ? n + pd::STORED_HEAD : block_bytes, size = pd::HEADER + payload + pd::TRAILER;
        uint32_t *slot = reinterpret_cast<uint32_t *>(slots + m * BGZF_SLOT);
        if (stored) {  // (workgroup-uniform)
            if (tid == 0) {
                pd::put_gzip_header(s.fixed, size);
                uint8_t *b = s.fixed + pd::HEADER;
                b[0] = 1;
                b[1] = (uint8_t)n, b[2] = (uint8_t)(n >> 8), b[3] = (uint8_t)~n, b[4] = (uint8_t)(~n >> 8);
                pd::put_le32(s.fixed + 24, s.crc);
                pd::put_le32(s.fixed + 28, n);
            }
            __syncthreads();
            const uint32_t head = pd::HEADER + pd::STORED_HEAD;
            for (uint32_t d = tid; d < (size + 3) / 4; d += DF_THREADS) {
                uint32_t w = 0;
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t j = 4 * d + k;
                    const uint32_t byte = j < head ? s.fixed[j] : j < head + n ? s.buf[sh + j - head] : j < size ? s.fixed[24 + (j - head - n)] : 0u;
                    w |= byte << (8 * k);
                }
                slot[d] = w;
            }
        } else {
            // ---- pass 2
            for (uint32_t i = tid; i < pd::SLOT / 16; i += DF_THREADS) reinterpret_cast<uint4 *>(s.buf)[i] = make_uint4(0, 0, 0, 0);
            __syncthreads();
            if (tid == 0) {
                pd::put_gzip_header(s.buf, size);
                pd::BitWriter b{s.buf, pd::HEADER * 8};
                pd::put_block_header(b, s.work);
                s.header_end = b.bit;
            }
            __syncthreads();
            uint32_t base = s.header_end;
            for (uint32_t t0 = 0; t0 < n; t0 += pd::TILE) {
                const uint32_t p = t0 + tid;
                const uint32_t tok = p < n ? my_tokens[p] : 0u;
                uint32_t nb = 0;
                uint64_t v = 0;
                if (tok) v = pd::token_bits(s.work, tok, &nb);
                uint32_t incl = nb;
                for (uint32_t d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(incl, d, 64);
                    if ((tid & 63u) >= d) incl += up;
                }
                if ((tid & 63u) == 63u) s.wave_bits[tid >> 6] = incl;
                __syncthreads();
                uint32_t before = base, total = 0;
                for (uint32_t w = 0; w < DF_WAVES; w++) {
                    if (w < (tid >> 6)) before += s.wave_bits[w];
                    total += s.wave_bits[w];
                }
                if (nb) {
                    const uint32_t at = before + incl - nb, sft = at & 31u;
                    const uint64_t lo = v << sft;
                    const uint32_t hi = sft ? (uint32_t)(v >> (64 - sft)) : 0u;
                    atomicOr(&words[at >> 5], (uint32_t)lo);
                    if (lo >> 32) atomicOr(&words[(at >> 5) + 1], (uint32_t)(lo >> 32));
                    if (hi) atomicOr(&words[(at >> 5) + 2], hi);
                }
                base += total;
                __syncthreads();  // (wave_bits are read; the tile's bits are in)
            }
            if (tid == 0) {
                pd::BitWriter b{s.buf, base};
                b.code(s.work.lit_code[pd::EOB]);
                pd::put_le32(s.buf + pd::HEADER + payload, s.crc);
                pd::put_le32(s.buf + pd::HEADER + payload + 4, n);
            }
            __syncthreads();
            for (uint32_t d = tid; d < (size + 3) / 4; d += DF_THREADS) slot[d] = words[d];
        }
        if (tid == 0) sizes[m] = size;
    }
}

// Member m's bytes from its slot to gz + off[m], a workgroup a member: bytes up to the destination's dword boundary, whole dwords
// from the aligned source dwords that hold their bytes (two joined with alignbyte), then the last bytes.  The source dwords may
// reach 3 bytes beyond the member, inside its slot.
__global__ __launch_bounds__(256) void k_bgzf_gather(const uint8_t *__restrict__ slots, const unsigned long long *__restrict__ off, uint64_t n_members,
                                                     uint8_t *__restrict__ gz) {
    const uint32_t tid = threadIdx.x;
    for (uint64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
        const uint8_t *src = slots + m * BGZF_SLOT;
        uint8_t *dst = gz + off[m];
        const uint32_t len = (uint32_t)(off[m + 1] - off[m]);
        if (!len || len > BGZF_SLOT - 4) continue;  // (workgroup-uniform; a size no member has)
        uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
        if (head > len) head = len;
        if (tid < head) dst[tid] = src[tid];
        const uint32_t nd = (len - head) >> 2, sh = head & 3u;  // (a slot begins aligned)
        const uint32_t *sw = reinterpret_cast<const uint32_t *>(src + head - sh);
        uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
        for (uint32_t d = tid; d < nd; d += 256) dw[d] = sh ? __builtin_amdgcn_alignbyte(sw[d + 1], sw[d], sh) : sw[d];
        const uint32_t done = head + 4u * nd;
        if (tid < len - done) dst[done + tid] = src[done + tid];
    }
}

}  // namespace

void launch_bgzf_deflate(const uint8_t *d_text, const BgzfMember *d_members, uint64_t n_members, uint32_t *d_tokens, uint8_t *d_slots, uint32_t *d_sizes,
                         uint32_t blocks, hipStream_t st) {
    if (!n_members) return;
    const uint32_t grid = (uint32_t)(n_members < blocks ? n_members : blocks);
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(grid ? grid : 1), dim3(DF_THREADS), 0, st, d_text, d_members, n_members, d_tokens, d_slots, d_sizes);
}

void launch_bgzf_gather(const uint8_t *d_slots, const unsigned long long *d_off, uint64_t n_members, uint8_t *d_gz, hipStream_t st) {
    if (!n_members) return;
    const uint32_t grid = (uint32_t)(n_members < 4096 ? n_members : 4096);
    hipLaunchKernelGGL(k_bgzf_gather, dim3(grid), dim3(256), 0, st, d_slots, d_off, n_members, d_gz);
}

}  // namespace pfq
