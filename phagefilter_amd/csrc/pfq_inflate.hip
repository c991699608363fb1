// pfq_text_inflate: the members of a blocked gzip (BGZF) chunk inflated on the device, one wave a member (DESIGN.md §5,
// "Device-side inflate").  The decoder is pfq_inflate_core.h, the text the host sanitizer program compiles too; this file gives
// it an environment in LDS: the member's whole output window, its decode tables, one staged piece of the compressed bytes and
// the CRC table.  The symbol loop is wave-uniform (every lane decodes the same bits); the lanes share the work where bytes move:
// staging, back-references, stored blocks, the window's way to the staging buffer and the CRC.
#include <hip/hip_runtime.h>

#include "pfq_inflate_core.h"
#include "pfq_kernels.h"

namespace pfq {
namespace {

namespace pi = pfq_inflate;

constexpr uint32_t GZ_WAVE = 64;
constexpr uint32_t GZ_LDS_WINDOW = 0, GZ_LDS_STAGE = pi::TEXT_MAX, GZ_LDS_CRC = GZ_LDS_STAGE + GZ_STAGE, GZ_LDS_TABLES = GZ_LDS_CRC + 1024,
                   GZ_LDS_BYTES = (GZ_LDS_TABLES + pi::TABLES_BYTES + 15) / 16 * 16;
static_assert(GZ_LDS_BYTES <= 80 * 1024, "two workgroups a CU: half of 160 KiB each");

struct LdsEnv {
    uint8_t *win, *stage;
    const uint8_t *gz;   // the chunk; 16-byte aligned, allocated up to a multiple of GZ_STAGE beyond every payload
    uint64_t pay_begin;  // of this member, in gz
    uint64_t staged;     // which piece of gz the stage holds (its first byte's offset), ~0: none
    uint32_t lane;
    // pos is wave-uniform, so is the branch; the payload bytes are read in ascending order, so a piece is staged once a member
    __device__ uint32_t in(uint32_t pos) {
        const uint64_t a = pay_begin + pos, piece = a & ~(uint64_t)(GZ_STAGE - 1);
        if (piece != staged) {
            __syncthreads();  // (what was read from the stage has been read)
            const uint4 *src = reinterpret_cast<const uint4 *>(gz + piece);
            uint4 *dst = reinterpret_cast<uint4 *>(stage);
            for (uint32_t i = lane; i < GZ_STAGE / 16; i += GZ_WAVE) dst[i] = src[i];
            __syncthreads();
            staged = piece;
        }
        return stage[a & (GZ_STAGE - 1)];
    }
    __device__ void put(uint32_t at, uint32_t byte) { win[at] = (uint8_t)byte; }  // every lane, the same byte
    // The bytes of a back-reference all lie below `at` once the period is folded in, so the lanes copy without order.
    __device__ void copy(uint32_t at, uint32_t dist, uint32_t n) {
        const uint32_t src = at - dist;
        if (dist >= n)
            for (uint32_t i = lane; i < n; i += GZ_WAVE) win[at + i] = win[src + i];
        else
            for (uint32_t i = lane; i < n; i += GZ_WAVE) win[at + i] = win[src + i % dist];
        __syncthreads();
    }
    __device__ void copy_in(uint32_t at, uint32_t pos, uint32_t n) {
        const uint8_t *src = gz + pay_begin + pos;
        for (uint32_t i = lane; i < n; i += GZ_WAVE) win[at + i] = src[i];
        __syncthreads();
    }
};

__global__ __launch_bounds__(GZ_WAVE) void k_gz_inflate(const uint8_t *__restrict__ gz, const GzMember *__restrict__ members, uint64_t n_members,
                                                         uint8_t *__restrict__ text, uint32_t *__restrict__ result) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[GZ_LDS_BYTES];
    const uint32_t lane = threadIdx.x;
    uint32_t *crc_table = reinterpret_cast<uint32_t *>(lds + GZ_LDS_CRC);
    for (uint32_t i = lane; i < 256; i += GZ_WAVE) crc_table[i] = pi::crc_table_entry(i);
    const pi::Tables T = pi::tables_at(lds + GZ_LDS_TABLES);
    LdsEnv env{lds + GZ_LDS_WINDOW, lds + GZ_LDS_STAGE, gz, 0, ~0ull, lane};
    for (uint64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
        __syncthreads();  // (the last member's window has been stored; the CRC table stands)
        const GzMember mem = members[m];
        env.pay_begin = mem.pay_begin;
        const uint32_t n = mem.isize <= pi::TEXT_MAX ? mem.isize : 0u;
        const uint32_t status = mem.isize <= pi::TEXT_MAX ? pi::inflate_member(env, T, mem.pay_len, n, nullptr) : (uint32_t)pi::ST_LENGTH;
        __syncthreads();
        uint32_t crc = 0;
        if (status == pi::ST_OK) {
            const uint8_t *win = env.win;
            crc = pi::crc_piece(win, crc_table, n, lane);
            for (uint32_t d = 1; d < GZ_WAVE; d <<= 1) crc ^= __shfl_xor(crc, d, GZ_WAVE);
            crc = ~crc;
            // the window to text[text_begin, text_begin + n): bytes up to the first dword boundary, dwords, bytes
            uint8_t *dst = text + mem.text_begin;
            uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
            if (head > n) head = n;
            const uint32_t n_dw = (n - head) / 4, tail = head + 4 * n_dw;
            if (lane < head) dst[lane] = win[lane];
            uint32_t *dst_dw = reinterpret_cast<uint32_t *>(dst + head);
            for (uint32_t j = lane; j < n_dw; j += GZ_WAVE) {
                const uint32_t k = head + 4 * j;
                dst_dw[j] = (uint32_t)win[k] | (uint32_t)win[k + 1] << 8 | (uint32_t)win[k + 2] << 16 | (uint32_t)win[k + 3] << 24;
            }
            if (tail + lane < n) dst[tail + lane] = win[tail + lane];
        }
        if (lane == 0) {
            result[2 * m] = status;
            result[2 * m + 1] = crc;
        }
    }
}

}  // namespace

void launch_gz_inflate(const uint8_t *d_gz, const GzMember *d_members, uint64_t n_members, uint8_t *d_text, uint32_t *d_result, uint32_t blocks,
                       hipStream_t st) {
    if (!n_members) return;
    const uint32_t grid = (uint32_t)(n_members < blocks ? n_members : blocks);
    hipLaunchKernelGGL(k_gz_inflate, dim3(grid ? grid : 1), dim3(GZ_WAVE), 0, st, d_gz, d_members, n_members, d_text, d_result);
}

}  // namespace pfq
