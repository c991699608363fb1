// The deflate core of libpfq (phagefilter_amd/csrc/pfq_deflate_core.h) on the host: the very text the device kernel compiles, one
// thread, over heap buffers of exactly the sizes the core is promised, so a read or write one byte outside is a sanitizer report.
// Build: g++ -std=c++17 -g -fsanitize=address,undefined -I phagefilter_amd/csrc tools/deflate_host.cpp -lz -o deflate_host
// Use:   deflate_host [--check] IN OUT [cut ..]
// IN is cut at the given ascending offsets into pieces, every piece into members of 65280 text bytes (the last shorter, an empty
// piece none), and OUT receives the members back to back, without an end marker.  One line a member:
//   <index> <piece> <text begin> <text bytes> <member bytes>
// then "members <n> bytes <total>".  --check also inflates every member with zlib and with pfq_inflate_core.h and compares the
// text, CRC-32, ISIZE and BSIZE; a difference is a message on stderr and status 1.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pfq_deflate_core.h"

namespace pd = pfq_deflate;
namespace pi = pfq_inflate;

struct HostEnv {
    const uint8_t *pay;
    uint8_t *win;
    uint32_t in(uint32_t pos) { return pay[pos]; }
    void put(uint32_t at, uint32_t byte) { win[at] = (uint8_t)byte; }
    void copy(uint32_t at, uint32_t dist, uint32_t n) {
        for (uint32_t i = 0; i < n; i++) win[at + i] = win[at + i - dist];
    }
    void copy_in(uint32_t at, uint32_t pos, uint32_t n) {
        for (uint32_t i = 0; i < n; i++) win[at + i] = pay[pos + i];
    }
};

static bool check_member(const uint8_t *member, uint32_t size, const uint8_t *text, uint32_t n, const uint32_t *crc_table) {
    pi::Member m{};
    if (pi::walk_member(member, size, &m) != pi::WALK_TAKEN || m.size != size || m.header != pd::HEADER) return fprintf(stderr, "header walk\n"), false;
    if (m.isize != n || m.crc != (uint32_t)crc32(0, text, n)) return fprintf(stderr, "ISIZE or CRC\n"), false;
    const uint32_t pay_len = size - pd::HEADER - pd::TRAILER;
    if (pay_len > n + pd::STORED_HEAD) return fprintf(stderr, "payload of %u bytes for %u of text\n", pay_len, n), false;
    std::vector<uint8_t> out(n + 1);
    z_stream z{};
    if (inflateInit2(&z, -15) != Z_OK) return false;
    z.next_in = const_cast<uint8_t *>(member + pd::HEADER);
    z.avail_in = pay_len;
    z.next_out = out.data();
    z.avail_out = n + 1;
    const int rc = inflate(&z, Z_FINISH);
    const bool z_ok = rc == Z_STREAM_END && z.total_out == n && z.avail_in == 0 && !memcmp(out.data(), text, n);
    inflateEnd(&z);
    if (!z_ok) return fprintf(stderr, "zlib: rc %d, %lu bytes out, %u in left\n", rc, z.total_out, z.avail_in), false;
    uint8_t *pay = (uint8_t *)malloc(pay_len), *win = (uint8_t *)malloc(n ? n : 1);
    memcpy(pay, member + pd::HEADER, pay_len);
    std::vector<uint8_t> table_mem(pi::TABLES_BYTES + 2);
    HostEnv env{pay, win};
    const uint32_t status = pi::inflate_member(env, pi::tables_at(table_mem.data()), pay_len, n, nullptr);
    uint32_t crc = 0;
    for (uint32_t lane = 0; lane < pi::CRC_PIECES; lane++) crc ^= pi::crc_piece(win, crc_table, n, lane);
    const bool ok = status == pi::ST_OK && !memcmp(win, text, n) && ~crc == m.crc;
    free(pay);
    free(win);
    if (!ok) fprintf(stderr, "inflate core: status %u\n", status);
    return ok;
}

int main(int argc, char **argv) {
    bool check = false;
    int arg = 1;
    if (arg < argc && !strcmp(argv[arg], "--check")) check = true, arg++;
    if (argc - arg < 2) {
        fprintf(stderr, "usage: deflate_host [--check] IN OUT [cut ..]\n");
        return 2;
    }
    FILE *f = fopen(argv[arg], "rb");
    if (!f) {
        perror(argv[arg]);
        return 2;
    }
    std::vector<uint8_t> data;
    uint8_t chunk[65536];
    for (size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) data.insert(data.end(), chunk, chunk + got);
    fclose(f);
    FILE *out = fopen(argv[arg + 1], "wb");
    if (!out) {
        perror(argv[arg + 1]);
        return 2;
    }
    std::vector<uint64_t> bounds(1, 0);
    for (int i = arg + 2; i < argc; i++) {
        const uint64_t c = strtoull(argv[i], nullptr, 10);
        if (c < bounds.back() || c > data.size()) {
            fprintf(stderr, "cut %s: not ascending or beyond the input\n", argv[i]);
            return 2;
        }
        bounds.push_back(c);
    }
    bounds.push_back(data.size());
    uint32_t crc_table[256];
    for (uint32_t i = 0; i < 256; i++) crc_table[i] = pi::crc_table_entry(i);
    std::vector<uint32_t> last(1u << pd::HASH_BITS), choice(pd::TILE);
    pd::Work *work = new pd::Work;
    uint64_t index = 0, total = 0;
    for (size_t piece = 0; piece + 1 < bounds.size(); piece++)
        for (uint64_t at = bounds[piece]; at < bounds[piece + 1]; at += pd::MEMBER_TEXT) {
            const uint32_t n = (uint32_t)(bounds[piece + 1] - at < pd::MEMBER_TEXT ? bounds[piece + 1] - at : pd::MEMBER_TEXT);
            // (the text, the tokens and the member in buffers of their own sizes)
            uint8_t *text = (uint8_t *)malloc(n), *member = (uint8_t *)malloc(pd::SLOT);
            uint32_t *tokens = (uint32_t *)malloc(n * sizeof(uint32_t));
            memcpy(text, data.data() + at, n);
            const uint32_t size = pd::deflate_member_serial(text, n, tokens, last.data(), choice.data(), *work, crc_table, member);
            if (size > n + pd::STORED_HEAD + pd::HEADER + pd::TRAILER || size > pd::SLOT) {
                fprintf(stderr, "member %llu: %u bytes for %u of text\n", (unsigned long long)index, size, n);
                return 1;
            }
            if (check && !check_member(member, size, text, n, crc_table)) {
                fprintf(stderr, "member %llu (text %llu + %u) fails the check\n", (unsigned long long)index, (unsigned long long)at, n);
                return 1;
            }
            fwrite(member, 1, size, out);
            printf("%llu %zu %llu %u %u\n", (unsigned long long)index, piece, (unsigned long long)at, n, size);
            free(text);
            free(member);
            free(tokens);
            index++;
            total += size;
        }
    printf("members %llu bytes %llu\n", (unsigned long long)index, (unsigned long long)total);
    delete work;
    fclose(out);
    return 0;
}
