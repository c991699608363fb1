// The inflate core of libpfq (phagefilter_amd/csrc/pfq_inflate_core.h) on the host, for sanitizer runs: the very text the device
// kernel compiles, over heap buffers of exactly the payload's and the text's size, so a read or write one byte outside is a
// report.  Build: g++ -std=c++17 -g -fsanitize=address,undefined -I phagefilter_amd/csrc tools/inflate_host.cpp -o inflate_host
// Use:   inflate_host IN.gz OUT.txt
// Walks the members of IN by their headers and prints one line a member:
//   <index> <status> <crc of the text produced, hex> <isize> <payload bytes> <largest distance> <largest length>
// then "stop <taken|short|foreign> <offset>".  OUT receives the texts of the members with status 0, back to back.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pfq_inflate_core.h"

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

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: inflate_host IN.gz OUT.txt\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint8_t> gz;
    uint8_t chunk[65536];
    for (size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) gz.insert(gz.end(), chunk, chunk + got);
    fclose(f);
    FILE *out = fopen(argv[2], "wb");
    if (!out) {
        perror(argv[2]);
        return 2;
    }
    uint32_t crc_table[256];
    for (uint32_t i = 0; i < 256; i++) crc_table[i] = pi::crc_table_entry(i);
    std::vector<uint8_t> table_mem(pi::TABLES_BYTES + 2);
    const pi::Tables T = pi::tables_at(table_mem.data());
    uint64_t at = 0, index = 0;
    pi::Walk w = pi::WALK_TAKEN;
    while (at < gz.size()) {
        // (the member alone in a buffer of its own size: the walk may not look beyond it either)
        pi::Member m{};
        {
            uint8_t *rest = (uint8_t *)malloc(gz.size() - at);
            memcpy(rest, gz.data() + at, gz.size() - at);
            w = pi::walk_member(rest, gz.size() - at, &m);
            free(rest);
        }
        if (w != pi::WALK_TAKEN) break;
        const uint32_t pay_len = m.size - 8 - m.header;
        uint8_t *pay = (uint8_t *)malloc(pay_len), *win = (uint8_t *)malloc(m.isize ? m.isize : 1);
        memcpy(pay, gz.data() + at + m.header, pay_len);
        memset(win, 0, m.isize ? m.isize : 1);
        HostEnv env{pay, win};
        pi::Seen seen{};
        uint32_t status = pi::inflate_member(env, T, pay_len, m.isize, &seen);
        uint32_t crc = 0;
        for (uint32_t lane = 0; lane < pi::CRC_PIECES; lane++) crc ^= pi::crc_piece(win, crc_table, m.isize, lane);
        crc = ~crc;
        if (status == pi::ST_OK && crc != m.crc) status = pi::ST_CRC;
        if (status == pi::ST_OK) fwrite(win, 1, m.isize, out);
        printf("%llu %u %08x %u %u %u %u\n", (unsigned long long)index, status, crc, m.isize, pay_len, seen.max_dist, seen.max_len);
        free(pay);
        free(win);
        at += m.size;
        index++;
    }
    printf("stop %s %llu\n", at >= gz.size() ? "taken" : w == pi::WALK_SHORT ? "short" : "foreign", (unsigned long long)at);
    fclose(out);
    return 0;
}
