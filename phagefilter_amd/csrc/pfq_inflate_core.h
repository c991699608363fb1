// Blocked gzip (BGZF): the header walk of one member and RFC 1951 for one member's deflate payload, written once as
// __host__ __device__ code.  k_gz_inflate (pfq_inflate.hip) and the stand-alone host program tools/inflate_host.cpp compile this
// same text, so what the sanitizers see on the host is what the device runs.  The input is untrusted: every doubt is a
// rejection (a status), never a fault; a rejected member is inflated by zlib on the host, so rejecting cannot change a result.
//
// The decoder works on an environment `Env` that owns the bytes:
//   uint32_t in(uint32_t pos)                        payload byte pos; the core only asks for pos < the payload's length
//   void put(uint32_t at, uint32_t byte)             window[at] = byte; the core only writes at < ISIZE <= 65536
//   void copy(uint32_t at, uint32_t dist, uint32_t n)     window[at + i] = window[at + i - dist], i ascending; dist <= at
//   void copy_in(uint32_t at, uint32_t pos, uint32_t n)   window[at + i] = in(pos + i)
// Every loop of the core consumes at least one bit of the payload per iteration or ends, so a member costs at most
// 8 * payload + 65536 iterations.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PFQ_HD __host__ __device__
#else
#define PFQ_HD
#endif

namespace pfq_inflate {

constexpr uint32_t TEXT_MAX = 65536;  // = PFQ_GZ_MEMBER_TEXT_MAX
enum Status : uint32_t { ST_OK = 0, ST_MALFORMED = 1, ST_LENGTH = 2, ST_CRC = 3 };

// ---- the header walk ------------------------------------------------------------------------------------------------------
enum Walk : uint32_t { WALK_TAKEN = 0, WALK_SHORT = 1, WALK_FOREIGN = 2 };  // SHORT: fewer bytes left than the header or the member needs
struct Member {
    uint32_t size, header, isize, crc;  // bytes of the member, of its header (the payload is [header, size - 8)), the trailer's words
};
PFQ_HD inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
PFQ_HD inline uint32_t le32(const uint8_t *p) { return le16(p) | le16(p + 2) << 16; }

// The member that begins at gz[0] of `left` bytes.  Nothing beyond gz[left) is read.
PFQ_HD inline Walk walk_member(const uint8_t *gz, uint64_t left, Member *m) {
    if (left < 12) return WALK_SHORT;  // (the fixed header and XLEN: shortness is decided before the bytes are looked at)
    if (gz[0] != 0x1f || gz[1] != 0x8b || gz[2] != 8) return WALK_FOREIGN;
    const uint32_t flg = gz[3];
    if (!(flg & 4) || (flg & 0xe0)) return WALK_FOREIGN;
    const uint64_t xlen = le16(gz + 10);
    if (left < 12 + xlen) return WALK_SHORT;
    uint64_t at = 12;
    const uint64_t xend = 12 + xlen;
    uint32_t bsize = 0;
    bool have = false;
    while (at < xend) {
        if (xend - at < 4) return WALK_FOREIGN;
        const uint64_t slen = le16(gz + at + 2);
        if (xend - at - 4 < slen) return WALK_FOREIGN;
        if (gz[at] == 'B' && gz[at + 1] == 'C' && slen == 2 && !have) {
            bsize = le16(gz + at + 4);
            have = true;
        }
        at += 4 + slen;
    }
    if (!have) return WALK_FOREIGN;
    const uint64_t size = (uint64_t)bsize + 1;
    if (left < size) return WALK_SHORT;
    for (int part = 0; part < 2; part++)  // FNAME, FCOMMENT: zero-terminated, inside the member
        if (flg & (part ? 16u : 8u)) {
            while (at < size && gz[at]) at++;
            if (at >= size) return WALK_FOREIGN;
            at++;
        }
    if (flg & 2) at += 2;  // FHCRC
    if (at + 1 + 8 > size) return WALK_FOREIGN;  // (a payload of at least one byte, then the trailer)
    m->size = (uint32_t)size;
    m->header = (uint32_t)at;
    m->crc = le32(gz + size - 8);
    m->isize = le32(gz + size - 4);
    if (m->isize > TEXT_MAX) return WALK_FOREIGN;
    return WALK_TAKEN;
}

// ---- CRC-32 in pieces -------------------------------------------------------------------------------------------------------
// Polynomials over GF(2) in the reflected form of CRC-32: bit 31 is x^0.  The register after the bytes A ++ B, started from R, is
// reg(0, B) ^ reg(R, A) * x^(8 |B|) mod P, so every lane takes a piece from register 0 (the first from ~0), multiplies by the
// power that stands for the bytes behind its piece, and the pieces are xor-ed.
constexpr uint32_t CRC_POLY = 0xedb88320u;
PFQ_HD inline uint32_t crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; k++) i = (i >> 1) ^ ((i & 1) ? CRC_POLY : 0u);
    return i;
}
PFQ_HD inline uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & 0x80000000u) p ^= b;
        a <<= 1;
        b = (b >> 1) ^ ((b & 1) ? CRC_POLY : 0u);
    }
    return p;
}
PFQ_HD inline uint32_t gf_x8_pow(uint32_t n) {  // x^(8 n) mod P
    uint32_t r = 0x80000000u, sq = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1) r = gf_mul(r, sq);
        sq = gf_mul(sq, sq);
    }
    return r;
}
constexpr uint32_t CRC_PIECES = 64;
// Piece `lane` of CRC_PIECES over window[0, n): what it contributes to the register; the xor of all pieces, inverted, is the CRC.
template <class Window>
PFQ_HD inline uint32_t crc_piece(const Window &window, const uint32_t *table, uint32_t n, uint32_t lane) {
    const uint32_t piece = (n + CRC_PIECES - 1) / CRC_PIECES;
    uint32_t lo = lane * piece, hi = lo + piece;
    if (lo > n) lo = n;
    if (hi > n) hi = n;
    uint32_t r = lane ? 0u : 0xffffffffu;
    for (uint32_t i = lo; i < hi; i++) r = (r >> 8) ^ table[(r ^ window[i]) & 0xff];
    return r ? gf_mul(r, gf_x8_pow(n - hi)) : 0u;
}

// ---- the decode tables of one block -----------------------------------------------------------------------------------------
// A direct-lookup first level over the next LIT_BITS / DIST_BITS bits of input (bit-reversed canonical codes): entry =
// symbol << 4 | code length, 0 where the bits begin a longer code or none.  Longer codes are found by the canonical walk over
// cnt (codes per length) and sym (symbols by length, then value).
constexpr uint32_t LIT_BITS = 10, DIST_BITS = 8, CLEN_BITS = 7;
constexpr uint32_t N_LIT = 288, N_DIST = 32, N_LENS = 320;
struct Tables {
    uint16_t *lit_fast;   // [1 << LIT_BITS]
    uint16_t *dist_fast;  // [1 << DIST_BITS]; also the code-length code's while a dynamic header is read
    uint16_t *lit_sym;    // [N_LIT]
    uint16_t *dist_sym;   // [N_DIST]
    uint16_t *lit_cnt;    // [16]
    uint16_t *dist_cnt;   // [16]
    uint16_t *next;       // [16] scratch of build()
    uint8_t *lens;        // [N_LENS] code lengths of the block being set up
};
constexpr uint32_t TABLES_U16 = (1u << LIT_BITS) + (1u << DIST_BITS) + N_LIT + N_DIST + 16 + 16 + 16;
constexpr uint32_t TABLES_BYTES = TABLES_U16 * 2 + N_LENS;
// Carves the tables out of TABLES_BYTES bytes at `mem` (2-byte aligned).
PFQ_HD inline Tables tables_at(void *mem) {
    Tables t;
    uint16_t *p = static_cast<uint16_t *>(mem);
    t.lit_fast = p, p += 1u << LIT_BITS;
    t.dist_fast = p, p += 1u << DIST_BITS;
    t.lit_sym = p, p += N_LIT;
    t.dist_sym = p, p += N_DIST;
    t.lit_cnt = p, p += 16;
    t.dist_cnt = p, p += 16;
    t.next = p, p += 16;
    t.lens = reinterpret_cast<uint8_t *>(p);
    return t;
}

enum Build : int { BUILD_OK = 0, BUILD_OVER = 1, BUILD_INCOMPLETE = 2, BUILD_EMPTY = 3 };  // EMPTY: no code at all
// The canonical code of lens[0, n) (each 0 .. 15): cnt, sym and the first level of `bits` bits.  The tables are filled for
// every outcome but BUILD_OVER, so the caller decides what an incomplete set means.
PFQ_HD inline Build build(const uint8_t *lens, uint32_t n, uint32_t bits, uint16_t *fast, uint16_t *cnt, uint16_t *sym, uint16_t *next) {
    for (uint32_t l = 0; l < 16; l++) cnt[l] = 0;
    for (uint32_t s = 0; s < n; s++) cnt[lens[s] & 15]++;
    for (uint32_t i = 0; i < (1u << bits); i++) fast[i] = 0;
    if (cnt[0] == n) return BUILD_EMPTY;
    int32_t left = 1;
    for (uint32_t l = 1; l < 16; l++) {
        left = left * 2 - (int32_t)cnt[l];
        if (left < 0) return BUILD_OVER;
    }
    // next[l]: where in sym the symbols of length l begin
    uint32_t at = 0;
    for (uint32_t l = 1; l < 16; l++) {
        next[l] = (uint16_t)at;
        at += cnt[l];
    }
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t l = lens[s] & 15;
        if (l) sym[next[l]++] = (uint16_t)s;
    }
    // the first level: symbols in order of (length, value) take consecutive codes
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= bits; l++) {
        code <<= 1;
        for (uint32_t j = 0; j < cnt[l]; j++, code++, idx++) {
            uint32_t rev = 0;
            for (uint32_t k = 0; k < l; k++) rev |= ((code >> k) & 1u) << (l - 1 - k);
            const uint16_t e = (uint16_t)((uint32_t)sym[idx] << 4 | l);
            for (uint32_t i = rev; i < (1u << bits); i += 1u << l) fast[i] = e;
        }
    }
    return left > 0 ? BUILD_INCOMPLETE : BUILD_OK;
}

// ---- the bit reader -----------------------------------------------------------------------------------------------------------
template <class Env>
struct Bits {
    Env &env;
    uint32_t pos, end;  // the next payload byte to load; the payload's length
    uint32_t buf, n;    // n bits of input not yet used, lowest first
    bool over;          // more bits were asked for than the payload holds
    PFQ_HD Bits(Env &e, uint32_t len) : env(e), pos(0), end(len), buf(0), n(0), over(false) {}
    PFQ_HD void refill() {  // at least 25 bits, or all that is left
        while (n <= 24 && pos < end) {
            buf |= env.in(pos++) << n;
            n += 8;
        }
    }
    PFQ_HD uint32_t take(uint32_t k) {  // k <= 16
        refill();
        if (k > n) {
            over = true;
            return 0;
        }
        const uint32_t v = buf & ((1u << k) - 1u);
        buf >>= k;
        n -= k;
        return v;
    }
    // One symbol of a code, or -1: no code of the set begins the bits that are left.
    PFQ_HD int32_t decode(const uint16_t *fast, uint32_t bits, const uint16_t *cnt, const uint16_t *sym) {
        refill();
        const uint32_t e = fast[buf & ((1u << bits) - 1u)];
        if (e) {
            const uint32_t l = e & 15u;
            if (l > n) return -1;
            buf >>= l;
            n -= l;
            return (int32_t)(e >> 4);
        }
        int32_t code = 0, first = 0, index = 0;
        for (uint32_t l = 1; l < 16; l++) {
            if (l > n) return -1;
            code |= (int32_t)((buf >> (l - 1)) & 1u);
            const int32_t count = cnt[l];
            if (code - count < first) {
                buf >>= l;
                n -= l;
                return sym[index + (code - first)];
            }
            index += count;
            first = (first + count) << 1;
            code <<= 1;
        }
        return -1;
    }
};

PFQ_HD inline uint32_t clen_order(uint32_t i) {  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                        11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

struct Seen {
    uint32_t max_dist, max_len, blocks[3];  // the largest distance and length met; blocks by type
};

// One member: payload of pay_len bytes behind env.in, text of exactly isize bytes into the window.
template <class Env>
PFQ_HD inline uint32_t inflate_member(Env &env, const Tables &T, uint32_t pay_len, uint32_t isize, Seen *seen) {
    Bits<Env> b(env, pay_len);
    uint32_t out = 0, last;
    if (isize > TEXT_MAX) return ST_LENGTH;
    do {
        last = b.take(1);
        const uint32_t type = b.take(2);
        if (b.over || type == 3) return ST_MALFORMED;
        if (seen) seen->blocks[type]++;
        if (type == 0) {
            b.take(b.n & 7u);  // to the byte boundary (refilled: n >= 25 or everything)
            const uint32_t len = b.take(16), nlen = b.take(16);
            if (b.over || (len ^ nlen) != 0xffffu) return ST_MALFORMED;
            b.pos -= b.n >> 3;  // whole bytes loaded ahead go back
            b.buf = b.n = 0;
            if (len > b.end - b.pos) return ST_MALFORMED;
            if (len > isize - out) return ST_LENGTH;
            env.copy_in(out, b.pos, len);
            b.pos += len;
            out += len;
            continue;
        }
        if (type == 1) {
            for (uint32_t s = 0; s < N_LIT; s++) T.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            build(T.lens, N_LIT, LIT_BITS, T.lit_fast, T.lit_cnt, T.lit_sym, T.next);
            for (uint32_t s = 0; s < N_DIST; s++) T.lens[s] = 5;
            build(T.lens, N_DIST, DIST_BITS, T.dist_fast, T.dist_cnt, T.dist_sym, T.next);
        } else {
            const uint32_t hlit = b.take(5) + 257, hdist = b.take(5) + 1, hclen = b.take(4) + 4;
            if (b.over || hlit > 286 || hdist > 30) return ST_MALFORMED;
            for (uint32_t i = 0; i < 19; i++) T.lens[clen_order(i)] = i < hclen ? (uint8_t)b.take(3) : 0;
            if (b.over) return ST_MALFORMED;
            if (build(T.lens, 19, CLEN_BITS, T.dist_fast, T.dist_cnt, T.dist_sym, T.next) != BUILD_OK) return ST_MALFORMED;
            const uint32_t total = hlit + hdist;
            uint32_t i = 0;
            while (i < total) {
                const int32_t s = b.decode(T.dist_fast, CLEN_BITS, T.dist_cnt, T.dist_sym);
                if (s < 0) return ST_MALFORMED;
                if (s < 16) {
                    T.lens[i++] = (uint8_t)s;
                    continue;
                }
                uint32_t rep, val = 0;
                if (s == 16) {
                    if (!i) return ST_MALFORMED;
                    val = T.lens[i - 1];
                    rep = 3 + b.take(2);
                } else if (s == 17) {
                    rep = 3 + b.take(3);
                } else {
                    rep = 11 + b.take(7);
                }
                if (b.over || rep > total - i) return ST_MALFORMED;
                while (rep--) T.lens[i++] = (uint8_t)val;
            }
            if (!T.lens[256]) return ST_MALFORMED;
            // (the distance lengths are read by the second build before anything overwrites lens: dist_fast is not lens)
            if (build(T.lens, hlit, LIT_BITS, T.lit_fast, T.lit_cnt, T.lit_sym, T.next) != BUILD_OK) return ST_MALFORMED;
            const Build d = build(T.lens + hlit, hdist, DIST_BITS, T.dist_fast, T.dist_cnt, T.dist_sym, T.next);
            if (d == BUILD_OVER) return ST_MALFORMED;
            if (d == BUILD_INCOMPLETE && !(T.dist_cnt[0] + 1u == hdist && T.dist_cnt[1] == 1)) return ST_MALFORMED;
        }
        for (;;) {
            const int32_t s = b.decode(T.lit_fast, LIT_BITS, T.lit_cnt, T.lit_sym);
            if (s < 0) return ST_MALFORMED;
            if (s < 256) {
                if (out >= isize) return ST_LENGTH;
                env.put(out++, (uint32_t)s);
                continue;
            }
            if (s == 256) break;
            if (s > 285) return ST_MALFORMED;
            uint32_t len;
            if (s < 265) len = (uint32_t)s - 254;
            else if (s == 285) len = 258;
            else {
                const uint32_t e = ((uint32_t)s - 261) >> 2;
                len = 3 + ((4 + (((uint32_t)s - 265) & 3u)) << e) + b.take(e);
            }
            const int32_t c = b.decode(T.dist_fast, DIST_BITS, T.dist_cnt, T.dist_sym);
            if (c < 0 || c > 29) return ST_MALFORMED;
            uint32_t dist;
            if (c < 4) dist = (uint32_t)c + 1;
            else {
                const uint32_t e = ((uint32_t)c >> 1) - 1;
                dist = 1 + ((2 + ((uint32_t)c & 1u)) << e) + b.take(e);
            }
            if (b.over || dist > out) return ST_MALFORMED;
            if (len > isize - out) return ST_LENGTH;
            if (seen) {
                if (dist > seen->max_dist) seen->max_dist = dist;
                if (len > seen->max_len) seen->max_len = len;
            }
            env.copy(out, dist, len);
            out += len;
        }
    } while (!last);
    if (out != isize) return ST_LENGTH;
    if (b.pos - (b.n >> 3) != b.end) return ST_LENGTH;  // payload bytes behind the final block
    return ST_OK;
}

}  // namespace pfq_inflate
