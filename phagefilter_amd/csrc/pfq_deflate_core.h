// RFC 1951 for one member of blocked gzip (BGZF), the writing side: the counterpart of pfq_inflate_core.h, written once as
// __host__ __device__ code.  k_bgzf_deflate (pfq_deflate.hip) and the stand-alone host program tools/deflate_host.cpp compile this
// same text.  The contract: THE BYTES OF A MEMBER ARE A PURE FUNCTION OF THE MEMBER'S TEXT.  The device finds the tokens in
// parallel and the host program one after the other; both follow the rules below, in which no order of execution appears.
//
// Matching.  Positions are taken in tiles of TILE = 256 consecutive bytes.  hash(p) = hash4 of the little-endian dword
// text[p .. p + 4), defined for p + 4 <= n.  last[h] before a tile = the largest position below the tile's first with that hash.
//   candidate A (only if p + 4 <= n, last[hash(p)] exists and p - last <= 32768): distance p - last
//   candidate B (only if p >= 1): distance 1
//   the length of a candidate at distance d is the common prefix of text[p ..) and text[p - d ..), at most 258 and at most n - p;
//   the longer candidate is the choice of p, on a tie candidate B (the smaller distance).
// Parse.  Greedy from position 0: at p, the choice is taken if its length is >= 4, or 3 with a distance < 4096, and the parse
//   goes on at p + length; otherwise text[p] is a literal and the parse goes on at p + 1.  A choice depends on the text and on p's
//   tile alone, never on the parse, so the lanes of the device make all choices of a tile at once and then find the chain.
// Coding.  One dynamic block (BTYPE 10) from the member's own token counts (the end-of-block symbol counts once).  A tree with
//   fewer than two used symbols gets symbol 0, then 1, with count 1 until it has two.  Code lengths: the minimum-redundancy lengths
//   of the counts sorted by (count, symbol) (Moffat and Katajainen's in-place algorithm), limited to 15 bits (7 for the code-length
//   code) by moving codes down from the longest length until Kraft's sum is 1; the k-th longest length goes to the k-th symbol of
//   the sorted order.  The lengths are sent with runs: a run of zeros as 18 (11 .. 138, the most first), then 17 (3 .. 10), then
//   single zeros; a run of another value as the value, then 16 (3 .. 6, the most first), then the value again for what is left.
//   HLIT and HDIST end at the last used symbol (HLIT >= 257), HCLEN at the last used entry of the order (>= 4).
//   If the block's bytes are not fewer than the text's, the member is one stored block (BTYPE 00) instead: text + 5 bytes.
// Framing.  The 18-byte header 1f 8b 08 04 | mtime 0 | xfl 0 | os ff | xlen 6 | 'B' 'C' 2 0 BSIZE, the payload, CRC-32, ISIZE.
#pragma once
#include <stdint.h>

#include "pfq_inflate_core.h"

namespace pfq_deflate {

constexpr uint32_t MEMBER_TEXT = 65280;  // = PFQ_BGZF_MEMBER_TEXT: text bytes of a full member
constexpr uint32_t SLOT = 65536;         // a member is at most MEMBER_TEXT + 5 + 26 bytes
constexpr uint32_t HEADER = 18, TRAILER = 8, STORED_HEAD = 5;
constexpr uint32_t TILE = 256, HASH_BITS = 13, MAX_MATCH = 258, MAX_DIST = 32768, SHORT_DIST = 4096;
constexpr uint32_t N_LIT = 286, N_DIST = 30, N_CLEN = 19, EOB = 256;
// A token, one per position of the text: 0 off the parse's chain, TOK_LIT | byte, or TOK_MATCH | (length - 3) << 16 | (distance - 1).
constexpr uint32_t TOK_LIT = 0x80000000u, TOK_MATCH = 0x40000000u;

PFQ_HD inline uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - HASH_BITS); }

// The choice at a position from its candidates' lengths (0: no such candidate): TOK_MATCH | .., or 0 for a literal.
PFQ_HD inline uint32_t choose(uint32_t len_a, uint32_t dist_a, uint32_t len_b) {
    uint32_t len = len_b, dist = 1;
    if (len_a > len_b) len = len_a, dist = dist_a;
    if (len >= 4 || (len == 3 && dist < SHORT_DIST)) return TOK_MATCH | (len - 3) << 16 | (dist - 1);
    return 0;
}
PFQ_HD inline uint32_t choice_len(uint32_t choice) { return choice ? ((choice >> 16) & 0xffu) + 3 : 1; }  // what the parse advances by

template <class Text>
PFQ_HD inline uint32_t common_prefix(const Text &text, uint32_t p, uint32_t q, uint32_t most) {
    uint32_t k = 0;
    while (k < most && text[p + k] == text[q + k]) k++;
    return k;
}

// ---- symbols --------------------------------------------------------------------------------------------------------------
struct Sym {
    uint32_t sym, extra_bits, extra;
};
PFQ_HD inline Sym length_sym(uint32_t len) {  // 3 .. 258
    const uint32_t l = len - 3;
    if (len == MAX_MATCH) return Sym{285, 0, 0};
    uint32_t e = 0;
    while ((l >> e) >= 8) e++;
    return Sym{257 + 4 * e + (l >> e), e, l & ((1u << e) - 1u)};
}
PFQ_HD inline Sym dist_sym(uint32_t dist) {  // 1 .. 32768
    const uint32_t d = dist - 1;
    uint32_t e = 0;
    while ((d >> e) >= 4) e++;
    return Sym{2 * e + (d >> e), e, d & ((1u << e) - 1u)};
}

// ---- code lengths -----------------------------------------------------------------------------------------------------------
// Everything the serial part of a member needs, in LDS on the device.  code[s] = the bit-reversed canonical code | length << 16.
struct Work {
    uint32_t lit_count[N_LIT + 2], dist_count[N_DIST + 2], clen_count[N_CLEN + 1];
    uint32_t lit_code[N_LIT + 2], dist_code[N_DIST + 2], clen_code[N_CLEN + 1];
    uint32_t key[N_LIT + 2], a[N_LIT + 2], per[33], next[16];  // scratch of lengths() and codes()
    uint8_t clen_len[N_CLEN + 1];
    uint8_t lens[N_LIT + N_DIST + 4];       // the literal tree's lengths, behind them the distance tree's
    uint16_t run[N_LIT + N_DIST + 4];       // the lengths as run symbols: symbol | extra << 8
    uint32_t n_run, hlit, hdist, hclen;
};

// count[0, n) -> len[0, n), each <= limit; at least two symbols get a length (counts of 0 are raised as the rules say).
PFQ_HD inline void lengths(const uint32_t *count, uint32_t n, uint32_t limit, uint8_t *len, Work &w) {
    uint32_t *key = w.key, *a = w.a, *per = w.per;
    uint32_t used = 0, raised = 0;
    for (uint32_t s = 0; s < n; s++) used += count[s] != 0;
    for (uint32_t s = 0; used < 2 && s < 2; s++)
        if (!count[s]) raised |= 1u << s, used++;
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t c = count[s] ? count[s] : (s < 2 && (raised >> s & 1u)) ? 1u : 0u;
        len[s] = 0;
        if (c) key[m++] = c << 9 | s;
    }
    // ascending (count, symbol): Shell's sort
    for (uint32_t gap = 132; gap; gap = gap > 1 && gap < 5 ? 1 : gap * 5 / 11) {
        for (uint32_t i = gap; i < m; i++) {
            const uint32_t v = key[i];
            uint32_t j = i;
            for (; j >= gap && key[j - gap] > v; j -= gap) key[j] = key[j - gap];
            key[j] = v;
        }
    }
    for (uint32_t i = 0; i < m; i++) a[i] = key[i] >> 9;
    // minimum-redundancy code lengths in place: a[i] = the length of the i-th smallest count
    a[0] += a[1];
    uint32_t root = 0, leaf = 2;
    for (uint32_t next = 1; next + 1 < m; next++) {
        if (leaf >= m || a[root] < a[leaf]) {
            a[next] = a[root];
            a[root++] = next;
        } else
            a[next] = a[leaf++];
        if (leaf >= m || (root < next && a[root] < a[leaf])) {
            a[next] += a[root];
            a[root++] = next;
        } else
            a[next] += a[leaf++];
    }
    a[m - 2] = 0;
    for (int32_t next = (int32_t)m - 3; next >= 0; next--) a[next] = a[a[next]] + 1;
    {
        int32_t avail = 1, used_nodes = 0, depth = 0, r = (int32_t)m - 2, next = (int32_t)m - 1;
        while (avail > 0) {
            while (r >= 0 && (int32_t)a[r] == depth) used_nodes++, r--;
            while (avail > used_nodes) a[next--] = (uint32_t)depth, avail--;
            avail = 2 * used_nodes;
            depth++;
            used_nodes = 0;
        }
    }
    // codes per length, limited
    for (uint32_t l = 0; l <= 32; l++) per[l] = 0;
    for (uint32_t i = 0; i < m; i++) per[a[i] > 32 ? 32 : a[i]]++;
    for (uint32_t l = limit + 1; l <= 32; l++) per[limit] += per[l];
    uint32_t total = 0;
    for (uint32_t l = limit; l >= 1; l--) total += per[l] << (limit - l);
    while (total > (1u << limit)) {
        per[limit]--;
        for (uint32_t l = limit - 1; l >= 1; l--)
            if (per[l]) {
                per[l]--;
                per[l + 1] += 2;
                break;
            }
        total--;
    }
    uint32_t i = 0;
    for (uint32_t l = limit; l >= 1; l--)
        for (uint32_t c = per[l]; c; c--) len[key[i++] & 511u] = (uint8_t)l;
}

// The canonical code of len[0, n): code[s] = reversed code | length << 16, 0 for an unused symbol.
PFQ_HD inline void codes(const uint8_t *len, uint32_t n, uint32_t *code, Work &w) {
    uint32_t *per = w.per, *next = w.next;
    for (uint32_t l = 0; l < 16; l++) per[l] = 0;
    for (uint32_t s = 0; s < n; s++) per[len[s]]++;
    per[0] = 0;
    uint32_t c = 0;
    for (uint32_t l = 1; l < 16; l++) {
        c = (c + per[l - 1]) << 1;
        next[l] = c;
    }
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t l = len[s];
        if (!l) {
            code[s] = 0;
            continue;
        }
        const uint32_t v = next[l]++;
        uint32_t rev = 0;
        for (uint32_t k = 0; k < l; k++) rev |= ((v >> k) & 1u) << (l - 1 - k);
        code[s] = rev | l << 16;
    }
}

// From the token counts (EOB counted) to the codes and the header's run symbols; returns the bits of the whole block.
PFQ_HD inline uint32_t plan(Work &w) {
    lengths(w.lit_count, N_LIT, 15, w.lens, w);
    w.hlit = N_LIT;
    while (w.hlit > 257 && !w.lens[w.hlit - 1]) w.hlit--;
    uint8_t *dl = w.lens + w.hlit;  // (the distance lengths are built behind the literal lengths that are sent)
    lengths(w.dist_count, N_DIST, 15, dl, w);
    w.hdist = N_DIST;
    while (w.hdist > 1 && !dl[w.hdist - 1]) w.hdist--;
    codes(w.lens, w.hlit, w.lit_code, w);
    codes(dl, w.hdist, w.dist_code, w);
    // the lengths as run symbols
    const uint32_t total = w.hlit + w.hdist;
    for (uint32_t s = 0; s < N_CLEN; s++) w.clen_count[s] = 0;
    uint32_t n_run = 0, i = 0;
    while (i < total) {
        const uint32_t v = w.lens[i];
        uint32_t run = 1;
        while (i + run < total && w.lens[i + run] == v) run++;
        i += run;
        if (!v) {
            while (run >= 11) {
                const uint32_t r = run < 138 ? run : 138;
                w.run[n_run++] = (uint16_t)(18 | (r - 11) << 8);
                run -= r;
            }
            if (run >= 3) {
                w.run[n_run++] = (uint16_t)(17 | (run - 3) << 8);
                run = 0;
            }
        } else {
            w.run[n_run++] = (uint16_t)v;
            run--;
            while (run >= 3) {
                const uint32_t r = run < 6 ? run : 6;
                w.run[n_run++] = (uint16_t)(16 | (r - 3) << 8);
                run -= r;
            }
        }
        while (run--) w.run[n_run++] = (uint16_t)v;
    }
    w.n_run = n_run;
    for (uint32_t r = 0; r < n_run; r++) w.clen_count[w.run[r] & 31u]++;
    lengths(w.clen_count, N_CLEN, 7, w.clen_len, w);
    codes(w.clen_len, N_CLEN, w.clen_code, w);
    w.hclen = N_CLEN;
    while (w.hclen > 4 && !(w.clen_code[pfq_inflate::clen_order(w.hclen - 1)] >> 16)) w.hclen--;
    uint32_t bits = 3 + 5 + 5 + 4 + 3 * w.hclen;
    for (uint32_t r = 0; r < n_run; r++) {
        const uint32_t s = w.run[r] & 31u;
        bits += (w.clen_code[s] >> 16) + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
    }
    for (uint32_t s = 0; s < w.hlit; s++) {
        uint32_t extra = 0;
        if (s >= 265 && s < 285) extra = (s - 261) >> 2;
        bits += w.lit_count[s] * ((w.lit_code[s] >> 16) + extra);
    }
    for (uint32_t s = 0; s < w.hdist; s++) bits += w.dist_count[s] * ((w.dist_code[s] >> 16) + (s >= 4 ? (s >> 1) - 1 : 0));
    return bits;
}

// ---- bits ---------------------------------------------------------------------------------------------------------------------
// One writer over zeroed bytes, for what one thread writes: the headers, the end of block, the trailer.
struct BitWriter {
    uint8_t *buf;
    uint32_t bit;
    PFQ_HD void put(uint32_t v, uint32_t n) {  // n <= 24
        uint32_t at = bit >> 3;
        uint32_t x = v << (bit & 7u);
        for (uint32_t left = n + (bit & 7u); left; left = left > 8 ? left - 8 : 0, x >>= 8) buf[at++] |= (uint8_t)x;
        bit += n;
    }
    PFQ_HD void code(uint32_t c) { put(c & 0xffffu, c >> 16); }
};

PFQ_HD inline void put_gzip_header(uint8_t *at, uint32_t member_bytes) {
    const uint64_t lo = 0x0000000004088b1full, hi = 0x000243420006ff00ull;  // 1f 8b 08 04 00 00 00 00 | 00 ff 06 00 'B' 'C' 02 00
    for (uint32_t i = 0; i < 8; i++) at[i] = (uint8_t)(lo >> (8 * i)), at[8 + i] = (uint8_t)(hi >> (8 * i));
    at[16] = (uint8_t)(member_bytes - 1);
    at[17] = (uint8_t)((member_bytes - 1) >> 8);
}
PFQ_HD inline void put_le32(uint8_t *at, uint32_t v) {
    for (uint32_t i = 0; i < 4; i++) at[i] = (uint8_t)(v >> (8 * i));
}
// The block header of a planned member: BFINAL, BTYPE 10, the three counts, the code-length code, the run symbols.
PFQ_HD inline void put_block_header(BitWriter &b, const Work &w) {
    b.put(1, 1);
    b.put(2, 2);
    b.put(w.hlit - 257, 5);
    b.put(w.hdist - 1, 5);
    b.put(w.hclen - 4, 4);
    for (uint32_t i = 0; i < w.hclen; i++) b.put(w.clen_code[pfq_inflate::clen_order(i)] >> 16, 3);
    for (uint32_t r = 0; r < w.n_run; r++) {
        const uint32_t s = w.run[r] & 31u, x = w.run[r] >> 8;
        b.code(w.clen_code[s]);
        if (s >= 16) b.put(x, s == 16 ? 2 : s == 17 ? 3 : 7);
    }
}
// A token's bits, lowest first: at most 15 + 5 + 15 + 13 = 48.
PFQ_HD inline uint64_t token_bits(const Work &w, uint32_t tok, uint32_t *n_bits) {
    if (tok & TOK_LIT) {
        const uint32_t c = w.lit_code[tok & 0xffu];
        *n_bits = c >> 16;
        return c & 0xffffu;
    }
    const Sym l = length_sym(((tok >> 16) & 0xffu) + 3), d = dist_sym((tok & 0x7fffu) + 1);
    const uint32_t lc = w.lit_code[l.sym], dc = w.dist_code[d.sym];
    uint64_t v = lc & 0xffffu;
    uint32_t n = lc >> 16;
    v |= (uint64_t)l.extra << n, n += l.extra_bits;
    v |= (uint64_t)(dc & 0xffffu) << n, n += dc >> 16;
    v |= (uint64_t)d.extra << n, n += d.extra_bits;
    *n_bits = n;
    return v;
}
PFQ_HD inline void count_token(Work &w, uint32_t tok) {  // (the device counts with LDS atomics instead)
    if (tok & TOK_LIT) {
        w.lit_count[tok & 0xffu]++;
    } else {
        w.lit_count[length_sym(((tok >> 16) & 0xffu) + 3).sym]++;
        w.dist_count[dist_sym((tok & 0x7fffu) + 1).sym]++;
    }
}

// ---- one member, one thread: what tools/deflate_host.cpp runs -----------------------------------------------------------------
// text[0, n), n <= MEMBER_TEXT; tokens [n]; last [1 << HASH_BITS]; member [SLOT].  Returns the member's bytes.
PFQ_HD inline uint32_t deflate_member_serial(const uint8_t *text, uint32_t n, uint32_t *tokens, uint32_t *last, uint32_t *choice, Work &w,
                                             const uint32_t *crc_table, uint8_t *member) {
    for (uint32_t h = 0; h < (1u << HASH_BITS); h++) last[h] = 0;  // position + 1; 0: none
    for (uint32_t s = 0; s < N_LIT + 2; s++) w.lit_count[s] = 0;
    for (uint32_t s = 0; s < N_DIST + 2; s++) w.dist_count[s] = 0;
    uint32_t at = 0;  // where the parse stands
    for (uint32_t t0 = 0; t0 < n; t0 += TILE) {
        const uint32_t t1 = t0 + TILE < n ? t0 + TILE : n;
        for (uint32_t p = t0; p < t1; p++) {
            const uint32_t most = n - p < MAX_MATCH ? n - p : MAX_MATCH;
            uint32_t len_a = 0, dist_a = 0, len_b = 0;
            if (p + 4 <= n) {
                const uint32_t q1 = last[hash4(pfq_inflate::le32(text + p))];
                if (q1 && p - (q1 - 1) <= MAX_DIST) dist_a = p - (q1 - 1), len_a = common_prefix(text, p, q1 - 1, most);
            }
            if (p) len_b = common_prefix(text, p, p - 1, most);
            choice[p - t0] = choose(len_a, dist_a, len_b);
        }
        for (uint32_t p = t0; p < t1; p++) tokens[p] = 0;
        while (at < t1) {
            const uint32_t c = choice[at - t0];
            tokens[at] = c ? c : TOK_LIT | text[at];
            count_token(w, tokens[at]);
            at += choice_len(c);
        }
        for (uint32_t p = t0; p < t1 && p + 4 <= n; p++) {
            uint32_t &e = last[hash4(pfq_inflate::le32(text + p))];
            if (p + 1 > e) e = p + 1;
        }
    }
    w.lit_count[EOB]++;
    const uint32_t bits = plan(w), block_bytes = (bits + 7) / 8;
    const bool stored = block_bytes >= n;
    const uint32_t payload = stored ? n + STORED_HEAD : block_bytes, size = HEADER + payload + TRAILER;
    for (uint32_t i = 0; i < size; i++) member[i] = 0;
    put_gzip_header(member, size);
    if (stored) {
        uint8_t *b = member + HEADER;
        b[0] = 1;
        b[1] = (uint8_t)n, b[2] = (uint8_t)(n >> 8), b[3] = (uint8_t)~n, b[4] = (uint8_t)(~n >> 8);
        for (uint32_t i = 0; i < n; i++) b[STORED_HEAD + i] = text[i];
    } else {
        BitWriter b{member, HEADER * 8};
        put_block_header(b, w);
        for (uint32_t p = 0; p < n; p++)
            if (tokens[p]) {
                uint32_t nb;
                const uint64_t v = token_bits(w, tokens[p], &nb);
                b.put((uint32_t)v & 0xffffffu, nb < 24 ? nb : 24);
                if (nb > 24) b.put((uint32_t)(v >> 24), nb - 24);
            }
        b.code(w.lit_code[EOB]);
    }
    uint32_t crc = 0;
    for (uint32_t lane = 0; lane < pfq_inflate::CRC_PIECES; lane++) crc ^= pfq_inflate::crc_piece(text, crc_table, n, lane);
    put_le32(member + HEADER + payload, ~crc);
    put_le32(member + HEADER + payload + 4, n);
    return size;
}

}  // namespace pfq_deflate
