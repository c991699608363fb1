"""Blocked gzip (BGZF) for the tests: a writer on Python's zlib that controls every header part, a restatement of the member scan
(include/pfq.h, pfq_gz_scan), and the fixed lists of members the inflate tests share: the zoo (every block type and edge of RFC
1951 that zlib can be made to emit) and the corrupt list (members that are framed well and broken inside)."""
import struct
import zlib

import numpy as np

TEXT_MAX = 65536
BLOCK = 65280
END, LIMIT, MORE, FOREIGN = 0, 1, 2, 3
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    """Raw deflate of `text`; flush_at: a Z_FULL_FLUSH after that many bytes."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(text) + c.flush()
    return c.compress(text[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[flush_at:]) + c.flush()


def frame(payload, text_len, crc, before=(), after=(), fname=None, fcomment=None, fhcrc=False):
    """One member round `payload`: a BC subfield among the extra subfields `before` and `after` ((b"XY", data) pairs), the
    optional header parts, the trailer."""
    extra_len = sum(4 + len(d) for _, d in before) + 6 + sum(4 + len(d) for _, d in after)
    opt = (fname + b"\0" if fname is not None else b"") + (fcomment + b"\0" if fcomment is not None else b"")
    total = 12 + extra_len + len(opt) + (2 if fhcrc else 0) + len(payload) + 8
    assert total <= 65536, total
    flg = 4 | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0)
    sub = lambda k, d: k + struct.pack("<H", len(d)) + d
    extra = b"".join(sub(k, d) for k, d in before) + sub(b"BC", struct.pack("<H", total - 1)) + b"".join(sub(k, d) for k, d in after)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + struct.pack("<H", extra_len) + extra + opt
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + payload + struct.pack("<II", crc & 0xFFFFFFFF, text_len)


def member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, **header):
    return frame(deflate(text, level, strategy, flush_at), len(text), zlib.crc32(text), **header)


def write(data, block=BLOCK, level=6, marker=True):
    """`data` as BGZF: members of `block` text bytes, then the end marker."""
    out = [member(data[i:i + block], level) for i in range(0, len(data), block)]
    return b"".join(out) + (member(b"") if marker else b"")


def walk(gz, p):
    """The member at gz[p:]: ("taken", size, header bytes, isize) or ("short",) or ("foreign",)."""
    left = len(gz) - p
    if left < 12:
        return ("short",)
    if gz[p:p + 3] != b"\x1f\x8b\x08":
        return ("foreign",)
    flg = gz[p + 3]
    if not flg & 4 or flg & 0xE0:
        return ("foreign",)
    xlen = struct.unpack_from("<H", gz, p + 10)[0]
    if left < 12 + xlen:
        return ("short",)
    at, xend, bsize = p + 12, p + 12 + xlen, None
    while at < xend:
        if xend - at < 4:
            return ("foreign",)
        slen = struct.unpack_from("<H", gz, at + 2)[0]
        if xend - at - 4 < slen:
            return ("foreign",)
        if gz[at:at + 2] == b"BC" and slen == 2 and bsize is None:
            bsize = struct.unpack_from("<H", gz, at + 4)[0]
        at += 4 + slen
    if bsize is None:
        return ("foreign",)
    size = bsize + 1
    if left < size:
        return ("short",)
    end = p + size
    for bit in (8, 16):
        if flg & bit:
            z = gz.find(b"\0", at, end)
            if z < 0:
                return ("foreign",)
            at = z + 1
    if flg & 2:
        at += 2
    if at + 1 + 8 > end:
        return ("foreign",)
    isize = struct.unpack_from("<I", gz, end - 4)[0]
    if isize > TEXT_MAX:
        return ("foreign",)
    return ("taken", size, at - p, isize)


def scan(gz, max_text=0, final=True):
    """pfq_gz_scan restated: (begin [n + 1], text_begin [n + 1], stop)."""
    assert max_text == 0 or max_text >= TEXT_MAX
    begin, text_begin, p, stop = [0], [0], 0, END
    while True:
        if p == len(gz):
            stop = END
            break
        w = walk(gz, p)
        if w[0] == "short":
            stop = FOREIGN if final else MORE
            break
        if w[0] == "foreign":
            stop = FOREIGN
            break
        text = text_begin[-1] + w[3]
        if (max_text and text > max_text) or text > (1 << 31) - 1:
            stop = LIMIT
            break
        p += w[1]
        begin.append(p)
        text_begin.append(text)
    return begin, text_begin, stop


def four_letter(n, seed):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)])


def fastq_like(n, seed):
    rng = np.random.default_rng(seed)
    out, i = [], 0
    while sum(map(len, out)) < n:
        L = int(rng.integers(30, 160))
        out.append(b"@read%d/1\n%s\n+\n%s\n" % (i, four_letter(L, seed * 1000 + i), bytes(rng.integers(35, 74, L).astype(np.uint8))))
        i += 1
    return b"".join(out)[:n]


def far_member(half):
    """zlib never looks back further than 32 768 - 262 bytes, so the member whose matches have the largest distance and length
    deflate allows is written by hand: one fixed-code block, `half` (32 768 bytes below 144) as literals, then 126 matches of
    length 258 at distance 32 768."""
    assert len(half) == 32768 and max(half) < 144
    bits = []
    code = lambda value, n: bits.extend((value >> (n - 1 - i)) & 1 for i in range(n))   # Huffman codes go most significant bit first
    plain = lambda value, n: bits.extend((value >> i) & 1 for i in range(n))            # everything else least significant first
    plain(1, 1), plain(1, 2)
    for c in half:
        code(0x30 + c, 8)
    for _ in range(126):
        code(0xC0 + 285 - 280, 8)                                                        # length 258, no extra bits
        code(29, 5), plain(32768 - 24577, 13)
    code(0, 7)
    bits.extend([0] * (-len(bits) % 8))
    text = half + (half * 2)[32768:32768 + 126 * 258]
    pay = bytes(np.packbits(np.array(bits, dtype=np.uint8), bitorder="little"))
    assert zlib.decompress(pay, -15) == text
    return text, frame(pay, len(text), zlib.crc32(text))


def zoo():
    """[(name, text, member)]: what the decoder has to get right."""
    rng = np.random.default_rng(1951)
    fq = fastq_like(BLOCK, 7)
    half = four_letter(32768, 3)
    out = []
    for level in (0, 1, 6, 9):
        out.append((f"level{level}", fq, member(fq, level)))
    same = b"G" * BLOCK
    for name, strategy in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        out.append((name + "_equal", same, member(same, 6, strategy)))
        out.append((name + "_fastq", fq[:20000], member(fq[:20000], 6, strategy)))
    noise = bytes(rng.integers(0, 256, BLOCK).astype(np.uint8))
    out.append(("random_stored", noise, member(noise, 6)))
    out.append(("full_flush", fq[:30000], member(fq[:30000], 6, flush_at=14321)))
    out.append(("empty", b"", member(b"")))
    out.append(("one_byte", b"A", member(b"A")))
    out.append(("one_byte_stored", b"\n", member(b"\n", 0)))
    out.append(("one_byte_fixed", b"\xff", member(b"\xff", 6, zlib.Z_FIXED)))
    far = (half + half)[:BLOCK]
    out.append(("distance_zlib_far", far, member(far, 9)))
    out.append(("distance_32768",) + far_member(half))
    out.append(("full_text", fq + fq[:TEXT_MAX - BLOCK], member(fq + fq[:TEXT_MAX - BLOCK], 6)))
    out.append(("with_header_parts", fq[:5000], member(fq[:5000], 6, before=[(b"XY", b"abc")], after=[(b"ZZ", b"")], fname=b"reads.fq",
                                                    fcomment=b"a comment", fhcrc=True)))
    assert member(b"") == EOF_MARKER
    return out


def payload_of(m):
    w = walk(m, 0)
    assert w[0] == "taken" and w[1] == len(m)
    return w[2], m[w[2]:len(m) - 8]


def corrupt_list():
    """[(name, original text, member)]: every single-bit flip in the first 64 payload bytes of a dynamic, a fixed and a stored
    member, every truncation of those payloads, a wrong ISIZE (both ways) and a wrong CRC.  Fixed: nothing here is random but
    the texts, which come from a fixed seed."""
    text = fastq_like(700, 11)
    noise = bytes(np.random.default_rng(12).integers(0, 256, 150).astype(np.uint8))
    bases = [("dynamic", text, member(text, 6)), ("fixed", text[:300], member(text[:300], 6, zlib.Z_FIXED)), ("stored", noise, member(noise, 0))]
    out = []
    for name, t, m in bases:
        h, pay = payload_of(m)
        assert len(pay) >= 64
        crc, n = zlib.crc32(t), len(t)
        for bit in range(64 * 8):
            p = bytearray(pay)
            p[bit >> 3] ^= 1 << (bit & 7)
            out.append((f"{name}_flip{bit}", t, frame(bytes(p), n, crc)))
        for cut in range(1, len(pay)):
            out.append((f"{name}_cut{cut}", t, frame(pay[:cut], n, crc)))
        out.append((f"{name}_isize_minus", t, frame(pay, n - 1, crc)))
        out.append((f"{name}_isize_plus", t, frame(pay, n + 1, crc)))
        out.append((f"{name}_crc", t, frame(pay, n, crc ^ 0x00010000)))
    return out


def zlib_says(m):
    """What zlib makes of a framed member's payload: its text, or None when it refuses it, stops early or leaves bytes over."""
    _, pay = payload_of(m)
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(pay)
    except zlib.error:
        return None
    if not d.eof or d.unused_data:
        return None
    crc, isize = struct.unpack("<II", m[-8:])
    return text if (len(text) == isize and zlib.crc32(text) == crc) else None
