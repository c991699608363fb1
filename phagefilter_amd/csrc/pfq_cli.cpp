// pfq_cli.cpp — `phage_filter query` on top of libpfq's C ABI: the process-level drop-in seam.
//
// Mirrors the query arm of the reference CLI (src/main.rs:100-135 flags, :249-376 flow, :380-404 helpers), the
// FASTA/FASTQ(.gz) ingest of src/file_parser.rs:33-101,:191-344 (bio 2.2.0 readers) and ResultMap
// (src/result_map.rs:9-46).  All classification work happens on the GPU through include/pfq.h; this file only
// parses text, keeps the reference's block bookkeeping and writes CLASSIFICATION.csv / POS_FILTERING.* /
// NEG_FILTERING.*.  `build` / `add` (main.rs:148-247) drive pfq_tree_create / pfq_tree_insert, the reference's greedy
// placement on the device; `build-balanced` makes the synthetic balanced tree of SURVEY §8d from a genome directory.
#include <dirent.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <climits>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <set>
#include <thread>
#include <string>
#include <unordered_map>
#include <string_view>
#include <vector>

#include <emmintrin.h>  // SSE2 (x86-64 baseline)
#include <functional>

#include "../../include/pfq.h"

namespace {

// dst[i] = ASCII upper case of src[i] (what `to_uppercase` does to a nucleotide string, main.rs:347-349), 16 bytes at a time
inline void copy_upper(char *dst, const uint8_t *src, size_t n) {
    const __m128i lo = _mm_set1_epi8('a' - 1), hi = _mm_set1_epi8('z' + 1), bit = _mm_set1_epi8(0x20);
    size_t i = 0;
    for (; i + 16 <= n; i += 16) {
        const __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src + i));
        const __m128i m = _mm_and_si128(_mm_cmpgt_epi8(v, lo), _mm_cmplt_epi8(v, hi));  // (bytes >= 0x80 are negative: no letters)
        _mm_storeu_si128(reinterpret_cast<__m128i *>(dst + i), _mm_sub_epi8(v, _mm_and_si128(m, bit)));
    }
    for (; i < n; ++i) {
        const uint8_t ch = src[i];
        dst[i] = (char)((ch >= 'a' && ch <= 'z') ? ch - 32 : ch);
    }
}

// fn(0), .., fn(n - 1) side by side: fn(0) on the calling thread, the others on threads of their own
template <class F>
void fan_out(size_t n, const F &fn) {
    std::vector<std::thread> th;
    for (size_t i = 1; i < n; ++i) th.emplace_back(std::cref(fn), i);
    fn(0);
    for (auto &t : th) t.join();
}

// die() off the main thread, and die_in_flight() anywhere, end the process WITHOUT exit(): exit() would run the atexit handlers
// and static destructors (the HIP runtime's among them) while the other threads are still inside HIP calls, which has ended
// such a run with a segmentation fault instead of the message's status.  Same message, same status.
const std::thread::id g_main_thread = std::this_thread::get_id();
[[noreturn]] void die_in_flight(const std::string &msg) {
    fprintf(stderr, "phage_filter: %s\n", msg.c_str());
    fflush(stderr);
    _exit(101);
}
[[noreturn]] void die(const std::string &msg) {  // the reference panics: message on stderr, exit code 101
    if (std::this_thread::get_id() != g_main_thread) die_in_flight(msg);
    fprintf(stderr, "phage_filter: %s\n", msg.c_str());
    exit(101);
}
void check(int rc) {
    if (rc != PFQ_OK) die(std::string("libpfq: ") + pfq_last_error());
}

// ---------------------------------------------------------------------------------------------------------------
// input files (file_parser.rs:303-344)
// ---------------------------------------------------------------------------------------------------------------
const char *SEQ_EXT[] = {"fa", "fasta", "fna", "fsa", "fas", "fq", "fastq"};
std::string ext_of(const std::string &p) {
    size_t slash = p.find_last_of('/');
    std::string base = slash == std::string::npos ? p : p.substr(slash + 1);
    size_t dot = base.find_last_of('.');
    if (dot == std::string::npos || dot == 0) return "";
    return base.substr(dot + 1);
}
std::string stem_of(const std::string &p) {
    size_t dot = p.find_last_of('.');
    return dot == std::string::npos ? p : p.substr(0, dot);
}
bool is_seq_ext(const std::string &e) {
    for (auto s : SEQ_EXT)
        if (e == s) return true;
    return false;
}
bool has_supported_extension(const std::string &path) {
    std::string e = ext_of(path);
    if (e.empty()) return false;
    if (is_seq_ext(e)) return true;
    if (e == "gz" || e == "gzip") return is_seq_ext(ext_of(stem_of(path)));
    return false;
}
// get_file_names: a file is taken as is; a directory contributes its entries with a supported extension.
// read_dir order is unspecified in the reference; here: sorted by name (and consumed from the back, like pop()).
std::vector<std::string> get_file_names(const std::string &path) {
    struct stat st;
    if (stat(path.c_str(), &st) != 0) die("cannot stat '" + path + "': " + strerror(errno));
    if (S_ISREG(st.st_mode)) return {path};
    std::vector<std::string> out;
    DIR *d = opendir(path.c_str());
    if (!d) die("cannot read directory '" + path + "'");
    while (dirent *e = readdir(d)) {
        std::string name = e->d_name;
        if (name == "." || name == "..") continue;
        std::string full = path + (path.back() == '/' ? "" : "/") + name;
        if (has_supported_extension(full)) out.push_back(full);
    }
    closedir(d);
    std::sort(out.begin(), out.end());
    return out;
}

enum class Fmt { Fasta, Fastq };
enum class FmtOverride { Auto, Fasta, Fastq };

Fmt format_from_extension(const std::string &path) {  // file_parser.rs:69-86
    std::string e = ext_of(path), low = e;
    for (auto &c : low) c = (char)tolower(c);
    std::string eff = (low == "gz" || low == "gzip") ? ext_of(stem_of(path)) : e;
    return (eff == "fq" || eff == "fastq") ? Fmt::Fastq : Fmt::Fasta;
}
Fmt detect_format(const std::string &path, FmtOverride ov) {  // file_parser.rs:33-66
    if (ov == FmtOverride::Fasta) return Fmt::Fasta;
    if (ov == FmtOverride::Fastq) return Fmt::Fastq;
    gzFile f = gzopen(path.c_str(), "rb");  // transparent for plain files, inflates gzip
    if (f) {
        int c = gzgetc(f);
        gzclose(f);
        if (c == '>') return Fmt::Fasta;
        if (c == '@') return Fmt::Fastq;
    }
    return format_from_extension(path);
}

// ---------------------------------------------------------------------------------------------------------------
// line sources: a (possibly gzip-compressed) stream, or a range of a memory-mapped plain file
// ---------------------------------------------------------------------------------------------------------------
// Lines are handed out as views (no per-line allocation); with GzLines a line that straddles a buffer refill is
// assembled in `carry`.  A view stays valid until the next call.
struct GzLines {
    gzFile f = nullptr;
    std::vector<char> buf;
    std::string carry;
    size_t pos = 0, len = 0;
    bool eof = false;
    explicit GzLines(const std::string &path) : buf(4 << 20) {
        f = gzopen(path.c_str(), "rb");
        if (!f) die("Failed to open '" + path + "': " + strerror(errno));
        gzbuffer(f, 1 << 20);
    }
    // The stream that begins at byte `offset` of the file (the begin of a gzip member), without its first `discard` bytes of text.
    GzLines(const std::string &path, uint64_t offset, uint64_t discard) : buf(4 << 20) {
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0 || lseek(fd, (off_t)offset, SEEK_SET) < 0 || !(f = gzdopen(fd, "rb"))) die("Failed to open '" + path + "': " + strerror(errno));
        gzbuffer(f, 1 << 20);
        while (discard) {
            const int got = gzread(f, buf.data(), (unsigned)std::min<uint64_t>(discard, buf.size()));
            if (got < 0) die_in_flight("read error (corrupt gzip?)");
            if (got == 0) break;
            discard -= (uint64_t)got;
        }
    }
    GzLines(const GzLines &) = delete;
    ~GzLines() {
        if (f) gzclose(f);
    }
    // One line without its '\n' as [p, p+n); false at end of file with nothing read.
    bool next(const char *&p, size_t &n) {
        bool use_carry = false;
        while (true) {
            if (pos == len) {
                if (eof) {
                    if (use_carry) { p = carry.data(); n = carry.size(); return true; }
                    return false;
                }
                int got = gzread(f, buf.data(), (unsigned)buf.size());
                if (got < 0) die_in_flight("read error (corrupt gzip?)");
                if (got == 0) { eof = true; continue; }
                pos = 0;
                len = (size_t)got;
            }
            const char *b = buf.data() + pos;
            const char *nl = (const char *)memchr(b, '\n', len - pos);
            if (nl) {
                if (use_carry) {
                    carry.append(b, nl - b);
                    p = carry.data();
                    n = carry.size();
                } else {
                    p = b;
                    n = (size_t)(nl - b);
                }
                pos += (size_t)(nl - b) + 1;
                return true;
            }
            if (!use_carry) { carry.clear(); use_carry = true; }
            carry.append(b, len - pos);
            pos = len;
        }
    }
    bool drained() const { return eof && pos == len; }
    uint64_t tell() const { return 0; }  // positions are only used with MemLines
};
struct MemLines {
    const char *base, *cur, *end;
    MemLines(const char *b, uint64_t from, uint64_t to) : base(b), cur(b + from), end(b + to) {}
    bool next(const char *&p, size_t &n) {
        if (cur == end) return false;
        const char *nl = (const char *)memchr(cur, '\n', (size_t)(end - cur));
        p = cur;
        if (nl) {
            n = (size_t)(nl - cur);
            cur = nl + 1;
        } else {
            n = (size_t)(end - cur);
            cur = end;
        }
        return true;
    }
    bool drained() const { return false; }
    uint64_t tell() const { return (uint64_t)(cur - base); }
};

// Bases and offsets of a batch go to the GPU as they are; when a tree is open their buffers are page-locked
// (pfq_host_alloc) so that the copy runs at PCIe rate.  Small blocks and the CPU-only subcommands use malloc.
bool g_pinned = false;  // set once, before the first batch is allocated
template <class T>
struct HostAlloc {
    using value_type = T;
    HostAlloc() = default;
    template <class U>
    HostAlloc(const HostAlloc<U> &) {}
    static bool pinned(size_t n) { return g_pinned && n * sizeof(T) >= (1u << 20); }
    // resize() without a fill: new elements are default-initialised (bytes and offsets are overwritten right away)
    template <class U>
    void construct(U *p) { ::new ((void *)p) U; }
    template <class U, class A0, class... A>
    void construct(U *p, A0 &&a0, A &&...a) { ::new ((void *)p) U(std::forward<A0>(a0), std::forward<A>(a)...); }
    T *allocate(size_t n) {
        void *p = nullptr;
        if (pinned(n)) {
            if (pfq_host_alloc(n * sizeof(T), &p) != PFQ_OK) die(std::string("libpfq: ") + pfq_last_error());
        } else if (!(p = malloc(n * sizeof(T)))) throw std::bad_alloc();
        return (T *)p;
    }
    void deallocate(T *p, size_t n) {
        if (pinned(n)) pfq_host_free(p);
        else free(p);
    }
    template <class U>
    bool operator==(const HostAlloc<U> &) const { return true; }
    template <class U>
    bool operator!=(const HostAlloc<U> &) const { return false; }
};

inline size_t trimmed_len(const char *p, size_t n) {  // str::trim_end
    while (n && isspace((unsigned char)p[n - 1])) --n;
    return n;
}

// One block of reads in the layout the C ABI takes (concatenated bases + n+1 offsets); ids and qualities are kept
// only when POS/NEG filtering needs them (the reference drops them otherwise too, file_parser.rs:202-204,217-220).
struct Segment;
struct Batch {
    std::vector<uint8_t, HostAlloc<uint8_t>> seq;
    std::vector<uint64_t, HostAlloc<uint64_t>> off{0};
    std::vector<char> id_bytes;       // concatenated ids (bio Record::id()) when kept
    std::vector<uint64_t> id_off{0};
    std::vector<char> qual;           // concatenated qualities when kept (bio does not require |qual| == |seq|)
    std::vector<uint64_t> qual_off{0};
    std::vector<uint8_t> has_qual;    // per read
    // A batch assembled for POS/NEG filtering copies only what the device needs (the bases): ids and qualities stay in the
    // parsed segments, which the batch holds until it has been written (append_ref).
    bool external = false;
    std::vector<std::string_view> ext_id, ext_qual;
    std::vector<Segment *> held;
    size_t n() const { return off.size() - 1; }
    void clear() {
        seq.clear();
        off.assign(1, 0);
        id_bytes.clear();
        id_off.assign(1, 0);
        qual.clear();
        qual_off.assign(1, 0);
        has_qual.clear();
        ext_id.clear();
        ext_qual.clear();
        external = false;
    }
    std::string_view quality(size_t r) const {
        return external ? ext_qual[r] : std::string_view(qual.data() + qual_off[r], qual_off[r + 1] - qual_off[r]);
    }
    std::string_view id(size_t r) const {
        return external ? ext_id[r] : std::string_view(id_bytes.data() + id_off[r], id_off[r + 1] - id_off[r]);
    }
    // Record::id(): header[1..].trim_end() up to the first separator — any whitespace in bio's FASTA reader
    // (`splitn(2, char::is_whitespace)`), a blank only in its FASTQ reader (`splitn(2, ' ')`)
    void push_id(const char *h, size_t n, bool fastq) {
        n = trimmed_len(h, n);
        size_t i = 1;
        while (i < n && !(fastq ? h[i] == ' ' : isspace((unsigned char)h[i]))) ++i;
        if (i > 1) id_bytes.insert(id_bytes.end(), h + 1, h + i);
        id_off.push_back(id_bytes.size());
    }
    // reads [r0, r1) of `o` appended to this batch
    void append(const Batch &o, size_t r0, size_t r1, bool keep) {
        auto copy_seq = [&] {
            const uint64_t s0 = o.off[r0], s1 = o.off[r1], base = seq.size();
            seq.insert(seq.end(), o.seq.begin() + s0, o.seq.begin() + s1);
            for (size_t r = r0 + 1; r <= r1; ++r) off.push_back(base + (o.off[r] - s0));
        };
        if (!keep) {
            copy_seq();
            return;
        }
        auto copy_qual = [&] {
            const uint64_t q0 = o.qual_off[r0], q1 = o.qual_off[r1], qb = qual.size();
            qual.insert(qual.end(), o.qual.begin() + q0, o.qual.begin() + q1);
            for (size_t r = r0 + 1; r <= r1; ++r) qual_off.push_back(qb + (o.qual_off[r] - q0));
        };
        // sequences, qualities and ids are separate arrays: large pieces are copied side by side (the assembler thread was
        // the slowest stage of the filtering pipeline: 10 GB of records through one core)
        const bool big = r1 - r0 >= 4096;
        std::thread ts, tq;
        if (big) {
            ts = std::thread(copy_seq);
            tq = std::thread(copy_qual);
        } else {
            copy_seq();
            copy_qual();
        }
        const uint64_t i0 = o.id_off[r0], i1 = o.id_off[r1], ib = id_bytes.size();
        id_bytes.insert(id_bytes.end(), o.id_bytes.begin() + i0, o.id_bytes.begin() + i1);
        for (size_t r = r0 + 1; r <= r1; ++r) id_off.push_back(ib + (o.id_off[r] - i0));
        has_qual.insert(has_qual.end(), o.has_qual.begin() + r0, o.has_qual.begin() + r1);
        if (big) {
            ts.join();
            tq.join();
        }
    }
    // reads [r0, r1) of `o`: bases copied, ids and qualities referenced (the caller keeps `o` alive, see `held`).  Large
    // pieces are handled by four threads side by side: the arrays are sized first, every thread fills its range of reads.
    void append_ref(const Batch &o, size_t r0, size_t r1) {
        external = true;
        const size_t n0 = n(), cnt = r1 - r0;
        const uint64_t s0 = o.off[r0], s1 = o.off[r1], base = seq.size();
        seq.resize(base + (s1 - s0));
        off.resize(n0 + 1 + cnt);
        ext_id.resize(n0 + cnt);
        ext_qual.resize(n0 + cnt);
        has_qual.resize(n0 + cnt);
        auto part = [&](size_t a, size_t b) {  // reads [a, b) of the piece
            memcpy(seq.data() + base + (o.off[r0 + a] - s0), o.seq.data() + o.off[r0 + a], o.off[r0 + b] - o.off[r0 + a]);
            for (size_t i = a; i < b; ++i) {
                off[n0 + 1 + i] = base + (o.off[r0 + i + 1] - s0);
                ext_id[n0 + i] = o.id(r0 + i);
                ext_qual[n0 + i] = o.quality(r0 + i);
                has_qual[n0 + i] = o.has_qual[r0 + i];
            }
        };
        const size_t T = cnt >= 16384 ? 4 : 1;
        fan_out(T, [&](size_t t) { part(cnt * t / T, cnt * (t + 1) / T); });
    }
};

// bio 2.2.0 `io::fasta::Reader::read` / `io::fastq::Reader::read` as the reference consumes them through
// `.records()` + `unwrap()` (file_parser.rs:191-224; no `Record::check()`), appending straight into a Batch:
//   FASTA: header line must start with '>'; every following line up to the next '>' line is sequence, trimmed at
//          the end;
//   FASTQ: header line must start with '@'; lines up to the first '+' line are sequence (trimmed, counted); then
//          the SAME NUMBER of lines is read as quality (trimmed); an empty quality is `IncompleteRecord`.  Lengths
//          of sequence and quality are not compared (that is `check()`, which the reference never calls).
// bio is a crates.io dependency that is not vendored in the reference: multi-line and malformed-record behaviour is
// restated from its published source, parity unpinned; the reference's own parser tests (file_parser.rs:410-604)
// only hold ordinary four-line records, which every reading of the rules agrees on.  Malformed input is reported through `err` (the caller decides when
// it becomes fatal: a speculative parse from a guessed record boundary must not kill the process).
template <class Src>
struct RecordParser {
    Src &lr;
    Fmt fmt;
    std::string header, pending;  // pending: a header line already consumed while finishing the previous FASTA record
    bool have_pending = false;
    uint64_t pending_pos = 0;     // where that line starts (MemLines)
    std::string err;
    RecordParser(Src &s, Fmt f) : lr(s), fmt(f) {}
    // Position at which the next record starts (MemLines only).
    uint64_t next_record_pos() const { return have_pending ? pending_pos : lr.tell(); }
    // 1: a record was appended; 0: clean end of input; -1: malformed (message in err)
    int next(Batch &b, bool keep) {
        const char *p;
        size_t n;
        if (have_pending) {
            header.swap(pending);
            have_pending = false;
        } else {
            if (!lr.next(p, n)) return 0;
            if (n == 0 && lr.drained()) return 0;
            header.assign(p, n);
        }
        const size_t seq0 = b.seq.size();
        if (fmt == Fmt::Fasta) {
            if (header.empty() || header[0] != '>') { err = "FASTA: Expected > at record start."; return -1; }
            while (true) {
                const uint64_t at = lr.tell();
                if (!lr.next(p, n)) break;
                if (n && p[0] == '>') {
                    pending.assign(p, n);
                    have_pending = true;
                    pending_pos = at;
                    break;
                }
                n = trimmed_len(p, n);
                b.seq.insert(b.seq.end(), p, p + n);
            }
            b.off.push_back(b.seq.size());
            if (keep) {
                b.push_id(header.data(), header.size(), false);
                b.qual_off.push_back(b.qual.size());
                b.has_qual.push_back(0);
            }
            return 1;
        }
        if (header.empty() || header[0] != '@') { err = "FASTQ: Expected @ at record start."; return -1; }
        size_t lines_read = 0;
        while (lr.next(p, n)) {
            if (n && p[0] == '+') break;
            n = trimmed_len(p, n);
            b.seq.insert(b.seq.end(), p, p + n);
            ++lines_read;
        }
        const size_t q0 = b.qual.size();
        size_t qlen = 0;
        for (size_t i = 0; i < lines_read; ++i) {
            if (!lr.next(p, n)) break;  // read_line at end of file: nothing appended
            n = trimmed_len(p, n);
            if (keep) b.qual.insert(b.qual.end(), p, p + n);
            qlen += n;
        }
        if (qlen == 0) {
            b.seq.resize(seq0);
            b.qual.resize(q0);
            err = "FASTQ: Incomplete record.";
            return -1;
        }
        b.off.push_back(b.seq.size());
        if (keep) {
            b.push_id(header.data(), header.size(), true);
            b.qual_off.push_back(b.qual.size());
            b.has_qual.push_back(1);
        }
        return 1;
    }
};

// ---------------------------------------------------------------------------------------------------------------
// ReadQueue (file_parser.rs:227-301): files consumed from the back of the list, records streamed across files.
//
// At 10^8 reads/s the text is the end-to-end limiter, so parsing is spread over `threads` workers:
//   * a plain file is memory-mapped and cut into chunks; every chunk is parsed on its own from the first record
//     start at or after its nominal begin to the first record start at or after its nominal end.  A FASTA record
//     start is any line beginning with '>' (exact); a FASTQ record start is guessed ('@' line followed by two
//     well-formed records) and then PROVEN by the consumer: chunk i+1 is accepted only if it starts exactly where
//     chunk i ended, which by induction from offset 0 makes every accepted start a true one.  A chunk that fails the
//     check is re-parsed from the proven position, so the result never depends on the guess;
//   * a gzip file is inflated and parsed by one worker as a stream of segments; several files run concurrently;
//   * --device-inflate: a blocked gzip file is cut into chunks of whole members by a walk over the members' headers
//     (bgzf_tasks); the workers only read them, the device inflates and parses (Query::counts_only_text).
// Segments are consumed strictly in input order, so blocks, ids and outputs are those of a sequential reader.
// ---------------------------------------------------------------------------------------------------------------
// A page-locked buffer (pfq_host_alloc) that only grows; --device-parse reads file bytes into it for pfq_text_parse.
struct PinnedBuf {
    char *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    ~PinnedBuf() {
        if (p) pfq_host_free(p);
    }
    char *ensure(size_t n) {
        if (n > cap) {
            if (p) pfq_host_free(p);
            p = nullptr;
            cap = 0;
            void *q = nullptr;
            if (pfq_host_alloc(n + n / 8, &q) != PFQ_OK) die(std::string("libpfq: ") + pfq_last_error());
            p = (char *)q;
            cap = n + n / 8;
        }
        return p;
    }
};
struct Segment {
    Batch b;
    std::atomic<int> refs{0};             // the consumer + every batch that references the segment's ids / qualities
    std::vector<char> raw;                // plain chunks: the bytes of the file the records were parsed from
    uint64_t start_pos = 0, end_pos = 0;  // plain chunks: first record start, start of the record after the last one
    std::string err;                      // malformed input met after the records in b
    bool last = true;                     // gzip streams: more segments of this task follow when false
    // --device-parse: a plain chunk as bytes [text_lo, text_hi) of the file, not parsed; start_pos is the guessed record start
    PinnedBuf text;
    uint64_t text_lo = 0, text_hi = 0;
    bool is_text = false;
    // --device-inflate: a chunk of whole blocked-gzip members as bytes [text_lo, text_hi) of the file, not inflated
    bool is_gz = false;
};
struct MappedFile {  // (plain files are read with pread into reused buffers: first-touch page faults of a mapping
    uint64_t size = 0;   //  cost more than the copy, and serialise the workers)
    int fd = -1;
    bool gz = false;
};
// bytes [lo, hi) of a file held in memory; p is the address byte 0 of the file would have
struct FileView {
    const char *p;
    uint64_t lo, hi;
};
struct Task {
    int file = 0;
    uint64_t lo = 0, hi = 0;  // nominal byte range of a plain chunk
    bool stream = false;      // gzip file: one streaming task
    bool bgzf = false;        // --device-inflate: whole members [lo, hi) of a blocked gzip file
    bool bgzf_tail = false;   // ... the header walk ended at lo short of the file's end: what follows is for the host reader
    bool last_of_file = false;
    std::deque<Segment *> out;
    bool taken = false;
};

struct ReadQueue {
    std::vector<std::string> files;   // consumption order (the reference pops from the back of its list)
    std::vector<Fmt> fmts;
    std::vector<MappedFile> maps;
    std::vector<Task> tasks;
    FmtOverride ov;
    bool keep = false;
    unsigned n_threads = 1;
    uint64_t chunk_bytes = 32ull << 20, seg_reads = 1u << 18;
    size_t lookahead = 8;
    bool device_parse = false;        // --device-parse: the workers only read the plain chunks (read_raw), the consumer parses
    std::unique_ptr<std::atomic<bool>[]> file_slow;  // ... until a file turned out not to be ordinary: its later chunks are parsed here
    bool device_inflate = false;      // --device-inflate: blocked gzip files are cut into chunks of whole members, which the workers only read
    std::vector<uint64_t> bgzf_members;  // per file: the members the header walk found (0: not read as chunks)

    std::mutex mu;
    std::condition_variable cv_work, cv_out;
    size_t next_task = 0, consume_task = 0;
    bool stop = false, started = false;
    std::vector<std::thread> workers;

    std::vector<Segment *> pool;  // consumed segments, handed back to the workers with their (warm) buffers
    Segment *cur = nullptr;  // segment being consumed
    size_t cur_read = 0;
    bool have_proven = false;
    uint64_t proven_pos = 0;  // plain files: where the next record of the current file provably starts

    ReadQueue(const std::string &path, FmtOverride o) : ov(o) {
        files = get_file_names(path);
        std::reverse(files.begin(), files.end());
        for (auto &f : files) fmts.push_back(detect_format(f, ov));
    }
    ~ReadQueue() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_work.notify_all();
        cv_out.notify_all();
        for (auto &t : workers) t.join();
        delete cur;
        for (auto *s : pool) delete s;
        for (auto &t : tasks)
            for (auto *s : t.out) delete s;
        for (auto &m : maps)
            if (m.fd >= 0) close(m.fd);
    }
    Fmt peek_format() const { return files.empty() ? Fmt::Fasta : fmts.front(); }

    void start(bool keep_ids, unsigned threads) {
        keep = keep_ids;
        n_threads = std::max(1u, threads);
        if (!keep) {  // counts only: a segment is one device call, which wants >= 2^18 reads (bucketed path)
            chunk_bytes = 128ull << 20;
            seg_reads = 1u << 19;
        }
        if (const char *e = getenv("PFQ_INGEST_CHUNK_BYTES")) chunk_bytes = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
        if (const char *e = getenv("PFQ_INGEST_SEGMENT_READS")) seg_reads = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
        lookahead = (size_t)n_threads + 2;
        for (size_t i = 0; i < files.size(); ++i) {
            MappedFile m;
            m.fd = open(files[i].c_str(), O_RDONLY);
            if (m.fd < 0) die("Failed to open '" + files[i] + "': " + strerror(errno));
            struct stat st;
            if (fstat(m.fd, &st) != 0) die("cannot stat '" + files[i] + "'");
            m.size = (uint64_t)st.st_size;
            unsigned char magic[2] = {0, 0};
            m.gz = pread(m.fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
            if (!m.gz) posix_fadvise(m.fd, 0, 0, POSIX_FADV_SEQUENTIAL);
            maps.push_back(m);
            bgzf_members.push_back(0);
            if (m.gz && device_inflate && bgzf_tasks(i, m)) continue;
            if (m.gz) {
                Task t;
                t.file = (int)i;
                t.stream = true;
                tasks.push_back(std::move(t));
            } else {
                for (uint64_t lo = 0; lo < std::max<uint64_t>(m.size, 1); lo += chunk_bytes) {
                    Task t;
                    t.file = (int)i;
                    t.lo = lo;
                    t.hi = std::min(m.size, lo + chunk_bytes);
                    tasks.push_back(std::move(t));
                }
            }
        }
        file_slow.reset(new std::atomic<bool>[files.size() + 1]);
        for (size_t i = 0; i < files.size(); ++i) file_slow[i] = false;
        started = true;
        for (unsigned i = 0; i < n_threads; ++i) workers.emplace_back([this] { work(); });
    }

    // --device-inflate: the size of the blocked-gzip member whose header begins at byte p, from its 'BC' extra subfield, or 0 if
    // the bytes there are no such header or the member would pass the file's end.  Only the header is read.
    static uint64_t bgzf_member_size(const MappedFile &m, uint64_t p, std::vector<unsigned char> &extra) {
        unsigned char h[12];
        if (p + 12 > m.size || pread(m.fd, h, 12, (off_t)p) != 12) return 0;
        if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4) || (h[3] & 0xe0)) return 0;
        const size_t xlen = (size_t)h[10] | (size_t)h[11] << 8;
        extra.resize(xlen + 1);
        if (p + 12 + xlen > m.size || pread(m.fd, extra.data(), xlen, (off_t)(p + 12)) != (ssize_t)xlen) return 0;
        for (size_t at = 0; at + 4 <= xlen;) {
            const size_t slen = (size_t)extra[at + 2] | (size_t)extra[at + 3] << 8;
            if (at + 4 + slen > xlen) return 0;
            if (extra[at] == 'B' && extra[at + 1] == 'C' && slen == 2) {
                const uint64_t size = ((uint64_t)extra[at + 4] | (uint64_t)extra[at + 5] << 8) + 1;
                return (size >= 12 + xlen + 9 && p + size <= m.size) ? size : 0;
            }
            at += 4 + slen;
        }
        return 0;
    }
    // The chunk tasks of a blocked gzip file: whole members, at least chunk_bytes of compressed bytes each, cut by a walk over
    // the headers; false if the file's first member is not one pfq_gz_scan takes (the file then keeps its streaming task).
    bool bgzf_tasks(size_t file, const MappedFile &m) {
        std::vector<unsigned char> head((size_t)std::min<uint64_t>(m.size, 65536));
        if (pread(m.fd, head.data(), head.size(), 0) != (ssize_t)head.size()) return false;
        pfq_gz_members first{};
        if (pfq_gz_scan(head.data(), head.size(), 0, head.size() == m.size ? PFQ_TEXT_FINAL : 0u, &first) != PFQ_OK || !first.n_members) return false;
        const uint64_t cut = std::min<uint64_t>(chunk_bytes, 1ull << 28);  // (a chunk's text must stay below 2^31 bytes)
        std::vector<unsigned char> extra;
        uint64_t lo = 0, p = 0, n = 0;
        while (p < m.size) {
            const uint64_t size = bgzf_member_size(m, p, extra);
            if (!size) break;
            p += size;
            ++n;
            if (p - lo >= cut || p == m.size) {
                Task t;
                t.file = (int)file;
                t.lo = lo;
                t.hi = p;
                t.bgzf = true;
                t.last_of_file = p == m.size;
                tasks.push_back(std::move(t));
                lo = p;
            }
        }
        if (p < m.size) {  // the walk ended early: the members up to here, then a task that only hands the rest to the host reader
            Task t;
            t.file = (int)file;
            t.bgzf = true;
            if (p > lo) {
                t.lo = lo;
                t.hi = p;
                tasks.push_back(t);
            }
            t.lo = t.hi = p;
            t.bgzf_tail = t.last_of_file = true;
            tasks.push_back(std::move(t));
        }
        bgzf_members[file] = n;
        posix_fadvise(m.fd, 0, 0, POSIX_FADV_SEQUENTIAL);
        return true;
    }
    // A chunk of whole members as it is in the file, in page-locked memory; nothing is inflated.
    void read_gz(const MappedFile &m, uint64_t lo, uint64_t hi, Segment &s) {
        s.b.clear();
        s.err.clear();
        s.text_lo = s.text_hi = lo;
        s.is_gz = true;
        if (hi == lo || file_slow_of(m)) return;
        read_range(m, s.text.ensure((size_t)(hi - lo)), lo, hi);
        s.text_hi = hi;
    }
    bool file_slow_of(const MappedFile &m) const { return file_slow[&m - maps.data()]; }

    // ---- chunk parsing ----------------------------------------------------------------------------------------
    // First record start at or after `from` (a line start) inside the view, or v.hi when there is none.
    uint64_t find_record_start(const FileView &v, Fmt fmt, uint64_t from) const {
        if (from == 0) return 0;
        uint64_t pos = from;
        if (v.p[pos - 1] != '\n') {  // not a line start: move to the next one
            const char *nl = (const char *)memchr(v.p + pos, '\n', v.hi - pos);
            if (!nl) return v.hi;
            pos = (uint64_t)(nl - v.p) + 1;
        }
        const char marker = fmt == Fmt::Fasta ? '>' : '@';
        while (pos < v.hi) {
            if (v.p[pos] == marker) {
                if (fmt == Fmt::Fasta) return pos;
                // FASTQ: '@' also starts quality lines; take the candidate if two records parse from it
                MemLines ml(v.p, pos, v.hi);
                RecordParser<MemLines> rp(ml, fmt);
                Batch scratch;
                int ok = rp.next(scratch, false);
                if (ok == 1) ok = rp.next(scratch, false);
                if (ok >= 0) return pos;  // (0: the file ends after the first record)
            }
            const char *nl = (const char *)memchr(v.p + pos, '\n', v.hi - pos);
            if (!nl) return v.hi;
            pos = (uint64_t)(nl - v.p) + 1;
        }
        return v.hi;
    }
    // Records starting in [start, nominal_end), parsed out of the view; returns whether the parser ran into the end of
    // the view (the caller reads more of the file and parses again unless the view ends where the file does).
    bool parse_view(const FileView &v, Fmt fmt, uint64_t start, uint64_t nominal_end, Segment &s) const {
        s.start_pos = start;
        if (nominal_end > start) {  // one allocation per buffer instead of a doubling series
            const uint64_t span = nominal_end - start;
            s.b.seq.reserve(span / (fmt == Fmt::Fastq ? 2 : 1) + 4096);
            s.b.off.reserve(span / 64 + 16);
        }
        MemLines ml(v.p, std::min(start, v.hi), v.hi);
        RecordParser<MemLines> rp(ml, fmt);
        while (rp.next_record_pos() < nominal_end) {
            int rc = rp.next(s.b, keep);
            if (rc == 0) break;
            if (rc < 0) {
                s.err = rp.err;
                break;
            }
        }
        s.end_pos = rp.next_record_pos();
        return ml.cur == ml.end;
    }
    // Chunk [lo, hi) of a plain file: records from the first record start at or after `lo` (or from `forced_start` when
    // the consumer knows it) up to the first record start at or after `hi`.
    void parse_chunk(const MappedFile &m, Fmt fmt, uint64_t lo, uint64_t hi, bool forced, uint64_t forced_start, Segment &s) {
        if (!m.size) return;
        const uint64_t want_lo = forced ? std::min(forced_start, m.size) : (lo ? lo - 1 : 0);
        for (uint64_t extra = 1ull << 20;; extra *= 8) {
            const uint64_t r_hi = std::min(m.size, std::max(hi, want_lo) + extra);
            s.raw.resize((size_t)(r_hi - want_lo));
            read_range(m, s.raw.data(), want_lo, r_hi);
            const FileView v{(const char *)((uintptr_t)s.raw.data() - (uintptr_t)want_lo), want_lo, r_hi};
            s.b.clear();
            s.err.clear();
            const uint64_t t0 = now_ns();
            const uint64_t start = forced ? forced_start : find_record_start(v, fmt, lo);
            const uint64_t t1 = now_ns();
            const bool hit_end = parse_view(v, fmt, start, hi, s);
            ns_find += t1 - t0;
            ns_parse += now_ns() - t1;
            if (!hit_end || r_hi == m.size) return;  // otherwise the last record may be cut: read further
        }
    }
    // --device-parse: chunk [lo, hi) of a plain file as bytes [lo - 1, hi + 1 MiB) in page-locked memory and the guessed start
    // of its first record; nothing is parsed.
    void read_raw(const MappedFile &m, Fmt fmt, uint64_t lo, uint64_t hi, Segment &s) {
        const uint64_t want_lo = lo ? lo - 1 : 0, r_hi = std::min<uint64_t>(m.size, hi + (1ull << 20));
        char *buf = s.text.ensure((size_t)(r_hi - want_lo));
        read_range(m, buf, want_lo, r_hi);
        const FileView v{(const char *)((uintptr_t)buf - (uintptr_t)want_lo), want_lo, r_hi};
        s.b.clear();
        s.err.clear();
        const uint64_t t0 = now_ns();
        s.start_pos = find_record_start(v, fmt, lo);
        ns_find += now_ns() - t0;
        s.end_pos = s.start_pos;
        s.text_lo = want_lo;
        s.text_hi = r_hi;
        s.is_text = true;
    }
    static void read_range(const MappedFile &m, char *buf, uint64_t lo, uint64_t hi) {
        for (uint64_t got = 0; got < hi - lo;) {
            ssize_t n = pread(m.fd, buf + got, (size_t)(hi - lo - got), (off_t)(lo + got));
            if (n < 0) die(std::string("read error: ") + strerror(errno));
            if (n == 0) die("input file shrank while it was being read");
            got += (uint64_t)n;
        }
    }
    Segment *fresh_segment() {
        Segment *s = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!pool.empty()) {
                s = pool.back();
                pool.pop_back();
            }
        }
        if (!s) return new Segment;
        s->b.clear();
        s->start_pos = s->end_pos = 0;
        s->err.clear();
        s->last = true;
        s->is_text = false;
        s->is_gz = false;
        return s;
    }
    // segments the pool takes back (filtering: batches in flight hold their segments)
    size_t pool_cap() const { return lookahead + 4 + (keep ? 48 : 0); }
    // a consumed segment back to the pool (one that ends in malformed input is not reused)
    void recycle(Segment *s) {
        if (!s->err.empty()) {
            delete s;
            return;
        }
        std::lock_guard<std::mutex> lk(mu);
        if (pool.size() < pool_cap()) pool.push_back(s);
        else delete s;
    }
    // one holder less; the last one hands the segment back
    void release(Segment *s) {
        if (--s->refs == 0) recycle(s);
    }
    void release_held(Batch &b) {
        for (Segment *s : b.held) release(s);
        b.held.clear();
    }
    void push(Task &t, Segment *s) {
        {
            std::lock_guard<std::mutex> lk(mu);
            t.out.push_back(s);
        }
        cv_out.notify_all();
    }
    void work() {
        while (true) {
            size_t ti;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return stop || (next_task < tasks.size() && next_task < consume_task + lookahead); });
                if (stop) return;
                ti = next_task++;
            }
            Task &t = tasks[ti];
            const MappedFile &m = maps[t.file];
            const Fmt fmt = fmts[t.file];
            if (!t.stream) {
                Segment *s = fresh_segment();
                if (t.bgzf) read_gz(m, t.lo, t.hi, *s);
                else if (device_parse && m.size && !file_slow[t.file]) read_raw(m, fmt, t.lo, t.hi, *s);
                else parse_chunk(m, fmt, t.lo, t.hi, false, 0, *s);
                push(t, s);
                continue;
            }
            GzLines gl(files[t.file]);
            RecordParser<GzLines> rp(gl, fmt);
            while (true) {
                Segment *s = fresh_segment();
                int rc = 1;
                while (s->b.n() < seg_reads && (rc = rp.next(s->b, keep)) == 1) {}
                if (rc < 0) s->err = rp.err;
                s->last = rc != 1;
                {
                    std::unique_lock<std::mutex> lk(mu);  // bounded: at most four segments of a stream wait
                    cv_work.wait(lk, [&] { return stop || t.out.size() < 4; });
                    if (stop) {
                        delete s;
                        return;
                    }
                    t.out.push_back(s);
                }
                cv_out.notify_all();
                if (rc != 1) break;
            }
        }
    }

    // ---- ordered consumption ----------------------------------------------------------------------------------
    // Next segment in input order (validated), or nullptr at the end of the input.
    Segment *next_segment() {
        const Task *t = nullptr;
        Segment *s = pop_segment(t);
        if (s) validate(*t, *s);
        return s;
    }
    // The two halves of next_segment: the next segment in input order as the workers left it, and the proof of a plain chunk's
    // start.  --device-parse takes segments on several threads and proves them one after the other, in the order taken.
    Segment *pop_segment(const Task *&task) {
        while (consume_task < tasks.size()) {
            Task &t = tasks[consume_task];
            Segment *s;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_out.wait(lk, [&] { return !t.out.empty(); });
                s = t.out.front();
                t.out.pop_front();
                if (s->last) ++consume_task;
            }
            cv_work.notify_all();
            task = &t;
            return s;
        }
        return nullptr;
    }
    uint64_t expected_start(const Task &t) const { return t.lo == 0 ? 0 : proven_pos; }
    void validate(const Task &t, Segment &s) {
        if (t.stream) return;
        const MappedFile &m = maps[t.file];
        const uint64_t expect = expected_start(t);
        if (m.size && (s.is_text || s.start_pos != expect)) {  // guessed boundary was wrong (or a record spans chunks): redo
            parse_chunk(m, fmts[t.file], t.lo, t.hi, true, expect, s);
            s.is_text = false;
        }
        proven_pos = s.end_pos;
    }
    // Appends up to max_reads reads (and at most ~max_bytes bases); false when the input is exhausted.
    // by_ref (needs keep): ids and qualities are referenced, not copied — the batch holds the segments (release_held).
    bool fill(Batch &b, uint64_t max_reads, uint64_t max_bytes, bool by_ref = false) {
        if (!started) die("ReadQueue::start was not called");
        while (b.n() < max_reads && b.seq.size() < max_bytes) {
            if (!cur) {
                const uint64_t t0 = now_ns();
                cur = next_segment();
                ns_wait += now_ns() - t0;
                cur_read = 0;
                if (!cur) return false;
                cur->refs = 1;  // this consumer
            }
            const size_t avail = cur->b.n() - cur_read;
            size_t take = (size_t)std::min<uint64_t>(avail, max_reads - b.n());
            if (take && max_bytes != ~0ull) {  // keep the byte bound (coarsely: per read)
                size_t t = 0;
                while (t < take && b.seq.size() + (cur->b.off[cur_read + t] - cur->b.off[cur_read]) < max_bytes) ++t;
                take = std::max<size_t>(t, 1);
            }
            const uint64_t t0 = now_ns();
            if (take && keep && by_ref) {
                b.append_ref(cur->b, cur_read, cur_read + take);
                if (b.held.empty() || b.held.back() != cur) {
                    b.held.push_back(cur);
                    ++cur->refs;
                }
            } else if (take) b.append(cur->b, cur_read, cur_read + take, keep);
            ns_append += now_ns() - t0;
            cur_read += take;
            if (cur_read == cur->b.n()) {
                if (!cur->err.empty()) {
                    pending_error = cur->err;
                    release(cur);
                    cur = nullptr;
                    return false;
                }
                release(cur);
                cur = nullptr;
            }
        }
        return true;
    }
    std::string pending_error;  // malformed input reached: fatal once the reads before it have been processed

    // PFQ_INGEST_TIMING=1: where the wall time of the reader went (stderr)
    std::atomic<uint64_t> ns_parse{0}, ns_find{0}, ns_wait{0}, ns_append{0};
    static uint64_t now_ns() {
        return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    void report_timing() const {
        if (!getenv("PFQ_INGEST_TIMING")) return;
        fprintf(stderr, "ingest: %u workers, parse %.3f s (sum over workers), boundary search %.3f s, consumer waited %.3f s, appended %.3f s\n",
                n_threads, ns_parse.load() * 1e-9, ns_find.load() * 1e-9, ns_wait.load() * 1e-9, ns_append.load() * 1e-9);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// paired-end input: two streams whose records are mates by index (--reads2), or one stream of adjacent mates
// (--interleaved).  Fragments come out as batches of records 2i (R1) and 2i + 1 (R2), what PFQ_PAIRED takes.
// ---------------------------------------------------------------------------------------------------------------
struct PairSource {
    ReadQueue &q1;
    ReadQueue *q2;        // nullptr: interleaved (mates are records 2i, 2i + 1 of q1)
    Batch b1, b2;
    uint64_t n_pairs = 0;  // fragments handed out so far
    std::string err;       // fatal, once the fragments before it have been processed
    bool done = false;

    // the mate id without its trailing "/1" (R1) or "/2" (R2)
    static std::string_view base_id(std::string_view id, char mate) {
        if (id.size() >= 2 && id[id.size() - 2] == '/' && id[id.size() - 1] == mate) id.remove_suffix(2);
        return id;
    }
    // Appends up to max_frags fragments (ids and qualities kept) to `out`; false: no fragment follows (end of the input, or
    // err: malformed input, streams of different lengths, mate ids that differ — the fragments before it are in `out`).
    bool next(Batch &out, uint64_t max_frags) {
        if (done) return false;
        b1.clear();
        b2.clear();
        bool more1 = q1.fill(b1, q2 ? max_frags : 2 * max_frags, ~0ull), more2 = more1;
        if (q2) more2 = q2->fill(b2, max_frags, ~0ull);
        const Batch &m1 = b1, &m2 = q2 ? b2 : b1;
        const uint64_t n1 = q2 ? b1.n() : b1.n() / 2, n2 = q2 ? b2.n() : b1.n() / 2;
        uint64_t n = std::min(n1, n2);
        if (!q1.pending_error.empty()) err = q1.pending_error;
        else if (q2 && !q2->pending_error.empty()) err = q2->pending_error;
        else if (q2 && n1 != n2)
            err = "paired input: " + std::string(n1 < n2 ? "--reads" : "--reads2") + " ends after " + std::to_string(n_pairs + n) +
                  " records, its mate stream has more";
        else if (!q2 && (b1.n() & 1))
            err = "paired input: --interleaved has an odd number of records (" + std::to_string(2 * (n_pairs + n) + 1) + ")";
        for (uint64_t i = 0; i < n; ++i) {  // Record::id() of the mates, "/1" and "/2" stripped, must be equal
            const std::string_view a = m1.id(q2 ? i : 2 * i), b = m2.id(q2 ? i : 2 * i + 1);
            if (base_id(a, '1') != base_id(b, '2')) {
                err = "paired input: the ids of mates " + std::to_string(n_pairs + i + 1) + " differ: '" + std::string(a) + "' and '" +
                      std::string(b) + "'";
                n = i;
                break;
            }
        }
        if (q2)
            for (uint64_t i = 0; i < n; ++i) {
                out.append(b1, i, i + 1, true);
                out.append(b2, i, i + 1, true);
            }
        else if (n)
            out.append(b1, 0, 2 * n, true);
        n_pairs += n;
        done = !err.empty() || (!more1 && !more2);
        return !done;
    }
};

// ---------------------------------------------------------------------------------------------------------------
// argument parsing (clap surface of main.rs:44-136)
// ---------------------------------------------------------------------------------------------------------------
struct Args {
    std::map<std::string, std::string> val;
    std::set<std::string> flags;
    int verbose = 0, quiet = 0;
};
struct Opt {
    const char *lng;
    char shrt;
    bool takes_value;
    bool repeatable = false;  // given again, the values are joined with ','
};
Args parse(int argc, char **argv, int start, const std::vector<Opt> &opts) {
    Args a;
    auto find_long = [&](const std::string &n) -> const Opt * {
        for (auto &o : opts)
            if (n == o.lng) return &o;
        return nullptr;
    };
    auto find_short = [&](char c) -> const Opt * {
        for (auto &o : opts)
            if (o.shrt && c == o.shrt) return &o;
        return nullptr;
    };
    for (int i = start; i < argc; ++i) {
        std::string s = argv[i];
        if (s.rfind("--", 0) == 0) {
            std::string name = s.substr(2), v;
            bool has_v = false;
            size_t eq = name.find('=');
            if (eq != std::string::npos) {
                v = name.substr(eq + 1);
                name = name.substr(0, eq);
                has_v = true;
            }
            if (name == "verbose") { ++a.verbose; continue; }
            if (name == "quiet") { ++a.quiet; continue; }
            const Opt *o = find_long(name);
            if (!o) die("error: unexpected argument '--" + name + "' found");
            if (!o->takes_value) { a.flags.insert(o->lng); continue; }
            if (!has_v) {
                if (i + 1 >= argc) die("error: a value is required for '--" + name + "'");
                v = argv[++i];
            }
            if (o->repeatable && a.val.count(o->lng)) a.val[o->lng] += "," + v;
            else a.val[o->lng] = v;
        } else if (s.size() >= 2 && s[0] == '-') {
            for (size_t j = 1; j < s.size(); ++j) {
                char c = s[j];
                if (c == 'v') { ++a.verbose; continue; }
                if (c == 'q') { ++a.quiet; continue; }
                const Opt *o = find_short(c);
                if (!o) die(std::string("error: unexpected argument '-") + c + "' found");
                if (!o->takes_value) { a.flags.insert(o->lng); continue; }
                std::string v = s.substr(j + 1);
                if (!v.empty() && v[0] == '=') v = v.substr(1);
                if (v.empty()) {
                    if (i + 1 >= argc) die(std::string("error: a value is required for '-") + c + "'");
                    v = argv[++i];
                }
                a.val[o->lng] = v;
                break;
            }
        } else die("error: unexpected argument '" + s + "' found");
    }
    return a;
}
std::string req(const Args &a, const char *name) {
    auto it = a.val.find(name);
    if (it == a.val.end()) die(std::string("error: the following required arguments were not provided: --") + name);
    return it->second;
}
std::string opt(const Args &a, const char *name, const std::string &def) {
    auto it = a.val.find(name);
    return it == a.val.end() ? def : it->second;
}
uint64_t to_u64(const std::string &s, const char *what) {
    char *e = nullptr;
    errno = 0;
    unsigned long long v = strtoull(s.c_str(), &e, 10);
    if (errno || !e || *e || s.empty() || s[0] == '-') die(std::string("error: invalid value '") + s + "' for '--" + what + "'");
    return v;
}
float to_f32(const std::string &s, const char *what) {
    char *e = nullptr;
    float v = strtof(s.c_str(), &e);
    if (!e || *e || s.empty()) die(std::string("error: invalid value '") + s + "' for '--" + what + "'");
    return v;
}
FmtOverride to_fmt(const std::string &s) {
    if (s == "auto") return FmtOverride::Auto;
    if (s == "fasta") return FmtOverride::Fasta;
    if (s == "fastq") return FmtOverride::Fastq;
    die("error: invalid value '" + s + "' for '--format' [possible values: auto, fasta, fastq]");
}

void rm_rf(const std::string &p) {
    struct stat st;
    if (lstat(p.c_str(), &st) != 0) return;
    if (S_ISDIR(st.st_mode)) {
        DIR *d = opendir(p.c_str());
        if (d) {
            while (dirent *e = readdir(d)) {
                std::string n = e->d_name;
                if (n != "." && n != "..") rm_rf(p + "/" + n);
            }
            closedir(d);
        }
        rmdir(p.c_str());
    } else unlink(p.c_str());
}

int device_from_env() {
    const char *e = getenv("PFQ_DEVICE");
    return e ? atoi(e) : 0;
}

// ---------------------------------------------------------------------------------------------------------------
// query (main.rs:249-376)
// ---------------------------------------------------------------------------------------------------------------
// An error on a worker thread ends the process at once, WITHOUT exit(): exit() would run the atexit handlers and static
// destructors (the HIP runtime's among them) while the other replicas' threads, the parser and the formatters are still
// inside HIP calls or writing.  Same message and status as die() (the reference panics: status 101).
[[noreturn]] void fail_from_thread(const char *what) {
    fprintf(stderr, "phage_filter: libpfq: %s\n", what);
    fflush(stderr);
    _exit(101);
}
void write_at(int fd, const char *buf, size_t len, uint64_t at) {
    for (size_t done = 0; done < len;) {
        ssize_t n = pwrite(fd, buf + done, len - done, (off_t)(at + done));
        if (n < 0) {
            fprintf(stderr, "phage_filter: write error: %s\n", strerror(errno));
            _exit(101);  // (called from writer threads: see fail_from_thread)
        }
        done += (size_t)n;
    }
}

// The database as a query serves it: one replica per listed device, or (--shard-depth) the subtree shards of its depth-E
// frontier, shard i on devices[i % N].  Shard i's leaves are [leaf_base[i], leaf_base[i + 1]) of the whole tree's
// leaf_names (after pruning); the shards' leaf ranges are disjoint and follow the whole tree's leaf order.
struct ServedDb {
    std::vector<int> devices;
    bool sharded;
    std::vector<pfq_tree *> trees;
    std::vector<std::string> leaf_names;
    std::vector<uint64_t> leaf_base{0};

    // BloomTree::load per replica (or shard), side by side.  At least one shard per device (no replication of shards),
    // checked before any device is touched.
    ServedDb(const std::string &path, const std::vector<int> &devs, bool shards, uint64_t shard_depth) : devices(devs), sharded(shards) {
        size_t n = devices.size();
        if (sharded) {
            uint64_t n_shards = 0;
            check(pfq_db_shard_count(path.c_str(), shard_depth, &n_shards));
            if (n_shards < devices.size())
                die("--shard-depth: the database has " + std::to_string(n_shards) + " subtree shards at depth " + std::to_string(shard_depth) +
                    ", fewer than the " + std::to_string(devices.size()) + " devices listed (every device needs a shard of its own)");
            n = (size_t)n_shards;
        }
        trees.assign(n, nullptr);
        std::vector<std::string> errs(n);
        fan_out(n, [&](size_t i) {
            const int rc = sharded ? pfq_tree_open_subtree(path.c_str(), devices[i % devices.size()], shard_depth, i, &trees[i])
                                   : pfq_tree_open(path.c_str(), devices[i], &trees[i]);
            if (rc != PFQ_OK) errs[i] = std::string("libpfq: ") + pfq_last_error();
        });
        for (auto &e : errs)
            if (!e.empty()) die(e);
    }
    void prune(uint64_t depth) {
        for (pfq_tree *t : trees) check(pfq_tree_prune(t, depth));
    }
    void load_leaf_names() {
        for (size_t i = 0; i < (sharded ? trees.size() : 1); ++i) {
            const char *const *tax = nullptr;
            uint64_t n_leaves = 0;
            check(pfq_leaf_counts(trees[i], &tax, nullptr, &n_leaves));
            leaf_names.insert(leaf_names.end(), tax, tax + n_leaves);
            leaf_base.push_back(leaf_base.back() + n_leaves);
        }
        if (sharded)
            for (size_t i = 0; i < trees.size(); ++i)
                fprintf(stderr, "shard %zu/%zu: leaves [%llu, %llu) of %llu on device %d\n", i, trees.size(), (unsigned long long)leaf_base[i],
                        (unsigned long long)leaf_base[i + 1], (unsigned long long)leaf_base.back(), devices[i % devices.size()]);
    }
    void save_counts(const std::string &csv) {
        if (!sharded) {
            // per-genome counts of all replicas: one RCCL all-reduce (every replica then holds the totals); replica 0 writes the file
            if (trees.size() > 1) check(pfq_trees_allreduce_counts(trees.data(), (uint32_t)trees.size()));
            check(pfq_save_leaf_counts(trees[0], csv.c_str()));
            return;
        }
        // the shards' counts one after the other, in pfq_save_leaf_counts' format: the leaf ranges are disjoint, so every
        // leaf (and every count stored in tree.bin) appears once — nothing to reduce
        FILE *f = fopen(csv.c_str(), "wb");
        if (!f) die("cannot create " + csv + ": " + strerror(errno));
        for (pfq_tree *t : trees) {
            const char *const *tax = nullptr;
            const uint64_t *cnt = nullptr;
            uint64_t n_leaves = 0;
            check(pfq_leaf_counts(t, &tax, &cnt, &n_leaves));
            for (uint64_t j = 0; j < n_leaves; ++j)
                if (cnt[j] > 0) fprintf(f, "%s,%llu\n", tax[j], (unsigned long long)cnt[j]);  // query.rs:177-182
        }
        if (fclose(f) != 0) die("short write to " + csv);
    }
    // --lca: the clade names (READ_LCA.tsv), from replica 0: the replicas hold one tree
    std::vector<std::string> clade_names;
    void load_clade_names() {
        const pfq_clade *cl = nullptr;
        uint64_t n = 0;
        check(pfq_tree_clades(trees[0], &cl, &n));
        for (uint64_t c = 0; c < n; ++c) clade_names.push_back(cl[c].name);
    }
    // --lca: CLADE_COUNTS.tsv.  Every replica counted its own reads: their `here` are summed on the host (a few KB) and
    // `below` is the sum over each clade's subtree (pre-order: children come after their parent).
    void save_clade_counts(const std::string &tsv) {
        const pfq_clade *cl = nullptr;
        uint64_t n = 0;
        check(pfq_tree_clades(trees[0], &cl, &n));
        std::vector<uint64_t> here(n, 0);
        for (pfq_tree *t : trees) {
            const uint64_t *h = nullptr;
            uint64_t nh = 0;
            check(pfq_clade_counts(t, &h, nullptr, &nh));
            if (nh != n) die("--lca: the replicas' clade tables differ");
            for (uint64_t c = 0; c < n; ++c) here[c] += h[c];
        }
        std::vector<uint64_t> below(here);
        for (uint64_t c = n; c-- > 1;) below[cl[c].parent] += below[c];
        FILE *f = fopen(tsv.c_str(), "wb");
        if (!f) die("cannot create " + tsv + ": " + strerror(errno));
        fputs("#clade\tparent\tdepth\tgenomes\tname\treads_here\treads_below\n", f);
        for (uint64_t c = 0; c < n; ++c) {
            if (!below[c]) continue;
            const std::string parent = cl[c].parent == PFQ_NO_CLADE ? "-" : std::to_string(cl[c].parent);
            fprintf(f, "%llu\t%s\t%u\t%u\t%s\t%llu\t%llu\n", (unsigned long long)c, parent.c_str(), cl[c].depth, cl[c].n_leaves, cl[c].name,
                    (unsigned long long)here[c], (unsigned long long)below[c]);
        }
        if (fclose(f) != 0) die("short write to " + tsv);
    }
    // --abundance: ABUNDANCE.tsv.  Every replica logged its own units' rows: they are moved into replica 0's log, which is
    // then estimated once (tol 65: below 0.001 unit).  estimated = mass / 2^16 rounded to three decimals.
    void save_abundance(const std::string &tsv, uint32_t max_iters) {
        for (size_t i = 1; i < trees.size(); ++i) check(pfq_abundance_absorb(trees[0], trees[i]));
        pfq_abundance ab{};
        check(pfq_abundance_estimate(trees[0], max_iters, 65, &ab));
        FILE *f = fopen(tsv.c_str(), "wb");
        if (!f) die("cannot create " + tsv + ": " + strerror(errno));
        fputs("#genome\tunique\testimated\tfraction\n", f);
        fprintf(f, "#units=%llu unhit=%llu unique=%llu ambiguous=%llu all_leaves=%llu iterations=%u converged=%u\n", (unsigned long long)ab.n_units,
                (unsigned long long)ab.n_unhit, (unsigned long long)ab.n_unique, (unsigned long long)ab.n_ambiguous,
                (unsigned long long)ab.n_all_leaves, ab.iterations, ab.converged);
        long double sum = 0;
        for (uint64_t l = 0; l < ab.n_leaves; ++l) sum += (long double)ab.mass[l];
        for (uint64_t l = 0; l < ab.n_leaves; ++l) {
            if (!ab.mass[l]) continue;
            const unsigned __int128 milli = ((unsigned __int128)ab.mass[l] * 1000 + 32768) >> 16;
            fprintf(f, "%s\t%llu\t%llu.%03llu\t%.6f\n", leaf_names[l].c_str(), (unsigned long long)ab.unique[l], (unsigned long long)(milli / 1000),
                    (unsigned long long)(milli % 1000), (double)((long double)ab.mass[l] / sum));
        }
        if (fclose(f) != 0) die("short write to " + tsv);
    }
    // --taxonomy: the file read for the current leaves (after --search-depth pruned them) and laid over every replica; the node
    // names (READ_TAXA.tsv) from replica 0.  The file's lines for other genomes and the leaves without a line go to stderr.
    std::vector<std::string> taxon_names;
    void set_taxonomy(const std::string &file) {
        std::vector<const char *> ids;
        for (const std::string &s : leaf_names) ids.push_back(s.c_str());
        pfq_taxonomy_file tf{};
        check(pfq_taxonomy_read(file.c_str(), ids.data(), ids.size(), &tf));
        fprintf(stderr, "taxonomy: %llu taxa from %llu lines; %llu lines for genomes that are not in the database; %llu of %llu genomes without a line sit under the root\n",
                (unsigned long long)tf.n_taxa, (unsigned long long)tf.lines_considered, (unsigned long long)tf.lines_other,
                (unsigned long long)tf.leaves_without_line, (unsigned long long)tf.n_leaves);
        for (pfq_tree *t : trees) check(pfq_tree_set_taxonomy(t, tf.n_taxa, tf.taxon_parent, tf.taxon_names, tf.leaf_taxon));
        const pfq_taxon *tx = nullptr;
        uint64_t n = 0;
        check(pfq_tree_taxa(trees[0], &tx, &n));
        for (uint64_t v = 0; v < n; ++v) taxon_names.push_back(tx[v].name);
    }
    // --taxonomy: TAXON_COUNTS.tsv.  Every replica counted its own reads: their `here` and `any` are summed on the host and `below`
    // is the sum of `here` over each node's subtree (pre-order: children come after their parent).  with_abundance: one more column,
    // the EM masses (replica 0's log, merged by save_abundance before) of the genomes below the node.
    void save_taxon_counts(const std::string &tsv, bool with_abundance, uint32_t max_iters) {
        const pfq_taxon *tx = nullptr;
        uint64_t n = 0;
        check(pfq_tree_taxa(trees[0], &tx, &n));
        std::vector<uint64_t> here(n, 0), any(n, 0);
        for (pfq_tree *t : trees) {
            const uint64_t *h = nullptr, *a = nullptr;
            uint64_t nh = 0;
            check(pfq_taxon_counts(t, &h, nullptr, &a, &nh));
            if (nh != n) die("--taxonomy: the replicas' node tables differ");
            for (uint64_t v = 0; v < n; ++v) {
                here[v] += h[v];
                any[v] += a[v];
            }
        }
        std::vector<uint64_t> below(here), mass(n, 0);
        for (uint64_t v = n; v-- > 1;) below[tx[v].parent] += below[v];
        if (with_abundance) {
            pfq_abundance ab{};
            check(pfq_abundance_estimate(trees[0], max_iters, 65, &ab));
            for (uint64_t v = 0; v < n; ++v)
                if (tx[v].leaf != PFQ_NO_CLADE) mass[v] = ab.mass[tx[v].leaf];
            for (uint64_t v = n; v-- > 1;) mass[tx[v].parent] += mass[v];
        }
        FILE *f = fopen(tsv.c_str(), "wb");
        if (!f) die("cannot create " + tsv + ": " + strerror(errno));
        fprintf(f, "#node\tparent\tdepth\tkind\tgenomes\tname\treads_here\treads_below\treads_any%s\n", with_abundance ? "\testimated" : "");
        for (uint64_t v = 0; v < n; ++v) {
            if (!any[v]) continue;
            const std::string parent = tx[v].parent == PFQ_NO_CLADE ? "-" : std::to_string(tx[v].parent);
            fprintf(f, "%llu\t%s\t%u\t%s\t%u\t%s\t%llu\t%llu\t%llu", (unsigned long long)v, parent.c_str(), tx[v].depth,
                    tx[v].leaf == PFQ_NO_CLADE ? "taxon" : "genome", tx[v].n_leaves, tx[v].name, (unsigned long long)here[v],
                    (unsigned long long)below[v], (unsigned long long)any[v]);
            if (with_abundance) {
                const unsigned __int128 milli = ((unsigned __int128)mass[v] * 1000 + 32768) >> 16;
                fprintf(f, "\t%llu.%03llu", (unsigned long long)(milli / 1000), (unsigned long long)(milli % 1000));
            }
            fputc('\n', f);
        }
        if (fclose(f) != 0) die("short write to " + tsv);
    }
    // --coverage: the precision of every replica's (shard's) sketch, before the first call makes it
    void set_coverage_precision(const std::string &p) {
        for (pfq_tree *t : trees) check(pfq_set_option(t, "PFQ_COVER_P", p.c_str()));
    }
    // --coverage: COVERAGE.tsv, one line per leaf in leaf order.  Every replica sketched its own units: the sketches are merged
    // into replica 0's (registers: maximum, counters: sums).  Shards hold disjoint leaf ranges in the whole tree's order and a
    // leaf's sketch depends only on the units that list it, so their lines follow one another like CLASSIFICATION.csv's.
    void save_coverage(const std::string &tsv) {
        if (!sharded)
            for (size_t i = 1; i < trees.size(); ++i) check(pfq_coverage_absorb(trees[0], trees[i]));
        FILE *f = fopen(tsv.c_str(), "wb");
        if (!f) die("cannot create " + tsv + ": " + strerror(errno));
        fputs("#genome\tunits\tmatched_kmers\tdistinct_kmers\tgenome_kmers\tbreadth\tduplication\n", f);
        for (size_t i = 0; i < (sharded ? trees.size() : 1); ++i) {
            pfq_coverage cv{};
            check(pfq_coverage_get(trees[i], &cv));
            for (uint64_t l = 0; l < cv.n_leaves; ++l) {
                const double distinct = cv.distinct[l], genome = cv.genome_kmers[l];
                fprintf(f, "%s\t%llu\t%llu\t%.1f\t%.1f\t%.4f\t%.2f\n", leaf_names[leaf_base[i] + l].c_str(), (unsigned long long)cv.units[l],
                        (unsigned long long)cv.matched[l], distinct, genome, genome > 0.0 ? distinct / genome : 0.0,
                        distinct > 0.0 ? (double)cv.matched[l] / distinct : 0.0);
            }
        }
        if (fclose(f) != 0) die("short write to " + tsv);
    }
    // --sweep: the list for every replica, before the first call; the library refuses a database that is not superset-verified
    void set_sweep(const std::vector<float> &thr) {
        for (pfq_tree *t : trees) check(pfq_tree_set_sweep(t, thr.data(), (uint32_t)thr.size()));
    }
    // --sweep: THRESHOLDS.tsv, one line per threshold, and THRESHOLD_GENOMES.tsv, one line per (genome, threshold) with reads, the
    // genomes in leaf order like CLASSIFICATION.csv.  Every replica counted its own reads: the counters are summed into replica
    // 0's.  typed: the thresholds as the user wrote them.
    void save_sweep(const std::string &dir, const std::vector<std::string> &typed) {
        for (size_t i = 1; i < trees.size(); ++i) check(pfq_sweep_absorb(trees[0], trees[i]));
        pfq_sweep sw{};
        check(pfq_sweep_get(trees[0], &sw));
        if (sw.n_thresholds != typed.size()) die("--sweep: the library holds another threshold list");
        const std::string tsv = dir + "/THRESHOLDS.tsv", per_genome = dir + "/THRESHOLD_GENOMES.tsv";
        FILE *f = fopen(tsv.c_str(), "wb");
        if (!f) die("cannot create " + tsv + ": " + strerror(errno));
        fputs("#threshold\treads\treads_hit\treads_unique\tassignments\tgenomes_hit\n", f);
        for (uint32_t t = 0; t < sw.n_thresholds; ++t)
            fprintf(f, "%s\t%llu\t%llu\t%llu\t%llu\t%llu\n", typed[t].c_str(), (unsigned long long)sw.n_units, (unsigned long long)sw.units_hit[t],
                    (unsigned long long)sw.units_unique[t], (unsigned long long)sw.entries[t], (unsigned long long)sw.genomes_hit[t]);
        if (fclose(f) != 0) die("short write to " + tsv);
        f = fopen(per_genome.c_str(), "wb");
        if (!f) die("cannot create " + per_genome + ": " + strerror(errno));
        fputs("#genome\tthreshold\treads\tunique_reads\n", f);
        for (uint64_t l = 0; l < sw.n_leaves; ++l)
            for (uint32_t t = 0; t < sw.n_thresholds; ++t) {
                const uint64_t reads = sw.leaf_units[t * sw.n_leaves + l];
                if (reads)
                    fprintf(f, "%s\t%s\t%llu\t%llu\n", leaf_names[l].c_str(), typed[t].c_str(), (unsigned long long)reads,
                            (unsigned long long)sw.leaf_unique[t * sw.n_leaves + l]);
            }
        if (fclose(f) != 0) die("short write to " + per_genome);
    }
    void close() {
        for (pfq_tree *t : trees) pfq_tree_close(t);
    }
};

// Everything the command line of `query` says, as parse_query_options() leaves it: plain data, read by everything below.
struct QueryOptions {
    std::string reads, reads2, out, db_path;
    unsigned threads = 4;                     // rayon pool size in the reference; here: parser workers
    uint64_t block = 100;                     // --block-size-reads
    float threshold = 1.0f;
    FmtOverride format = FmtOverride::Auto;
    bool pos = false, neg = false;  // --pos-filter, --neg-filter
    bool scores = false;            // --scores: READ_SCORES.tsv, one line per (read record, hit genome) with how many of the read's k-mers the genome contains
    int lca = 0;                    // --lca: 0 none, 1 all, 2 best: CLADE_COUNTS.tsv
    bool lca_reads = false;         // --lca-reads: READ_LCA.tsv, one line per record with hits
    bool abundance = false;         // --abundance [--abundance-iters N]: ABUNDANCE.tsv, an EM over the logged hit rows
    bool coverage = false;          // --coverage [--coverage-precision P]: COVERAGE.tsv, the distinct k-mers every genome's reads matched
    bool taxonomy = false;          // --taxonomy FILE: TAXON_COUNTS.tsv
    uint64_t abundance_iters = 200;
    std::string coverage_precision = "12", taxonomy_file;
    bool taxon_reads = false;  // --taxon-reads: READ_TAXA.tsv, one line per record with hits
    bool best_hits = false;    // --best-hits: --taxonomy, --abundance and --coverage take every unit's best-scoring genomes
    bool sweep = false;        // --sweep T1,T2,..: THRESHOLDS.tsv and THRESHOLD_GENOMES.tsv; the values as numbers and as typed
    std::vector<float> sweep_thr;
    std::vector<std::string> sweep_typed;
    uint32_t frame = 0, frame_step = 0;  // --frame F [--frame-step S] (frame 0: whole sequences): SEGMENTS.tsv
    bool device_parse = false, device_inflate = false, device_output = false;
    bool gzip_output = false;  // --gzip-output [--gzip-level L]: the POS / NEG files are blocked gzip (BGZF)
    int gzip_level = 6;        // zlib's, for the members the host makes
    bool has_reads2 = false, interleaved = false, pair_both = false;  // --reads2, --interleaved, --pair-mode both
    std::vector<int> devices;                     // --devices or PFQ_DEVICES, else the one of PFQ_DEVICE
    bool sharded = false, pruned = false;         // --shard-depth D, already lowered to the search depth; --search-depth, as typed: it is
    uint64_t shard_depth = 0;                     // read after the database is open
    std::string search_depth;
    // read preprocessing: any trimming, adapter or mate option or --deplete turns it on
    bool prep = false;
    pfq_prep_params params{0, 4, 0, 0, 0xffffffffu, 0, 0};  // (min_length 0: not given, the database's k)
    std::vector<std::string> adapters[2];                   // --adapter / --adapter2: upper case, presets replaced
    uint32_t adapter_overlap = 5, adapter_errors = 10;
    uint32_t mate_overlap = 0, mate_overlap_errors = 10;    // (0: off)
    uint32_t mate_correct_high = 0, mate_correct_low = 0;  // (high 0: off)
    std::vector<std::string> deplete_dirs;                  // --deplete DIR [..], in the order given
    float deplete_threshold = 1.0f;                         // --deplete-threshold T (default: -f), and as typed
    std::string deplete_threshold_typed;
    bool adapters_on() const { return !adapters[0].empty(); }
    bool paired() const { return interleaved || has_reads2; }
    bool per_read() const {  // the per-read hit lists are needed
        return pos || neg || scores || lca == 2 || lca_reads || abundance || coverage || taxonomy || sweep;
    }
};

// One member of blocked gzip (BGZF) made with zlib: text[0, n), n <= BGZF_TEXT, into member (BGZF_ROOM bytes); returns its size.
// The empty text at a level above 0 is the 28-byte end marker every reader knows, byte for byte.
constexpr size_t BGZF_TEXT = 65280, BGZF_ROOM = 65536 + 1024;
size_t bgzf_member(const unsigned char *text, size_t n, int level, unsigned char *member) {
    z_stream z{};
    if (deflateInit2(&z, n ? level : 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) die("zlib: deflateInit2 failed");
    z.next_in = const_cast<unsigned char *>(text);
    z.avail_in = (uInt)n;
    z.next_out = member + 18;
    z.avail_out = (uInt)(BGZF_ROOM - 18 - 8);
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) die("zlib: deflate did not finish a member");
    const size_t pay = z.total_out, size = 18 + pay + 8;
    deflateEnd(&z);
    if (size > 65536) die("bgzf: a member of more than 64 KiB");  // (cannot happen: 65 280 bytes stored are 65 290)
    const unsigned char head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (unsigned char)((size - 1) & 0xff), (unsigned char)((size - 1) >> 8)};
    memcpy(member, head, 18);
    const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), text, (uInt)n), isize = (uint32_t)n;
    for (int i = 0; i < 4; ++i) {
        member[18 + pay + i] = (unsigned char)(crc >> (8 * i));
        member[18 + pay + 4 + i] = (unsigned char)(isize >> (8 * i));
    }
    return size;
}
// text[0, n) as members of at most BGZF_TEXT text bytes, appended to gz
void bgzf_pack(const char *text, size_t n, int level, std::vector<unsigned char> &gz) {
    for (size_t at = 0; at < n; at += BGZF_TEXT) {
        const size_t have = gz.size();
        gz.resize(have + BGZF_ROOM);
        gz.resize(have + bgzf_member((const unsigned char *)text + at, std::min(BGZF_TEXT, n - at), level, gz.data() + have));
    }
}

// A POS/NEG file and the bytes written to it so far (the formatters' parts are written at computed offsets).  --gzip-output
// (gz_level >= 0): what append() is given is text and is written as members zlib makes of it; append_raw() takes members.
struct OutFile {
    int fd = -1;
    uint64_t size = 0;
    int gz_level = -1;
    std::vector<unsigned char> gz;
    void append_raw(const char *p, size_t len) {
        if (fd < 0 || !len) return;
        write_at(fd, p, len, size);
        size += len;
    }
    void append(const char *p, size_t len) {
        if (fd < 0 || !len) return;
        if (gz_level < 0) return append_raw(p, len);
        gz.clear();
        bgzf_pack(p, len, gz_level, gz);
        append_raw((const char *)gz.data(), gz.size());
    }
};
struct Outputs {
    OutFile pos, neg, pos2, neg2;  // --reads2: the mates of R2 go to POS_FILTERING_2 / NEG_FILTERING_2, those of R1 to _1
    FILE *scores = nullptr;        // --scores: READ_SCORES.tsv
    FILE *lca = nullptr;           // --lca-reads: READ_LCA.tsv
    FILE *taxa = nullptr;          // --taxon-reads: READ_TAXA.tsv
    Outputs(const QueryOptions &o, const char *ext) {
        const std::string &dir = o.out;
        const bool has_reads2 = o.has_reads2;
        auto create = [&](OutFile &f, const std::string &name, const char *suffix) {
            if ((f.fd = open((dir + "/" + name + suffix + ext + (o.gzip_output ? ".gz" : "")).c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666)) < 0)
                die("cannot create " + name + " in " + dir);
            if (o.gzip_output) f.gz_level = o.gzip_level;
        };
        const char *mate1 = has_reads2 ? "_1." : ".";
        if (o.pos) create(pos, "POS_FILTERING", mate1);
        if (o.neg) create(neg, "NEG_FILTERING", mate1);
        if (has_reads2 && o.pos) create(pos2, "POS_FILTERING_2", ".");
        if (has_reads2 && o.neg) create(neg2, "NEG_FILTERING_2", ".");
        if (o.scores) {
            if (!(scores = fopen((dir + "/READ_SCORES.tsv").c_str(), "wb"))) die("cannot create READ_SCORES.tsv in " + dir);
            fputs("#read_id\tkmers\tgenome\tmatched_kmers\n", scores);
        }
        if (o.lca_reads) {
            if (!(lca = fopen((dir + "/READ_LCA.tsv").c_str(), "wb"))) die("cannot create READ_LCA.tsv in " + dir);
            fputs("#read_id\thits\tclade\tname\n", lca);
        }
        if (o.taxon_reads) {
            if (!(taxa = fopen((dir + "/READ_TAXA.tsv").c_str(), "wb"))) die("cannot create READ_TAXA.tsv in " + dir);
            fputs("#read_id\thits\tnode\tname\n", taxa);
        }
    }
    void close() {
        for (OutFile *f : {&pos, &neg, &pos2, &neg2}) {
            if (f->fd >= 0 && f->gz_level >= 0) {  // the end marker, also of a file without a record
                unsigned char marker[BGZF_ROOM];
                f->append_raw((const char *)marker, bgzf_member(marker, 0, 6, marker));
            }
            if (f->fd >= 0) ::close(f->fd);
        }
        if (scores && fclose(scores) != 0) die("short write to READ_SCORES.tsv");
        if (lca && fclose(lca) != 0) die("short write to READ_LCA.tsv");
        if (taxa && fclose(taxa) != 0) die("short write to READ_TAXA.tsv");
    }
};

// Hit lists: unit u (a read, or with PFQ_PAIRED a fragment) hits leaves[off[u], off[u + 1]), ascending; --scores: the
// matched k-mers, aligned with leaves
struct Hits {
    std::vector<uint64_t> off;
    std::vector<uint32_t> leaves, scores;
    std::vector<uint32_t> lca;       // --lca-reads: the unit's clade (PFQ_NO_CLADE: no hit)
    std::vector<uint32_t> taxa;      // --taxon-reads: the unit's node of the taxonomy (PFQ_NO_CLADE: no hit)
    std::vector<uint64_t> call_off;  // the call's read offsets, when its range does not start at the batch's first read
};
// Read preprocessing: the totals of all calls and replicas (PREPROCESS.tsv, INSERT_SIZES.tsv) and every replica's own copies of
// the screens of --deplete on its device (screens_of: by the replica's tree; filled before the loop starts, only read afterwards)
struct PrepRun {
    static constexpr size_t DEPLETE_MAX = 4;
    std::atomic<uint64_t> reads{0}, kept{0}, trimmed{0}, bases{0}, bases_kept{0};
    std::atomic<uint64_t> reason[5] = {};
    std::atomic<uint64_t> adapter_reads{0}, adapter_bases{0};
    std::atomic<uint64_t> adapter_found[2 * PFQ_ADAPTER_MAX] = {};
    std::atomic<uint64_t> overlap_fragments{0}, overlap_skipped{0}, overlap_found{0}, overlap_readthrough{0}, overlap_reads{0}, overlap_bases{0};
    std::atomic<uint64_t> insert_hist[PFQ_OVERLAP_INSERT_MAX + 1] = {};
    std::atomic<uint64_t> corrected_fragments{0}, corrected_bases{0}, correct_unresolved{0}, correct_no_quality{0};
    std::atomic<uint64_t> depleted_units[DEPLETE_MAX] = {}, depleted_reads[DEPLETE_MAX] = {}, depleted_bases[DEPLETE_MAX] = {};
    std::map<pfq_tree *, std::vector<pfq_tree *>> screens_of;
};
// What a call kept of its reads [r0, r1): begin and len of every read, the kept reads' indices (relative to r0), ascending; with
// --mate-correct the call's patch list (read relative to r0), ascending by (read, pos)
struct PrepKept {
    std::vector<uint32_t> begin, len, kept;
    std::vector<pfq_prep_patch> patches;
};
// Reads [r0, r1) of the padded batch b through `tree` in one pfq_query_batch at o.threshold.  With PFQ_WANT_HITS the hit lists (and
// scores; --lca-reads, --taxon-reads: the units' LCAs and nodes) are copied out of the library's buffers, which the next call on
// the tree reuses, into h.  With preprocessing on the reads go through pfq_prep_reads first — the qualities in a buffer aligned to
// the bases; a read whose quality length differs from its sequence length, and every FASTA read, has none — and pfq_prep_query
// classifies what it kept: the units are then the kept reads (fragments), which pk (if asked for) names.  The parameters of
// preprocessing are the options', what it did is added to `prep`.
void classify(pfq_tree *tree, const Batch &b, uint64_t r0, uint64_t r1, const QueryOptions &o, uint32_t flags, Hits &h, PrepRun &prep, PrepKept *pk = nullptr) {
    const bool want = (flags & PFQ_WANT_HITS) != 0;
    uint64_t units = flags & PFQ_PAIRED ? (r1 - r0) / 2 : r1 - r0;
    if (pk) {
        pk->begin.clear();
        pk->len.clear();
        pk->kept.clear();
        pk->patches.clear();
    }
    if (want) {
        h.off.assign(units + 1, 0);
        h.leaves.clear();
        h.scores.clear();
        h.lca.clear();
        h.taxa.clear();
    }
    if (r1 == r0) return;
    const uint64_t *off = b.off.data();
    if (r0) {
        h.call_off.resize(r1 - r0 + 1);
        for (uint64_t r = r0; r <= r1; ++r) h.call_off[r - r0] = b.off[r] - b.off[r0];
        off = h.call_off.data();
    }
    pfq_hits hits{};
    if (o.prep) {
        static thread_local std::vector<uint8_t> qual, has;
        const uint64_t base = b.off[r0];
        qual.assign(b.off[r1] - base, 0);
        has.assign(r1 - r0, 0);
        bool any_qual = false;
        if ((o.params.trim_quality || o.mate_correct_high) && !b.has_qual.empty())  // (the two steps that look at qualities)
            for (uint64_t r = r0; r < r1; ++r) {
                if (!b.has_qual[r]) continue;
                const std::string_view q = b.quality(r);
                if (q.size() != b.off[r + 1] - b.off[r]) continue;
                if (!q.empty()) memcpy(qual.data() + (b.off[r] - base), q.data(), q.size());
                has[r - r0] = 1;
                any_qual = true;
            }
        pfq_prep_params par = o.params;
        par.flags = (flags & PFQ_PAIRED ? PFQ_PREP_PAIRED : 0u) | (pk ? PFQ_PREP_WANT_READS : 0u);
        pfq_prep res{};
        if (pfq_prep_reads(tree, b.seq.data() + base, any_qual ? qual.data() : nullptr, off, any_qual ? has.data() : nullptr, r1 - r0, &par, &res) != PFQ_OK)
            fail_from_thread(pfq_last_error());
        prep.reads += res.n_reads;
        prep.kept += res.n_kept;
        prep.trimmed += res.n_trimmed;
        prep.bases += res.bases_in;
        prep.bases_kept += res.bases_kept;
        for (int c = 0; c < 5; ++c) prep.reason[c] += res.n_reason[c];
        if (o.adapters_on()) {
            pfq_prep_adapters ad{};
            if (pfq_prep_last_adapters(tree, &ad) != PFQ_OK) fail_from_thread(pfq_last_error());
            prep.adapter_reads += ad.n_found;
            prep.adapter_bases += ad.bases_cut;
            for (int c = 0; c < 2 * PFQ_ADAPTER_MAX; ++c) prep.adapter_found[c] += ad.found[c];
        }
        if (o.mate_overlap && (par.flags & PFQ_PREP_PAIRED)) {
            pfq_prep_overlap ov{};
            if (pfq_prep_last_overlap(tree, &ov) != PFQ_OK) fail_from_thread(pfq_last_error());
            prep.overlap_fragments += ov.n_analysed;
            prep.overlap_skipped += ov.n_skipped;
            prep.overlap_found += ov.n_overlapped;
            prep.overlap_readthrough += ov.n_readthrough;
            prep.overlap_reads += ov.reads_cut;
            prep.overlap_bases += ov.bases_cut;
            for (int i = 0; i <= PFQ_OVERLAP_INSERT_MAX; ++i)
                if (ov.hist[i]) prep.insert_hist[i] += ov.hist[i];
            if (o.mate_correct_high) {
                pfq_prep_corrections co{};
                if (pfq_prep_last_corrections(tree, &co) != PFQ_OK) fail_from_thread(pfq_last_error());
                prep.corrected_fragments += co.n_fragments_corrected;
                prep.corrected_bases += co.n_bases[0] + co.n_bases[1];
                prep.correct_unresolved += co.n_unresolved;
                prep.correct_no_quality += co.n_no_quality;
                if (pk) pk->patches.assign(co.patches, co.patches + co.n_patches);
            }
        }
        // --deplete: the screens take their units out of the prepared block, one after the other; a fragment leaves when either
        // mate hits.  What is mapped back is what the last screen left.
        uint64_t n_kept = res.n_kept;
        const uint32_t *kept = res.kept;
        if (!o.deplete_dirs.empty()) {
            const std::vector<pfq_tree *> &screens = prep.screens_of.at(tree);
            for (size_t i = 0; i < screens.size(); ++i) {
                pfq_prep_depleted d{};
                if (pfq_prep_deplete(tree, screens[i], o.deplete_threshold, flags & PFQ_PAIRED ? PFQ_PAIRED : 0u, &d) != PFQ_OK) fail_from_thread(pfq_last_error());
                prep.depleted_units[i] += d.units_removed;
                prep.depleted_reads[i] += d.reads_removed;
                prep.depleted_bases[i] += d.bases_removed;
                n_kept = d.n_kept;
                if (pk) kept = d.kept;
            }
        }
        if (pk) {
            pk->begin.assign(res.begin, res.begin + res.n_reads);
            pk->len.assign(res.len, res.len + res.n_reads);
            pk->kept.assign(kept, kept + n_kept);
        }
        units = flags & PFQ_PAIRED ? n_kept / 2 : n_kept;
        if (want) h.off.assign(units + 1, 0);
        if (!n_kept) return;
        if (pfq_prep_query(tree, o.threshold, flags, want ? &hits : nullptr) != PFQ_OK) fail_from_thread(pfq_last_error());
    } else if (pfq_query_batch(tree, b.seq.data() + b.off[r0], off, r1 - r0, o.threshold, flags, want ? &hits : nullptr) != PFQ_OK) {
        fail_from_thread(pfq_last_error());
    }
    if (!want) return;
    memcpy(h.off.data(), hits.offsets, (units + 1) * sizeof(uint64_t));
    h.leaves.assign(hits.leaves, hits.leaves + hits.offsets[units]);
    if (flags & PFQ_WANT_SCORES) {
        const uint32_t *sc = nullptr;
        uint64_t n_sc = 0;
        if (pfq_last_hit_scores(tree, &sc, &n_sc) != PFQ_OK) fail_from_thread(pfq_last_error());
        h.scores.assign(sc, sc + n_sc);
    }
    if (o.lca_reads) {
        const uint32_t *lca = nullptr;
        uint64_t n_lca = 0;
        if (pfq_last_lca(tree, &lca, &n_lca) != PFQ_OK) fail_from_thread(pfq_last_error());
        h.lca.assign(lca, lca + n_lca);
    }
    if (o.taxon_reads) {
        const uint32_t *node = nullptr;
        uint64_t n_node = 0;
        if (pfq_last_taxa(tree, &node, &n_node) != PFQ_OK) fail_from_thread(pfq_last_error());
        h.taxa.assign(node, node + n_node);
    }
}
// The trees' hit lists of n units in the whole tree's leaf order.  Part i covers units [n i / P, n (i + 1) / P) for a
// replica (the shares follow one another) and all of them for a shard (per unit, the shards' lists in shard order, each
// offset by the shard's first leaf).  A single part is swapped into `out`.  cuts (replicas, preprocessing): part i covers units
// [cuts[i], cuts[i + 1]) instead — what share i kept.
void merge_hits(std::vector<Hits> &parts, uint64_t n, const ServedDb &db, Hits &out, const std::vector<uint64_t> *cuts = nullptr) {
    const size_t P = parts.size();
    if (P == 1) {
        std::swap(out, parts[0]);
        return;
    }
    uint64_t total = 0;
    bool with_scores = false, with_lca = false, with_taxa = false;
    for (const Hits &h : parts) {
        total += h.leaves.size();
        with_scores |= !h.scores.empty();
        with_lca |= !h.lca.empty();
        with_taxa |= !h.taxa.empty();
    }
    out.lca.assign(with_lca ? n : 0, PFQ_NO_CLADE);  // (replicas only: --lca does not serve shards)
    out.taxa.assign(with_taxa ? n : 0, PFQ_NO_CLADE);  // (replicas only, likewise)
    out.off.assign(n + 1, 0);
    out.leaves.resize(total);
    out.scores.resize(with_scores ? total : 0);
    uint64_t at = 0;
    for (uint64_t u = 0; u < n; ++u) {
        for (size_t i = 0; i < P; ++i) {
            const uint64_t u0 = db.sharded ? 0 : cuts ? (*cuts)[i] : n * i / P, u1 = db.sharded ? n : cuts ? (*cuts)[i + 1] : n * (i + 1) / P;
            if (u < u0 || u >= u1) continue;
            const Hits &h = parts[i];
            const uint64_t j0 = h.off[u - u0], j1 = h.off[u - u0 + 1];
            const uint32_t base = db.sharded ? (uint32_t)db.leaf_base[i] : 0u;
            if (with_scores) std::copy(h.scores.begin() + j0, h.scores.begin() + j1, out.scores.begin() + at);
            if (with_lca) out.lca[u] = h.lca[u - u0];
            if (with_taxa) out.taxa[u] = h.taxa[u - u0];
            for (uint64_t j = j0; j < j1; ++j) out.leaves[at++] = h.leaves[j] + base;
        }
        out.off[u + 1] = at;
    }
}

// Preprocessing with per-read outputs: the batch becomes what the parsers would have made of an input that holds only the kept
// reads, each cut to [begin, begin + len) in bases and qualities, ids unchanged — everything behind the classification then
// works as it does without the options.  Share i of the batch is reads [share[i], share[i + 1]) and pks[i] what its call kept;
// returns the kept reads before every share (and their total).  A quality whose length differs from its sequence's stays whole.
std::vector<uint64_t> keep_prepared(Batch &b, const std::vector<uint64_t> &share, const std::vector<PrepKept> &pks) {
    Batch nb;
    std::vector<uint64_t> cuts(pks.size() + 1, 0);
    for (size_t i = 0; i < pks.size(); ++i) {
        const PrepKept &pk = pks[i];
        size_t pi = 0;  // (--mate-correct: the patches and the kept reads both ascend)
        for (uint32_t j : pk.kept) {
            const uint64_t r = share[i] + j, s0 = b.off[r] + pk.begin[j], len = pk.len[j];
            const uint64_t at = nb.seq.size(), qat = nb.qual.size();
            nb.seq.insert(nb.seq.end(), b.seq.begin() + s0, b.seq.begin() + s0 + len);
            nb.off.push_back(nb.seq.size());
            const std::string_view id = b.id(r), q = b.quality(r);
            nb.id_bytes.insert(nb.id_bytes.end(), id.begin(), id.end());
            nb.id_off.push_back(nb.id_bytes.size());
            if (q.size() == b.off[r + 1] - b.off[r]) nb.qual.insert(nb.qual.end(), q.begin() + pk.begin[j], q.begin() + pk.begin[j] + len);
            else nb.qual.insert(nb.qual.end(), q.begin(), q.end());
            // the corrections that lie in what is kept of the read (a corrected read has qualities as long as its bases)
            while (pi < pk.patches.size() && pk.patches[pi].read < j) ++pi;
            for (; pi < pk.patches.size() && pk.patches[pi].read == j; ++pi) {
                const pfq_prep_patch &pt = pk.patches[pi];
                if (pt.pos < pk.begin[j] || pt.pos >= pk.begin[j] + len) continue;
                nb.seq[at + (pt.pos - pk.begin[j])] = pt.base;
                nb.qual[qat + (pt.pos - pk.begin[j])] = (char)pt.qual;
            }
            nb.qual_off.push_back(nb.qual.size());
            nb.has_qual.push_back(b.has_qual[r]);
        }
        cuts[i + 1] = nb.n();
    }
    nb.held = std::move(b.held);  // (the parsed segments go back to the parsers when the batch is released, as before)
    b = std::move(nb);
    return cuts;
}

// Output buffers of the formatters: grown with realloc (no zero fill), kept from batch to batch.
struct OutBuf {
    char *p = nullptr;
    size_t n = 0, cap = 0;
    ~OutBuf() { free(p); }
    char *room(size_t want) {
        if (n + want > cap) {
            cap = std::max(n + want, cap + cap / 2 + (1u << 20));
            p = (char *)realloc(p, cap);
            if (!p) die("out of memory (output buffer)");
        }
        return p + n;
    }
    void put(const char *src, size_t len) {
        memcpy(room(len), src, len);
        n += len;
    }
    void put(char c) {
        *room(1) = c;
        ++n;
    }
};
// write_record (main.rs:394-404) of read r: '@' / '>' + id; for a mapped read get_ext_id's " |g1,g2" with the genomes
// [l0, l1) (set order unspecified in the reference; leaf order here); the sequence, upper-cased (main.rs:347-349); FASTQ:
// '+' and the quality.  No allocation per record.
void put_record(OutBuf &o, const Batch &b, uint64_t r, const uint32_t *l0, const uint32_t *l1, const std::vector<std::string> &names) {
    const std::string_view id = b.id(r);
    const uint64_t len = b.off[r + 1] - b.off[r];
    const bool fq = b.has_qual[r] != 0;
    {
        char *dst = o.room(id.size() + 3);
        dst[0] = fq ? '@' : '>';
        memcpy(dst + 1, id.data(), id.size());
        o.n += id.size() + 1;
    }
    if (l0 != l1) {
        o.put(" |", 2);
        for (const uint32_t *l = l0; l < l1; ++l) {
            if (l != l0) o.put(',');
            o.put(names[*l].data(), names[*l].size());
        }
    }
    const std::string_view q = fq ? b.quality(r) : std::string_view();
    char *dst = o.room(len + q.size() + 5);
    *dst++ = '\n';
    copy_upper(dst, b.seq.data() + b.off[r], len);
    dst += len;
    *dst++ = '\n';
    size_t wrote = len + 2;
    if (fq) {
        dst[0] = '+';
        dst[1] = '\n';
        memcpy(dst + 2, q.data(), q.size());
        dst[2 + q.size()] = '\n';
        wrote += q.size() + 3;
    }
    o.n += wrote;
}
uint64_t n_kmers(uint64_t len, uint64_t k) { return len >= k ? len - k + 1 : 0; }
// READ_SCORES.tsv lines of a record (or fragment) with hits, "id\tkmers\tgenome\tmatched": its n genomes by matched
// k-mers, descending (ties in leaf order)
void put_scores(std::string &o, std::string_view id, uint64_t kmers, const uint32_t *leaves, const uint32_t *sc, uint64_t n,
                const std::vector<std::string> &names, std::vector<uint64_t> &order) {
    order.resize(n);
    for (uint64_t j = 0; j < n; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return sc[x] > sc[y]; });
    char ks[32], num[32];
    const int nk = snprintf(ks, sizeof ks, "\t%llu\t", (unsigned long long)kmers);
    for (uint64_t j : order) {
        o.append(id.data(), id.size());
        o.append(ks, (size_t)nk);
        o.append(names[leaves[j]]);
        o.append(num, (size_t)snprintf(num, sizeof num, "\t%u\n", sc[j]));
    }
}

// READ_LCA.tsv (READ_TAXA.tsv) line of a record (or fragment) with hits: "id\thits\tclade\tname" (the node of the taxonomy and its name)
void put_lca(std::string &o, std::string_view id, uint64_t n_hits, uint32_t clade, const std::vector<std::string> &clade_names) {
    char num[64];
    o.append(id.data(), id.size());
    o.append(num, (size_t)snprintf(num, sizeof num, "\t%llu\t%u\t", (unsigned long long)n_hits, clade));
    o.append(clade_names[clade]);
    o.push_back('\n');
}

// ResultMap of one block (result_map.rs:20-45) without allocations: an open-addressing table over the ids of the reads that
// hit.  An id that hits twice in a block (the same read id in two records) merges its genomes.
struct BlockGroup {
    std::string_view id;
    uint64_t first_read;  // the (first) read with this id that hit
    int32_t merged;       // index into the block's merged sets once a second read with the id has hit
};
inline uint64_t hash_id(std::string_view v) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ v.size();
    size_t i = 0;
    for (; i + 8 <= v.size(); i += 8) {
        uint64_t x;
        memcpy(&x, v.data() + i, 8);
        h = (h ^ x) * 0xff51afd7ed558ccdull;
        h ^= h >> 32;
    }
    uint64_t x = 0;
    if (i < v.size()) memcpy(&x, v.data() + i, v.size() - i);
    h = (h ^ x) * 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 29);
}
// slots of the table of a block in which n_hit reads hit (a power of two; 0: the block has no hit and needs no table)
inline uint64_t block_table_slots(uint64_t n_hit) {
    if (!n_hit) return 0;
    uint64_t want = 16;
    while (want < 2 * n_hit) want <<= 1;
    return want;
}
// The map of block [b0, b1) of batch b with the hit rows (h_off, h_leaves): grp [reads of the block that hit], tab [tab_slots,
// zeroed], the genome sets of the ids that hit more than once in `merged`; then for EVERY read of the block its group in
// grp_of[r] (read_mapped: the id is in the block's map, also for reads that did not hit themselves), -1: not mapped.
void map_block(const Batch &b, uint64_t b0, uint64_t b1, const uint64_t *h_off, const uint32_t *h_leaves, BlockGroup *grp, uint32_t *tab,
               size_t tab_slots, std::vector<std::vector<uint32_t>> &merged, int32_t *grp_of) {
    const size_t mask = tab_slots - 1;  // (no table: the block has no hit)
    const bool any = tab_slots != 0;
    merged.clear();
    uint32_t n_grp = 0;
    auto find = [&](std::string_view id, bool insert, uint64_t r) -> int32_t {
        for (size_t i = (size_t)hash_id(id) & mask;; i = (i + 1) & mask) {
            const uint32_t g = tab[i];
            if (!g) {
                if (!insert) return -1;
                grp[n_grp] = BlockGroup{id, r, -1};
                tab[i] = ++n_grp;
                return (int32_t)n_grp - 1;
            }
            if (grp[g - 1].id == id) return (int32_t)g - 1;
        }
    };
    if (any)
        for (uint64_t r = b0; r < b1; ++r) {
            if (h_off[r] == h_off[r + 1]) continue;
            const int32_t g = find(b.id(r), true, r);
            grp_of[r] = g;
            BlockGroup &gr = grp[g];
            if (gr.first_read == r) continue;        // new id
            if (gr.merged < 0) {                      // second read with this id: the sets merge
                gr.merged = (int32_t)merged.size();
                merged.emplace_back(h_leaves + h_off[gr.first_read], h_leaves + h_off[gr.first_read + 1]);
            }
            merged[gr.merged].insert(merged[gr.merged].end(), h_leaves + h_off[r], h_leaves + h_off[r + 1]);
        }
    for (auto &v : merged) {  // a set of genomes per id; printed in leaf order
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
    }
    for (uint64_t r = b0; r < b1; ++r)
        if (h_off[r] == h_off[r + 1]) grp_of[r] = any ? find(b.id(r), false, 0) : -1;
}
// Read r of a mapped block (group g of grp, -1: not mapped) into the POS or the NEG buffer, if that stream is wanted.
inline void put_block_record(OutBuf &pb, OutBuf &nb, const Batch &b, uint64_t r, int32_t g, const BlockGroup *grp,
                             const std::vector<std::vector<uint32_t>> &merged, const uint64_t *h_off, const uint32_t *h_leaves, bool pos, bool neg,
                             const std::vector<std::string> &names) {
    const bool mapped = g >= 0;
    if (mapped ? !pos : !neg) return;
    const uint32_t *l0 = nullptr, *l1 = nullptr;
    if (mapped) {
        const BlockGroup &gr = grp[g];
        if (gr.merged >= 0) {
            l0 = merged[gr.merged].data();
            l1 = l0 + merged[gr.merged].size();
        } else {
            l0 = h_leaves + h_off[gr.first_read];   // (ascending within a read, no duplicates)
            l1 = h_leaves + h_off[gr.first_read + 1];
        }
    }
    put_record(mapped ? pb : nb, b, r, l0, l1, names);
}
// One block on its own: reads [0, n) of b through the block's map, appended to pb / nb (--device-output: the blocks the device
// leaves to the host).
struct BlockFormatter {
    std::vector<BlockGroup> grp;
    std::vector<uint32_t> tab;
    std::vector<int32_t> grp_of;
    std::vector<std::vector<uint32_t>> merged;
    void run(const Batch &b, const uint64_t *h_off, const uint32_t *h_leaves, bool pos, bool neg, const std::vector<std::string> &names, OutBuf &pb,
             OutBuf &nb) {
        const uint64_t n = b.n();
        uint64_t n_hit = 0;
        for (uint64_t r = 0; r < n; ++r) n_hit += h_off[r] != h_off[r + 1];
        grp.resize(n_hit);
        tab.assign(block_table_slots(n_hit), 0);
        grp_of.resize(n);
        map_block(b, 0, n, h_off, h_leaves, grp.data(), tab.data(), tab.size(), merged, grp_of.data());
        for (uint64_t r = 0; r < n; ++r) put_block_record(pb, nb, b, r, grp_of[r], grp.data(), merged, h_off, h_leaves, pos, neg, names);
    }
};

// The three query loops over an open database, the reader and the outputs.
struct QueryLoop {
    ServedDb &db;
    ReadQueue &rq;
    Outputs &out;
    const QueryOptions &o;
    PrepRun &prep;  // read preprocessing (o.prep): every call trims and filters its reads on the device first and adds to these totals
    const uint64_t kmer_size;
    // what the post-stages ask of every call: --abundance logs the hit rows, --coverage sketches the listed genomes' matched k-mers,
    // --taxonomy counts the units on the taxonomy's nodes, --best-hits gives the three every unit's best-scoring genomes, --sweep
    // counts rows and scores against the threshold list (the last two: the library is asked for hits and scores)
    uint32_t abundance_flags() const {
        return (o.abundance ? (PFQ_WANT_HITS | PFQ_WANT_ABUNDANCE) : 0u) | (o.coverage ? (PFQ_WANT_HITS | PFQ_WANT_COVERAGE) : 0u) |
               (o.taxonomy ? (PFQ_WANT_HITS | PFQ_WANT_TAXA) : 0u) | (o.best_hits ? (PFQ_WANT_HITS | PFQ_WANT_SCORES | PFQ_ROWS_BEST) : 0u) |
               (o.sweep ? (PFQ_WANT_HITS | PFQ_WANT_SCORES | PFQ_WANT_SWEEP) : 0u);
    }
    uint32_t lca_flags() const { return o.lca == 0 ? 0u : o.lca == 1 ? PFQ_WANT_LCA : (PFQ_WANT_LCA | PFQ_LCA_BEST | PFQ_WANT_HITS | PFQ_WANT_SCORES); }
    std::atomic<uint64_t> ns_gpu{0}, ns_out{0}, n_total{0};

    size_t n_trees() const { return db.trees.size(); }
    uint64_t batch_size(uint64_t target) const {  // a whole number of reference blocks
        if (const char *e = getenv("PFQ_CLI_BATCH_READS")) target = std::max<uint64_t>(1, strtoull(e, nullptr, 10));  // (tests: several batches)
        return std::max<uint64_t>(o.block, target) / o.block * o.block;
    }

    // Fragments, batch by batch: the parsers fill a batch of whole fragments (mates adjacent, -b counts fragments); every
    // replica classifies a contiguous share of its fragments (every shard: all of them) with PFQ_PAIRED on its own thread,
    // so no batch, device share or shard slot splits a pair; then the batch is written.  Without filtering or scores the
    // calls want counts only.
    void paired(ReadQueue *rq2, bool both) {
        const uint64_t batch_frags = batch_size(1u << 19);
        const bool per_read = o.pos || o.neg || o.scores || o.lca_reads || o.taxon_reads;
        const uint32_t flags = PFQ_PAIRED | (both ? PFQ_PAIR_BOTH : 0u) | (per_read ? PFQ_WANT_HITS : 0u) | (o.scores ? PFQ_WANT_SCORES : 0u) | lca_flags() |
                               abundance_flags();
        PairSource src{rq, rq2, {}, {}, 0, {}, false};
        Batch b;
        std::vector<Hits> parts(n_trees());
        Hits f;  // the fragments' lists in the whole tree's leaf order
        OutBuf pos_out, neg_out, pos2_out, neg2_out;
        std::string sc_out, lca_out, taxa_out;
        std::vector<uint64_t> order;
        bool more = true;
        while (more) {
            b.clear();
            more = src.next(b, batch_frags);
            const uint64_t n = b.n();
            uint64_t nf = n / 2;
            if (!nf) continue;
            b.seq.resize(b.seq.size() + 16);
            const uint64_t tq0 = ReadQueue::now_ns();
            const bool map_back = per_read && o.prep;  // (the rows of the kept fragments are mapped back through kept, begin and len)
            std::vector<PrepKept> pks(map_back ? n_trees() : 0);
            std::vector<uint64_t> share(n_trees() + 1, 0);
            fan_out(n_trees(), [&](size_t i) {
                const size_t P = n_trees();
                const uint64_t f0 = db.sharded ? 0 : nf * i / P, f1 = db.sharded ? nf : nf * (i + 1) / P;
                share[i] = 2 * f0;
                classify(db.trees[i], b, 2 * f0, 2 * f1, o, flags, parts[i], prep, map_back ? &pks[i] : nullptr);
            });
            ns_gpu += ReadQueue::now_ns() - tq0;
            n_total += n;
            if (!per_read) continue;
            std::vector<uint64_t> cuts;
            if (map_back) {
                cuts = keep_prepared(b, share, pks);
                for (uint64_t &c : cuts) c /= 2;
                nf = cuts.back();
            }
            merge_hits(parts, nf, db, f, map_back ? &cuts : nullptr);
            // every mate with its own id and its fragment's genomes; a fragment with genomes goes to POS, both mates alike
            pos_out.n = neg_out.n = pos2_out.n = neg2_out.n = 0;
            sc_out.clear();
            for (uint64_t fr = 0; fr < nf; ++fr) {
                const uint32_t *l0 = f.leaves.data() + f.off[fr], *l1 = f.leaves.data() + f.off[fr + 1];
                const bool mapped = l0 != l1;
                if (mapped ? !o.pos : !o.neg) continue;
                for (uint64_t r = 2 * fr; r < 2 * fr + 2; ++r)
                    put_record((r & 1) && rq2 ? (mapped ? pos2_out : neg2_out) : (mapped ? pos_out : neg_out), b, r, l0, l1, db.leaf_names);
            }
            if (o.scores) {
                // READ_SCORES.tsv: per fragment with hits (R1's id), both mates' k-mers and matched k-mers per genome
                for (uint64_t fr = 0; fr < nf; ++fr) {
                    if (f.off[fr] == f.off[fr + 1]) continue;
                    const uint64_t nk = n_kmers(b.off[2 * fr + 1] - b.off[2 * fr], kmer_size) + n_kmers(b.off[2 * fr + 2] - b.off[2 * fr + 1], kmer_size);
                    put_scores(sc_out, b.id(2 * fr), nk, f.leaves.data() + f.off[fr], f.scores.data() + f.off[fr], f.off[fr + 1] - f.off[fr],
                               db.leaf_names, order);
                }
                if (!sc_out.empty() && fwrite(sc_out.data(), 1, sc_out.size(), out.scores) != sc_out.size()) die("short write to READ_SCORES.tsv");
            }
            if (o.lca_reads) {
                lca_out.clear();
                for (uint64_t fr = 0; fr < nf; ++fr)
                    if (f.off[fr] != f.off[fr + 1]) put_lca(lca_out, b.id(2 * fr), f.off[fr + 1] - f.off[fr], f.lca[fr], db.clade_names);
                if (!lca_out.empty() && fwrite(lca_out.data(), 1, lca_out.size(), out.lca) != lca_out.size()) die("short write to READ_LCA.tsv");
            }
            if (o.taxon_reads) {
                taxa_out.clear();
                for (uint64_t fr = 0; fr < nf; ++fr)
                    if (f.off[fr] != f.off[fr + 1]) put_lca(taxa_out, b.id(2 * fr), f.off[fr + 1] - f.off[fr], f.taxa[fr], db.taxon_names);
                if (!taxa_out.empty() && fwrite(taxa_out.data(), 1, taxa_out.size(), out.taxa) != taxa_out.size()) die("short write to READ_TAXA.tsv");
            }
            out.pos.append(pos_out.p, pos_out.n);
            out.neg.append(neg_out.p, neg_out.n);
            out.pos2.append(pos2_out.p, pos2_out.n);
            out.neg2.append(neg2_out.p, neg2_out.n);
        }
        if (!src.err.empty()) rq.pending_error = src.err;  // fatal later, after the outputs of the fragments before it
    }

    // --frame: sequences batch by batch, whole sequences dealt to the replicas in contiguous shares (a sequence's segments and
    // its count need all of its frames), each share one pfq_query_frames on the replica's own thread; then the batch's lines
    // are written in input order.  A batch is cut by sequences (PFQ_CLI_BATCH_READS) and by bases, so that the frames' bytes of
    // one call — its bases times frame / step — stay near 1 GiB and its frames far below the call's limit; a sequence larger
    // than that is a call of its own.  The results do not depend on the cut.
    void frames(uint32_t frame, uint32_t step, const std::string &tsv) {
        FILE *f = fopen(tsv.c_str(), "wb");
        if (!f) die("cannot create " + tsv);
        fputs("sequence\tgenome\tbegin\tend\tmatch_begin\tmatch_end\tframes\tkmers\tmatched\tlongest_run\n", f);
        const uint64_t batch_seqs = batch_size(1u << 16);
        const uint64_t batch_bases = std::max<uint64_t>(1, (uint64_t)((double)(1ull << 30) * step / frame));
        struct Part {
            std::vector<uint64_t> off, call_off;
            std::vector<pfq_segment> seg;
        };
        std::vector<Part> parts(n_trees());
        Batch b;
        std::string lines;
        char num[128];
        bool more = true;
        while (more) {
            b.clear();
            more = rq.fill(b, batch_seqs, batch_bases);
            const uint64_t n = b.n();
            if (!n) continue;
            b.seq.resize(b.seq.size() + 16);
            const uint64_t tq0 = ReadQueue::now_ns();
            fan_out(n_trees(), [&](size_t i) {
                const size_t P = n_trees();
                const uint64_t r0 = n * i / P, r1 = n * (i + 1) / P;
                Part &p = parts[i];
                p.off.assign(r1 - r0 + 1, 0);
                p.seg.clear();
                if (r1 == r0) return;
                p.call_off.resize(r1 - r0 + 1);
                for (uint64_t r = r0; r <= r1; ++r) p.call_off[r - r0] = b.off[r] - b.off[r0];
                pfq_segments sg{};
                if (pfq_query_frames(db.trees[i], b.seq.data() + b.off[r0], p.call_off.data(), r1 - r0, frame, step, o.threshold, 0, &sg) != PFQ_OK)
                    fail_from_thread(pfq_last_error());
                p.off.assign(sg.offsets, sg.offsets + (r1 - r0) + 1);
                p.seg.assign(sg.seg, sg.seg + sg.offsets[r1 - r0]);
            });
            ns_gpu += ReadQueue::now_ns() - tq0;
            n_total += n;
            lines.clear();
            for (size_t i = 0; i < n_trees(); ++i) {
                const uint64_t r0 = n * i / n_trees();
                const Part &p = parts[i];
                for (uint64_t u = 0; u + 1 < p.off.size(); ++u)
                    for (uint64_t j = p.off[u]; j < p.off[u + 1]; ++j) {
                        const pfq_segment &s = p.seg[j];
                        const std::string_view id = b.id(r0 + u);
                        lines.append(id.data(), id.size());
                        lines.push_back('\t');
                        lines.append(db.leaf_names[s.leaf]);
                        lines.append(num, (size_t)snprintf(num, sizeof num, "\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", s.begin, s.end, s.match_begin, s.match_end,
                                                           s.n_frames, s.kmers, s.matched, s.longest_run));
                    }
            }
            if (!lines.empty() && fwrite(lines.data(), 1, lines.size(), f) != lines.size()) die("short write to SEGMENTS.tsv");
        }
        if (fclose(f) != 0) die("short write to SEGMENTS.tsv");
    }

    // Counts only: the next parsed segment in input order, padded for the device, or nullptr at the end of the input.
    // `end`: nothing follows it — malformed input ends the input (the reads before it are still classified).
    Segment *fetch_segment(bool &end) {
        Segment *sg = rq.next_segment();
        end = !sg || !sg->err.empty();
        if (!sg) return nullptr;
        if (!sg->err.empty()) rq.pending_error = sg->err;
        if (sg->b.n()) sg->b.seq.resize(sg->b.seq.size() + 16);
        return sg;
    }
    void count_segment(size_t i, const Segment &sg, Hits &unused) {
        const uint64_t n = sg.b.n();
        if (!n) return;
        const uint64_t tq0 = ReadQueue::now_ns();
        classify(db.trees[i], sg.b, 0, n, o, lca_flags(), unused, prep);
        ns_gpu += ReadQueue::now_ns() - tq0;
        if (!db.sharded || i == 0) n_total += n;
    }
    // Counts only: the result does not depend on how the reads are cut into device calls (mapped_reads just accumulates,
    // query.rs:143), so every parsed segment goes to a GPU as it is — no host-side copy.
    //   replicas: segments are handed out in input order to whichever replica's thread asks next;
    //   shards: every segment goes to every shard's thread; segment k sits in ring[k % W] until the last shard is done with
    //   it, then goes back to the reader.  W is what the reader's pool takes back, so at most W segments are in flight and
    //   a shard at most W segments ahead of the slowest one.  One thread at a time takes the next segment from the reader
    //   (outside the lock: the others go on with the segments already taken).
    void counts_only() {
        std::mutex qm;
        if (!db.sharded) {
            bool done = false;
            fan_out(n_trees(), [&](size_t d) {
                Hits unused;
                while (true) {
                    Segment *sg;
                    {
                        std::lock_guard<std::mutex> lk(qm);
                        if (done) return;
                        if (!(sg = fetch_segment(done))) return;
                    }
                    count_segment(d, *sg, unused);
                    rq.recycle(sg);
                }
            });
            return;
        }
        const size_t W = rq.pool_cap();
        std::vector<Segment *> ring(W, nullptr);
        std::vector<size_t> shards_left(W, 0);
        std::condition_variable qcv;
        uint64_t fetched = 0;      // segments taken from the reader
        bool fetching = false;
        long long n_seg = -1;      // number of segments, once the end of the input (or malformed input) is reached
        fan_out(n_trees(), [&](size_t i) {
            Hits unused;
            for (uint64_t k = 0;; ++k) {
                const size_t slot = (size_t)(k % W);
                Segment *sg = nullptr;
                {
                    std::unique_lock<std::mutex> lk(qm);
                    qcv.wait(lk, [&] {
                        return k < fetched || (n_seg >= 0 && (long long)k >= n_seg) || (k == fetched && !fetching && !ring[slot]);
                    });
                    if (n_seg >= 0 && (long long)k >= n_seg) return;
                    if (k == fetched) {
                        fetching = true;
                        lk.unlock();
                        bool end;
                        sg = fetch_segment(end);
                        lk.lock();
                        fetching = false;
                        if (end) n_seg = (long long)k + (sg ? 1 : 0);
                        if (sg) {
                            ring[slot] = sg;
                            shards_left[slot] = n_trees();
                            ++fetched;
                        }
                        qcv.notify_all();
                        if (!sg) return;
                    }
                    sg = ring[slot];
                }
                count_segment(i, *sg, unused);
                bool last;
                {
                    std::lock_guard<std::mutex> lk(qm);
                    last = --shards_left[slot] == 0;
                    if (last) ring[slot] = nullptr;
                }
                if (!last) continue;
                rq.recycle(sg);
                qcv.notify_all();
            }
        });
    }

    // --device-parse: counts only on replicas, the plain files parsed on the device.  A replica's thread takes the next segment
    // in input order (a ticket) and, if it is a chunk's bytes, has its own tree parse them from the guessed record start
    // (pfq_text_parse: speculative, no counter changes).  Then, ticket after ticket, the start is proven as next_segment proves
    // it — it must be where the chunk before ended — and a wrong guess is parsed again from the proven position; the records
    // taken are committed (proven_pos moves behind them) and classified after the turn is handed on (pfq_text_query).  Where the
    // device stopped at text that is not ordinary (SLOW) or not complete within the chunk's slack (MORE), the sequential reader
    // parses the rest of the chunk from exactly there, malformed input included; after a SLOW the file's later chunks go to
    // the reader at once.  gzip streams arrive parsed, as ever.  Counting commutes, so only the proofs are ordered.
    std::atomic<uint64_t> n_device_records{0}, n_host_records{0}, ns_text_parse{0}, n_text_bytes{0};
    // --device-inflate: blocked gzip files arrive as chunks of whole members (ReadQueue::bgzf_tasks).  A replica's thread has its
    // tree inflate the chunk it took (pfq_text_inflate: outside the turn, this is the parallel part); inside its turn the text is
    // parsed behind the carry the file's previous chunk left (pfq_text_parse_inflated), the bytes behind the last record taken
    // become the next carry (pfq_text_read), and the records are classified after the turn, as those of a plain chunk are.  Where
    // the device declines — bytes that are no member, a member it rejects, text that is not ordinary (SLOW), a carry above the
    // cap, a file that ends inside a record — the file's streaming reader takes over for the rest of the file, inside the turn:
    // it opens the file at the begin of a chunk whose first member the scan took (never at foreign bytes, which zlib would copy
    // through at the start of a stream but ignores behind a member) and discards the text up to the first record not taken.
    struct GzFile {
        std::vector<uint8_t> carry;  // the text behind the last record taken
        uint64_t text_done = 0;      // where in the file's text the carry begins: the first record not taken
        std::vector<std::pair<uint64_t, uint64_t>> chunks;  // (file offset, text offset) of the chunks whose first member the scan took
        uint64_t members_used = 0;
    };
    static constexpr uint64_t GZ_CARRY_MAX = 1ull << 20;
    std::vector<GzFile> gz_files;
    std::atomic<uint64_t> n_gz_members{0}, n_gz_host{0}, ns_inflate{0}, n_gz_bytes{0}, n_gz_text{0};
    void gz_takeover(size_t d, const Task &task, GzFile &g, uint64_t at, Fmt fmt, std::atomic<bool> &aborted) {
        rq.file_slow[task.file] = true;
        n_gz_host += rq.bgzf_members[task.file] - g.members_used;
        size_t j = g.chunks.size();
        while (j && g.chunks[j - 1].second > at) --j;
        if (!j) die("'" + rq.files[task.file] + "' changed while it was being read");
        GzLines gl(rq.files[task.file], g.chunks[j - 1].first, at - g.chunks[j - 1].second);
        RecordParser<GzLines> rp(gl, fmt);
        Hits unused;
        Segment seg;
        for (int rc = 1; rc == 1;) {
            seg.b.clear();
            while (seg.b.n() < rq.seg_reads && (rc = rp.next(seg.b, false)) == 1) {}
            if (seg.b.n()) {
                seg.b.seq.resize(seg.b.seq.size() + 16);
                n_host_records += seg.b.n();
                count_segment(d, seg, unused);
            }
            if (rc < 0) {
                rq.pending_error = rp.err;  // (fatal later, after the reads before it)
                aborted = true;
            }
        }
    }
    // The turn of a chunk of members; returns the records the device parsed, which the caller classifies after the turn.
    uint64_t gz_turn(size_t d, pfq_tree *tree, const Task &task, const pfq_text_inflated *inf, Fmt fmt, std::atomic<bool> &aborted) {
        GzFile &g = gz_files[task.file];
        const uint64_t text0 = g.text_done + g.carry.size();  // where in the file's text this chunk's first member begins
        if (inf && inf->members.n_members) g.chunks.push_back({task.lo, text0});
        bool decline = task.bgzf_tail || !inf || inf->members.stop != PFQ_GZ_END || inf->members.consumed != task.hi - task.lo ||
                       inf->n_good < inf->members.n_members || ((g.carry.size() + inf->good_text) >> 31);
        uint64_t n_dev = 0, takeover_at = g.text_done;
        if (!decline) {
            pfq_text res{};
            const uint64_t t0 = ReadQueue::now_ns();
            if (pfq_text_parse_inflated(tree, g.carry.data(), g.carry.size(), ~0ull, fmt == Fmt::Fastq ? PFQ_TEXT_FASTQ : PFQ_TEXT_FASTA,
                                        task.last_of_file ? PFQ_TEXT_FINAL : 0u, &res) != PFQ_OK)
                fail_from_thread(pfq_last_error());
            ns_text_parse += ReadQueue::now_ns() - t0;
            const uint64_t len = g.carry.size() + inf->good_text, rest = len - res.consumed;
            n_text_bytes += len;
            n_dev = res.n_records;
            takeover_at = g.text_done + res.consumed;
            if (res.stop == PFQ_TEXT_SLOW || rest > GZ_CARRY_MAX || (task.last_of_file && rest)) decline = true;
            else {
                g.carry.resize(rest);
                if (rest && pfq_text_read(tree, res.consumed, rest, g.carry.data()) != PFQ_OK) fail_from_thread(pfq_last_error());
                g.text_done = takeover_at;
                g.members_used += inf->members.n_members;
                n_gz_members += inf->members.n_members;
            }
        }
        if (decline) gz_takeover(d, task, g, takeover_at, fmt, aborted);
        return n_dev;
    }
    void report_device_inflate() const {
        const double s = ns_inflate.load() * 1e-9;
        fprintf(stderr, "device inflate: %llu members inflated on the device, %llu handed to the host reader; pfq_text_inflate took %llu compressed bytes (%llu bytes of text) in %.3f s (%.2f GB/s of text, copy and kernel, summed over devices)\n",
                (unsigned long long)n_gz_members.load(), (unsigned long long)n_gz_host.load(), (unsigned long long)n_gz_bytes.load(),
                (unsigned long long)n_gz_text.load(), s, s > 0 ? n_gz_text.load() / s * 1e-9 : 0.0);
    }
    void counts_only_text() {
        gz_files.resize(rq.files.size());
        std::mutex take_mu, turn_mu;
        std::condition_variable turn_cv;
        uint64_t taken = 0, commit_next = 0;
        std::atomic<bool> exhausted{false}, aborted{false};  // no segment is left; malformed input was met: later tickets are dropped
        fan_out(n_trees(), [&](size_t d) {
            pfq_tree *tree = db.trees[d];
            Hits unused;
            while (true) {
                Segment *sg;
                const Task *task = nullptr;
                uint64_t ticket;
                {
                    std::lock_guard<std::mutex> lk(take_mu);
                    if (exhausted || aborted) return;
                    if (!(sg = rq.pop_segment(task))) {
                        exhausted = true;
                        return;
                    }
                    ticket = taken++;
                }
                const MappedFile &m = rq.maps[task->file];
                const Fmt fmt = rq.fmts[task->file];
                pfq_text res{};
                uint64_t parsed_from = ~0ull;
                auto parse_from = [&](uint64_t from) {  // the chunk's records from file offset `from` on
                    parsed_from = from;
                    res = pfq_text{};
                    res.stop = PFQ_TEXT_LIMIT;
                    if (from >= task->hi || from > sg->text_hi) return;  // (no record of this chunk begins there)
                    const uint64_t t0 = ReadQueue::now_ns();
                    if (pfq_text_parse(tree, (const uint8_t *)sg->text.p + (from - sg->text_lo), sg->text_hi - from, task->hi - from,
                                       fmt == Fmt::Fastq ? PFQ_TEXT_FASTQ : PFQ_TEXT_FASTA, sg->text_hi == m.size ? PFQ_TEXT_FINAL : 0u, &res) != PFQ_OK)
                        fail_from_thread(pfq_last_error());
                    ns_text_parse += ReadQueue::now_ns() - t0;
                    n_text_bytes += sg->text_hi - from;
                };
                if (sg->is_text && !rq.file_slow[task->file]) parse_from(sg->start_pos);
                pfq_text_inflated inf{};
                bool inflated = false;
                if (sg->is_gz && sg->text_hi > sg->text_lo && !rq.file_slow[task->file] && !aborted) {
                    const uint64_t t0 = ReadQueue::now_ns();
                    if (pfq_text_inflate(tree, (const uint8_t *)sg->text.p, sg->text_hi - sg->text_lo, 0, task->last_of_file ? PFQ_TEXT_FINAL : 0u, &inf) != PFQ_OK)
                        fail_from_thread(pfq_last_error());
                    ns_inflate += ReadQueue::now_ns() - t0;
                    n_gz_bytes += inf.members.consumed;
                    n_gz_text += inf.members.text_bytes;
                    inflated = true;
                }
                {
                    std::unique_lock<std::mutex> lk(turn_mu);
                    turn_cv.wait(lk, [&] { return commit_next == ticket; });
                }
                // (the turn: one thread at a time, in the order the segments were taken)
                const bool dropped = aborted;
                uint64_t n_dev = 0;
                if (!dropped && sg->is_gz) {
                    if (!rq.file_slow[task->file]) n_dev = gz_turn(d, tree, *task, inflated ? &inf : nullptr, fmt, aborted);
                } else if (!dropped && sg->is_text) {
                    const uint64_t expect = rq.expected_start(*task);
                    bool host_rest = rq.file_slow[task->file];
                    uint64_t rest_from = expect;
                    if (!host_rest) {
                        if (parsed_from != expect) parse_from(expect);  // the guess was wrong (or a record spans chunks)
                        n_dev = res.n_records;
                        rest_from = expect + res.consumed;
                        if (res.stop == PFQ_TEXT_SLOW) rq.file_slow[task->file] = host_rest = true;
                        // (END short of the chunk's end in a window that is not the file's end: the window was used up, as with MORE)
                        else if (res.stop == PFQ_TEXT_MORE || (res.stop == PFQ_TEXT_END && sg->text_hi != m.size && rest_from < task->hi)) host_rest = true;
                    }
                    if (host_rest) {
                        rq.parse_chunk(m, fmt, task->lo, task->hi, true, rest_from, *sg);
                        rq.proven_pos = sg->end_pos;
                    } else rq.proven_pos = rest_from;
                    sg->is_text = false;
                } else if (!dropped) rq.validate(*task, *sg);
                if (!dropped && !sg->err.empty()) {
                    rq.pending_error = sg->err;  // (fatal later, after the reads before it)
                    aborted = true;
                }
                {
                    std::lock_guard<std::mutex> lk(turn_mu);
                    ++commit_next;
                }
                turn_cv.notify_all();
                if (!dropped && n_dev) {
                    const uint64_t tq0 = ReadQueue::now_ns();
                    if (pfq_text_query(tree, o.threshold, lca_flags(), nullptr) != PFQ_OK) fail_from_thread(pfq_last_error());
                    ns_gpu += ReadQueue::now_ns() - tq0;
                    n_total += n_dev;
                    n_device_records += n_dev;
                }
                if (!dropped && sg->b.n()) {
                    sg->b.seq.resize(sg->b.seq.size() + 16);
                    n_host_records += sg->b.n();
                    count_segment(d, *sg, unused);
                }
                rq.recycle(sg);
            }
        });
    }
    void report_device_parse() const {
        const double s = ns_text_parse.load() * 1e-9;
        fprintf(stderr, "device parse: %llu records parsed on the device, %llu by the host reader; pfq_text_parse took %llu bytes in %.3f s (%.2f GB/s, copy and kernels, summed over devices)\n",
                (unsigned long long)n_device_records.load(), (unsigned long long)n_host_records.load(), (unsigned long long)n_text_bytes.load(), s,
                s > 0 ? n_text_bytes.load() / s * 1e-9 : 0.0);
    }

    // --device-output: POS / NEG on replicas with the plain files parsed AND formatted on the device.  Tickets as in
    // counts_only_text: a replica's thread parses its chunk (with the records' begins), proves the start in its turn — which also
    // gives the chunk's first global record index — then classifies with hit lists (pfq_text_query) and formats
    // (pfq_text_format: the whole result blocks whose ids are pairwise different).  A second ordered turn is the output stage:
    // the device streams are written as they are; a block with a repeated id is parsed on the host from the chunk's own bytes
    // and goes through the block map with the hits the query call already returned; the records at the chunk's edges (HEAD,
    // TAIL) and everything the host reader parsed (gzip, the rest of a chunk after SLOW / MORE, malformed tails: classify())
    // go into a carry that becomes a block when it holds `block` records, or at the end of the input.
    std::atomic<uint64_t> n_fmt_device{0}, n_fmt_host{0}, ns_text_format{0}, n_fmt_bytes{0}, n_fmt_gz_bytes{0};
    double ms_deflate = 0.0;  // --gzip-output: the deflate kernels (pfq_debug_last_deflate), summed in the output turns
    void device_output() {
        std::mutex take_mu, turn_mu;
        std::condition_variable turn_cv;
        uint64_t taken = 0, commit_next = 0, write_next = 0, next_index = 0;
        std::atomic<bool> exhausted{false}, aborted{false};
        const uint32_t fmt_flags = (o.pos ? PFQ_FMT_POS : 0u) | (o.neg ? PFQ_FMT_NEG : 0u);
        const uint32_t query_flags = PFQ_WANT_HITS | lca_flags();
        // the output stage's state: touched only inside the output turn (and after the threads have joined)
        Batch carry;
        std::vector<uint64_t> carry_off{0};
        std::vector<uint32_t> carry_leaves;
        BlockFormatter bf;
        OutBuf pb, nb;
        auto write_block = [&](const Batch &b, const uint64_t *h_off, const uint32_t *h_leaves) {
            pb.n = nb.n = 0;
            bf.run(b, h_off, h_leaves, o.pos, o.neg, db.leaf_names, pb, nb);
            out.pos.append(pb.p, pb.n);
            out.neg.append(nb.p, nb.n);
            n_fmt_host += b.n();
        };
        auto flush_carry = [&] {
            if (!carry.n()) return;
            write_block(carry, carry_off.data(), carry_leaves.data());
            carry.clear();
            carry_off.assign(1, 0);
            carry_leaves.clear();
        };
        // records [r0, r1) of src with their rows (h_off relative to h_leaves) join the carry; it is written whenever it is a block
        auto carry_add = [&](const Batch &src, uint64_t r0, uint64_t r1, const uint64_t *h_off, const uint32_t *h_leaves) {
            while (r0 < r1) {
                const uint64_t take = std::min<uint64_t>(r1 - r0, o.block - carry.n());
                carry.append(src, r0, r0 + take, true);
                carry_leaves.insert(carry_leaves.end(), h_leaves + h_off[r0], h_leaves + h_off[r0 + take]);
                for (uint64_t r = r0 + 1; r <= r0 + take; ++r) carry_off.push_back(carry_off.back() + (h_off[r] - h_off[r - 1]));
                r0 += take;
                if (carry.n() == o.block) flush_carry();
            }
        };
        fan_out(n_trees(), [&](size_t d) {
            pfq_tree *tree = db.trees[d];
            Hits host_hits;
            Batch run_b;                       // a left run parsed on the host
            std::vector<uint64_t> left_off;    // the rows of the left runs, copied before the tree's next query call
            std::vector<uint32_t> left_leaves;
            while (true) {
                Segment *sg;
                const Task *task = nullptr;
                uint64_t ticket;
                {
                    std::lock_guard<std::mutex> lk(take_mu);
                    if (exhausted || aborted) return;
                    if (!(sg = rq.pop_segment(task))) {
                        exhausted = true;
                        return;
                    }
                    ticket = taken++;
                }
                const MappedFile &m = rq.maps[task->file];
                const Fmt fmt = rq.fmts[task->file];
                pfq_text res{};
                uint64_t parsed_from = ~0ull;
                auto parse_from = [&](uint64_t from) {  // the chunk's records from file offset `from` on
                    parsed_from = from;
                    res = pfq_text{};
                    res.stop = PFQ_TEXT_LIMIT;
                    if (from >= task->hi || from > sg->text_hi) return;  // (no record of this chunk begins there)
                    const uint64_t t0 = ReadQueue::now_ns();
                    if (pfq_text_parse(tree, (const uint8_t *)sg->text.p + (from - sg->text_lo), sg->text_hi - from, task->hi - from,
                                       fmt == Fmt::Fastq ? PFQ_TEXT_FASTQ : PFQ_TEXT_FASTA,
                                       (sg->text_hi == m.size ? PFQ_TEXT_FINAL : 0u) | PFQ_TEXT_WANT_RECORDS, &res) != PFQ_OK)
                        fail_from_thread(pfq_last_error());
                    ns_text_parse += ReadQueue::now_ns() - t0;
                    n_text_bytes += sg->text_hi - from;
                };
                if (sg->is_text && !rq.file_slow[task->file]) parse_from(sg->start_pos);
                {
                    std::unique_lock<std::mutex> lk(turn_mu);
                    turn_cv.wait(lk, [&] { return commit_next == ticket; });
                }
                // (the proof turn: one thread at a time, in the order the segments were taken)
                const bool dropped = aborted;
                const bool was_text = sg->is_text;
                uint64_t n_dev = 0, first_index = 0;
                if (!dropped && was_text) {
                    const uint64_t expect = rq.expected_start(*task);
                    bool host_rest = rq.file_slow[task->file];
                    uint64_t rest_from = expect;
                    if (!host_rest) {
                        if (parsed_from != expect) parse_from(expect);  // the guess was wrong (or a record spans chunks)
                        n_dev = res.n_records;
                        rest_from = expect + res.consumed;
                        if (res.stop == PFQ_TEXT_SLOW) rq.file_slow[task->file] = host_rest = true;
                        else if (res.stop == PFQ_TEXT_MORE || (res.stop == PFQ_TEXT_END && sg->text_hi != m.size && rest_from < task->hi)) host_rest = true;
                    }
                    if (host_rest) {
                        rq.parse_chunk(m, fmt, task->lo, task->hi, true, rest_from, *sg);
                        rq.proven_pos = sg->end_pos;
                    } else rq.proven_pos = rest_from;
                    sg->is_text = false;
                } else if (!dropped) rq.validate(*task, *sg);
                if (!dropped) {
                    first_index = next_index;
                    next_index += n_dev + sg->b.n();
                    if (!sg->err.empty()) {
                        rq.pending_error = sg->err;  // (fatal later, after the reads before it)
                        aborted = true;
                    }
                }
                {
                    std::lock_guard<std::mutex> lk(turn_mu);
                    ++commit_next;
                }
                turn_cv.notify_all();
                // ---- outside the turns: classify and format the device's records, classify the host's
                pfq_text_records recs{};
                pfq_bgzf pos_gz{}, neg_gz{};  // --gzip-output: the streams as the device deflated them, a piece between two left runs
                double deflate_ms[3] = {0.0, 0.0, 0.0};
                if (!dropped && n_dev) {
                    const uint64_t tq0 = ReadQueue::now_ns();
                    pfq_hits hits{};
                    if (pfq_text_query(tree, o.threshold, query_flags, &hits) != PFQ_OK) fail_from_thread(pfq_last_error());
                    const uint64_t tq1 = ReadQueue::now_ns();
                    if ((o.gzip_output ? pfq_text_format_gz(tree, first_index, (uint32_t)o.block, fmt_flags, &recs, &pos_gz, &neg_gz)
                                       : pfq_text_format(tree, first_index, (uint32_t)o.block, fmt_flags, &recs)) != PFQ_OK)
                        fail_from_thread(pfq_last_error());
                    if (o.gzip_output && pos_gz.n_members + neg_gz.n_members && pfq_debug_last_deflate(tree, deflate_ms) != PFQ_OK) fail_from_thread(pfq_last_error());
                    n_fmt_gz_bytes += pos_gz.gz_bytes + neg_gz.gz_bytes;
                    ns_text_format += ReadQueue::now_ns() - tq1;
                    ns_gpu += tq1 - tq0;
                    n_fmt_bytes += recs.pos_bytes + recs.neg_bytes;
                    n_total += n_dev;
                    n_device_records += n_dev;
                    left_off.assign(1, 0);
                    left_leaves.clear();
                    for (uint64_t i = 0; i < recs.n_left; ++i) {  // (the library's hit lists live until the tree's next query call)
                        const pfq_text_left &l = recs.left[i];
                        left_leaves.insert(left_leaves.end(), hits.leaves + hits.offsets[l.first], hits.leaves + hits.offsets[l.first + l.count]);
                        for (uint64_t r = l.first + 1; r <= l.first + l.count; ++r) left_off.push_back(left_off.back() + (hits.offsets[r] - hits.offsets[r - 1]));
                    }
                }
                const uint64_t n_host = dropped ? 0 : sg->b.n();
                if (n_host) {
                    sg->b.seq.resize(sg->b.seq.size() + 16);
                    const uint64_t tq0 = ReadQueue::now_ns();
                    classify(tree, sg->b, 0, n_host, o, query_flags, host_hits, prep);
                    ns_gpu += ReadQueue::now_ns() - tq0;
                    n_total += n_host;
                    n_host_records += n_host;
                }
                {
                    std::unique_lock<std::mutex> lk(turn_mu);
                    turn_cv.wait(lk, [&] { return write_next == ticket; });
                }
                // (the output turn: one thread at a time, in input order)
                const uint64_t t_out0 = ReadQueue::now_ns();
                // the device's bytes between left run i - 1 and left run i (i = n_left: behind the last)
                auto device_bytes = [&](uint64_t i, uint64_t pc, uint64_t qc, uint64_t p_end, uint64_t q_end) {
                    if (o.gzip_output) {
                        out.pos.append_raw((const char *)pos_gz.gz + pos_gz.piece_begin[i], pos_gz.piece_begin[i + 1] - pos_gz.piece_begin[i]);
                        out.neg.append_raw((const char *)neg_gz.gz + neg_gz.piece_begin[i], neg_gz.piece_begin[i + 1] - neg_gz.piece_begin[i]);
                    } else {
                        out.pos.append((const char *)recs.pos + pc, p_end - pc);
                        out.neg.append((const char *)recs.neg + qc, q_end - qc);
                    }
                };
                if (!dropped && n_dev) {
                    const char *text = sg->text.p - sg->text_lo;  // (the address byte 0 of the file would have)
                    uint64_t pc = 0, qc = 0, left_rows = 0, n_left_records = 0;
                    ms_deflate += deflate_ms[1];
                    for (uint64_t i = 0; i < recs.n_left; ++i) {
                        const pfq_text_left &l = recs.left[i];
                        device_bytes(i, pc, qc, l.pos_at, l.neg_at);
                        pc = l.pos_at;
                        qc = l.neg_at;
                        run_b.clear();
                        MemLines ml(text, parsed_from + res.rec_begin[l.first], parsed_from + res.rec_begin[l.first + l.count]);
                        RecordParser<MemLines> rp(ml, fmt);
                        while (run_b.n() < l.count && rp.next(run_b, true) == 1) {}
                        if (run_b.n() != l.count) fail_from_thread("internal error: the host reader and the device disagree about a chunk's records");
                        const uint64_t *off = left_off.data() + left_rows;  // (rows of this run; relative to off[0])
                        std::vector<uint64_t> rel(l.count + 1);
                        for (uint64_t r = 0; r <= l.count; ++r) rel[r] = off[r] - off[0];
                        if (l.why == PFQ_LEFT_REPEATED_ID) write_block(run_b, rel.data(), left_leaves.data() + off[0]);
                        else carry_add(run_b, 0, l.count, rel.data(), left_leaves.data() + off[0]);
                        left_rows += l.count;
                        n_left_records += l.count;
                    }
                    device_bytes(recs.n_left, pc, qc, recs.pos_bytes, recs.neg_bytes);
                    n_fmt_device += n_dev - n_left_records;
                }
                if (n_host) carry_add(sg->b, 0, n_host, host_hits.off.data(), host_hits.leaves.data());
                ns_out += ReadQueue::now_ns() - t_out0;
                {
                    std::lock_guard<std::mutex> lk(turn_mu);
                    ++write_next;
                }
                turn_cv.notify_all();
                rq.recycle(sg);
            }
        });
        flush_carry();  // the last block of the input is a partial one
    }
    void report_device_output() const {
        const double s = ns_text_format.load() * 1e-9;
        fprintf(stderr, "device output: %llu records formatted on the device, %llu by the host formatter; pfq_text_format made %llu bytes in %.3f s (%.2f GB/s, kernels and copy, summed over devices)",
                (unsigned long long)n_fmt_device.load(), (unsigned long long)n_fmt_host.load(), (unsigned long long)n_fmt_bytes.load(), s,
                s > 0 ? n_fmt_bytes.load() / s * 1e-9 : 0.0);
        if (o.gzip_output)
            fprintf(stderr, "; deflated on the device to %llu bytes, %.3f s in the deflate kernels (of each call's last stream)", (unsigned long long)n_fmt_gz_bytes.load(),
                    ms_deflate * 1e-3);
        fprintf(stderr, "\n");
    }

    // Per read, with POS/NEG and/or READ_SCORES.  The device processes big batches; ResultMap semantics (ids merged per
    // reference block, cleared per block, main.rs:334-368) are applied per `block` consecutive reads so the outputs do not
    // depend on the batch size.  Three stages, each on its own thread(s), batches in flight between them: (1) the
    // assembler (above all the copy of the parsed records into batches of whole reference blocks), (2) one thread per
    // tree: pfq_query_batch with hits, which are copied out of the library's buffers, (3) ONE output thread that takes the
    // classified batches in input order, formats them with `threads` workers and writes every worker's part at its offset
    // (pwrite, side by side) — while batch k is formatted and written, batch k + 1 is on the GPU and batch k + 2 is being
    // assembled.
    void per_read() {
        const uint64_t batch_reads = batch_size(1u << 20);
        struct Slot {
            Batch b;
            int ready = 0;            // 0 = free for the assembler, 1 = filled, 2 = classified
            uint64_t seq = 0;         // which batch the slot holds
            size_t trees_left = 0;    // trees that have yet to classify it
            std::vector<Hits> parts;  // per tree (a replica: one)
            Hits hits;                // the whole tree's
        };
        std::vector<Slot> slots(db.devices.size() + 3);
        const size_t NB = slots.size();
        for (Slot &s : slots) s.parts.resize(db.sharded ? n_trees() : 1);
        const uint32_t query_flags = PFQ_WANT_HITS | (o.scores ? PFQ_WANT_SCORES : 0u) | lca_flags() | abundance_flags();
        std::mutex mu;
        std::condition_variable cv;
        long long last_seq = -1;                 // sequence number of the last batch, once the assembler knows it
        auto past_end = [&](uint64_t k) { return last_seq >= 0 && (long long)k > last_seq; };
        uint64_t next_take = 0;
        std::atomic<uint64_t> ns_fmt{0}, ns_write{0};
        std::thread parser([&] {
            bool more = true;
            for (uint64_t k = 0; more; ++k) {
                Slot &s = slots[k % NB];
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return s.ready == 0; });
                }
                rq.release_held(s.b);  // (written: its segments go back to the parsers)
                s.b.clear();
                more = rq.fill(s.b, batch_reads, 3ull << 30, true);
                // padded here, once: every shard's thread reads the batch at the same time
                if (s.b.n()) s.b.seq.resize(s.b.seq.size() + 16);
                {
                    std::lock_guard<std::mutex> lk(mu);
                    s.trees_left = db.sharded ? n_trees() : 1;
                    s.ready = 1;
                    s.seq = k;
                    if (!more) last_seq = (long long)k;
                }
                cv.notify_all();
            }
        });
        // A replica's thread takes the next batch nobody has taken; a shard's thread takes every batch.  The thread that
        // classifies a batch last merges the trees' hits (shards: see merge_hits) and hands it to the output thread.
        auto classify_loop = [&](size_t i) {
            for (uint64_t mine = 0;;) {
                uint64_t k;
                Slot *s;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    k = db.sharded ? mine++ : next_take++;
                    s = &slots[k % NB];
                    cv.wait(lk, [&] { return (s->ready == 1 && s->seq == k) || past_end(k); });
                    if (past_end(k)) return;
                }
                uint64_t n = s->b.n();
                const uint64_t tq0 = ReadQueue::now_ns();
                std::vector<PrepKept> pks(o.prep ? 1 : 0);
                classify(db.trees[i], s->b, 0, n, o, query_flags, s->parts[db.sharded ? i : 0], prep, o.prep ? &pks[0] : nullptr);
                if (n) {
                    ns_gpu += ReadQueue::now_ns() - tq0;
                    if (!db.sharded || i == 0) n_total += n;
                }
                if (o.prep) n = keep_prepared(s->b, {0, n}, pks).back();  // (replicas only: this thread alone holds the batch)
                {
                    std::lock_guard<std::mutex> lk(mu);
                    if (--s->trees_left != 0) continue;
                }
                merge_hits(s->parts, n, db, s->hits);
                {
                    std::lock_guard<std::mutex> lk(mu);
                    s->ready = 2;
                }
                cv.notify_all();
            }
        };
        // (formatters and writers share the cores with the parser workers and the assembler; measured on 16 cores with
        // -t 16: 16 formatters / 16 writers 18.6 - 19.2 M reads/s, 12 / 8: 19.5 - 19.7, 8 / 4: 16.8 - 17.1.  PFQ_CLI_FMT_WORKERS /
        // PFQ_CLI_WRITERS override the split.)
        unsigned fmt_workers = std::max(1u, o.threads * 3u / 4u);
        if (const char *e = getenv("PFQ_CLI_FMT_WORKERS")) fmt_workers = std::max(1u, (unsigned)atoi(e));
        unsigned max_writers = std::max(1u, o.threads / 2u);
        if (const char *e = getenv("PFQ_CLI_WRITERS")) max_writers = std::max(1u, (unsigned)atoi(e));
        // two sets of output buffers: while the writer thread puts set s into the files, the formatters fill the other one
        std::vector<OutBuf> pos_sets[2] = {std::vector<OutBuf>(fmt_workers), std::vector<OutBuf>(fmt_workers)};
        std::vector<OutBuf> neg_sets[2] = {std::vector<OutBuf>(fmt_workers), std::vector<OutBuf>(fmt_workers)};
        std::vector<std::vector<unsigned char>> gz_parts(fmt_workers);  // --gzip-output: a worker's members before they replace its text
        struct WriteJob {
            int state = 0;  // 0 free, 1 to be written
            unsigned nw = 0;
            std::vector<uint64_t> pos_at, neg_at;
        } jobs[2];
        bool writer_done = false;
        std::thread writer([&] {
            for (uint64_t j = 0;; ++j) {
                WriteJob &job = jobs[j & 1];
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return job.state == 1 || writer_done; });
                    if (job.state != 1) return;
                }
                const uint64_t t1 = ReadQueue::now_ns();
                std::vector<OutBuf> &pb = pos_sets[j & 1], &nb = neg_sets[j & 1];
                const unsigned n_wr = std::min(job.nw, max_writers);
                fan_out(n_wr, [&](size_t x) {  // writer x takes parts x, x + n_wr, ...
                    for (size_t w = x; w < job.nw; w += n_wr) {
                        if (out.pos.fd >= 0) write_at(out.pos.fd, pb[w].p, pb[w].n, job.pos_at[w]);
                        if (out.neg.fd >= 0) write_at(out.neg.fd, nb[w].p, nb[w].n, job.neg_at[w]);
                    }
                });
                ns_write += ReadQueue::now_ns() - t1;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    job.state = 0;
                }
                cv.notify_all();
            }
        });
        std::thread output([&] {
            // The blocks' ResultMaps (map_block).  Two phases per batch: (1) workers take whole blocks: table of the block's hit
            // ids, then for EVERY read of the block its group (read_mapped: the id is in the block's map) — all hashing happens
            // here; (2) workers take equal ranges of reads and only format (a block of 100 000 reads is formatted by several
            // workers).
            std::vector<BlockGroup> groups;                       // [hit reads of the batch], a slice per block
            std::vector<uint32_t> table;                          // open-addressing tables of all blocks, a slice (power of two) per block
            std::vector<uint64_t> grp0, tab0;                     // [blocks + 1] first group / first table slot of every block
            std::vector<int32_t> grp_of;                          // [reads] group of the read within its block, -1: not mapped
            std::vector<std::vector<std::vector<uint32_t>>> merged_of;  // [blocks] merged genome sets (ids that hit more than once)
            for (uint64_t k = 0;; ++k) {
                Slot &s = slots[k % NB];
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return (s.ready == 2 && s.seq == k) || past_end(k); });
                    if (past_end(k)) return;
                }
                const Batch &b = s.b;
                const uint64_t n = b.n();
                const uint64_t *h_off = s.hits.off.data();
                const uint32_t *h_leaves = s.hits.leaves.data();
                {   // the buffer set of this batch must have been written
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return jobs[k & 1].state == 0; });
                }
                std::vector<OutBuf> &pos_buf = pos_sets[k & 1], &neg_buf = neg_sets[k & 1];
                const uint64_t t0 = ReadQueue::now_ns();
                const uint64_t n_blocks = n ? (n + o.block - 1) / o.block : 0;
                // ---- phase 1: the blocks' maps
                grp0.assign(n_blocks + 1, 0);
                tab0.assign(n_blocks + 1, 0);
                for (uint64_t blk = 0; blk < n_blocks; ++blk) {
                    const uint64_t b0 = blk * o.block, b1 = std::min(n, b0 + o.block);
                    uint64_t n_hit = 0;
                    for (uint64_t r = b0; r < b1; ++r) n_hit += h_off[r] != h_off[r + 1];
                    grp0[blk + 1] = grp0[blk] + n_hit;
                    tab0[blk + 1] = tab0[blk] + block_table_slots(n_hit);
                }
                if (groups.size() < grp0[n_blocks]) groups.resize(grp0[n_blocks]);
                table.assign(tab0[n_blocks], 0);
                if (grp_of.size() < n) grp_of.resize(n);
                merged_of.resize(std::max<size_t>(merged_of.size(), n_blocks));
                const unsigned nw1 = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(fmt_workers, n_blocks));
                fan_out(nw1, [&](size_t w) {
                    for (uint64_t blk = n_blocks * w / nw1; blk < n_blocks * (w + 1) / nw1; ++blk) {
                        const uint64_t b0 = blk * o.block, b1 = std::min(n, b0 + o.block);
                        map_block(b, b0, b1, h_off, h_leaves, groups.data() + grp0[blk], table.data() + tab0[blk], (size_t)(tab0[blk + 1] - tab0[blk]),
                                  merged_of[blk], grp_of.data());
                    }
                });
                // ---- phase 2: the records
                const unsigned nw = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(fmt_workers, (n + 4095) / 4096));
                fan_out(nw, [&](size_t w) {
                    OutBuf &pb = pos_buf[w], &nb = neg_buf[w];
                    pb.n = nb.n = 0;
                    for (uint64_t r = n * w / nw; r < n * (w + 1) / nw; ++r) {
                        const uint64_t blk = r / o.block;
                        put_block_record(pb, nb, b, r, grp_of[r], groups.data() + grp0[blk], merged_of[blk], h_off, h_leaves, o.pos, o.neg, db.leaf_names);
                    }
                    if (o.gzip_output)  // the worker deflates its own part; the parts' places then follow from the compressed sizes
                        for (OutBuf *part : {&pb, &nb}) {
                            std::vector<unsigned char> &gz = gz_parts[w];
                            gz.clear();
                            bgzf_pack(part->p, part->n, o.gzip_level, gz);
                            part->n = 0;
                            part->put((const char *)gz.data(), gz.size());
                        }
                });
                for (unsigned w = nw; w < fmt_workers; ++w) pos_buf[w].n = neg_buf[w].n = 0;
                if (o.scores) {
                    // READ_SCORES.tsv: per record with hits, its genomes by matched k-mers
                    std::vector<std::string> parts(nw);
                    const uint32_t *h_sc = s.hits.scores.data();
                    fan_out(nw, [&](size_t w) {
                        std::vector<uint64_t> order;
                        for (uint64_t r = n * w / nw; r < n * (w + 1) / nw; ++r)
                            if (h_off[r] != h_off[r + 1])
                                put_scores(parts[w], b.id(r), n_kmers(b.off[r + 1] - b.off[r], kmer_size), h_leaves + h_off[r], h_sc + h_off[r],
                                           h_off[r + 1] - h_off[r], db.leaf_names, order);
                    });
                    for (const std::string &p : parts)
                        if (!p.empty() && fwrite(p.data(), 1, p.size(), out.scores) != p.size()) fail_from_thread("short write to READ_SCORES.tsv");
                }
                if (o.lca_reads) {
                    // READ_LCA.tsv: per record with hits, the size of its hit set and its clade
                    std::vector<std::string> parts(nw);
                    const uint32_t *h_lca = s.hits.lca.data();
                    fan_out(nw, [&](size_t w) {
                        for (uint64_t r = n * w / nw; r < n * (w + 1) / nw; ++r)
                            if (h_off[r] != h_off[r + 1]) put_lca(parts[w], b.id(r), h_off[r + 1] - h_off[r], h_lca[r], db.clade_names);
                    });
                    for (const std::string &p : parts)
                        if (!p.empty() && fwrite(p.data(), 1, p.size(), out.lca) != p.size()) fail_from_thread("short write to READ_LCA.tsv");
                }
                if (o.taxon_reads) {
                    // READ_TAXA.tsv: per record with hits, the size of its hit set and its node of the taxonomy
                    std::vector<std::string> parts(nw);
                    const uint32_t *h_taxa = s.hits.taxa.data();
                    fan_out(nw, [&](size_t w) {
                        for (uint64_t r = n * w / nw; r < n * (w + 1) / nw; ++r)
                            if (h_off[r] != h_off[r + 1]) put_lca(parts[w], b.id(r), h_off[r + 1] - h_off[r], h_taxa[r], db.taxon_names);
                    });
                    for (const std::string &p : parts)
                        if (!p.empty() && fwrite(p.data(), 1, p.size(), out.taxa) != p.size()) fail_from_thread("short write to READ_TAXA.tsv");
                }
                const uint64_t t1 = ReadQueue::now_ns();
                ns_fmt += t1 - t0;
                // the bytes: batches come in input order, so a part's place is the sum of what lies before it
                std::vector<uint64_t> pos_at(nw + 1, out.pos.size), neg_at(nw + 1, out.neg.size);
                for (unsigned x = 0; x < nw; ++x) {
                    pos_at[x + 1] = pos_at[x] + pos_buf[x].n;
                    neg_at[x + 1] = neg_at[x] + neg_buf[x].n;
                }
                out.pos.size = pos_at[nw];
                out.neg.size = neg_at[nw];
                ns_out += ReadQueue::now_ns() - t0;
                {   // the batch is free again (everything it holds is in the buffers); the writer takes over
                    std::lock_guard<std::mutex> lk(mu);
                    s.ready = 0;
                    jobs[k & 1].nw = nw;
                    jobs[k & 1].pos_at = pos_at;
                    jobs[k & 1].neg_at = neg_at;
                    jobs[k & 1].state = 1;
                }
                cv.notify_all();
            }
        });
        fan_out(n_trees(), classify_loop);
        parser.join();
        output.join();
        {
            std::lock_guard<std::mutex> lk(mu);
            writer_done = true;
        }
        cv.notify_all();
        writer.join();
        for (Slot &s : slots) rq.release_held(s.b);
        if (getenv("PFQ_INGEST_TIMING"))
            fprintf(stderr, "output: format %.3f s, write %.3f s (%u workers; wall times of the formatter and the writer thread, which overlap)\n",
                    ns_fmt.load() * 1e-9, ns_write.load() * 1e-9, fmt_workers);
    }
};

// --- the options of `query`: values ---
[[noreturn]] void invalid(const std::string &name, const std::string &value, const std::string &what) {
    die("error: invalid value '" + value + "' for '--" + name + "': " + what);
}
// The strict rule for a number: it starts with a digit, nothing follows the digits, it fits and lies in [lo, hi].  (to_u64 is the
// lenient one, with the shorter message: it takes "+5" and " 5".)
bool strict_uint(const std::string &text, uint64_t lo, uint64_t hi, uint64_t &x) {
    char *end = nullptr;
    errno = 0;
    x = strtoull(text.c_str(), &end, 10);
    return !text.empty() && isdigit((unsigned char)text[0]) && !*end && !errno && x >= lo && x <= hi;
}
uint64_t parse_uint(const char *name, const std::string &text, uint64_t lo, uint64_t hi, const char *what) {
    uint64_t x = 0;
    if (!strict_uint(text, lo, hi, x)) invalid(name, text, what);
    return x;
}
std::vector<std::string> split_list(const std::string &text) {  // at every ',': empty items are kept, "" is one empty item
    std::vector<std::string> items;
    for (size_t at = 0, end = 0; end != std::string::npos; at = end + 1) {
        end = text.find(',', at);
        items.push_back(text.substr(at, end == std::string::npos ? end : end - at));
    }
    return items;
}

// --- the options of `query`: which go together ---
// REFUSALS, read from top to bottom, is THE order in which a command line is refused: parse_query_options() walks it stage by
// stage, each named in the call, and does between two stages the checks that are no pairs (values, lists, files), which the
// comment at that place names.  A row says: WITH: `option` cannot be used with any of `others` (the first one given is named);
// NEEDS: `option` needs one of `others`, and `reason` is what the message says it needs; ARGUMENT: as WITH, in the words of the
// reference's parser.  An entry is an option's name, or "name value" (given with just that value), or "any-prep": the first of
// PREP_OPTIONS given, but --deplete before all of them.  Where a row sits decides which option a refusal names when several rows
// apply, so a new option's rows go where its priority demands, not at the end.
enum class Stage { FIRST, LCA, COVERAGE, DEVICE_OUTPUT, FRAME_STEP, MODES, ADAPTERS, MATES, TAXONOMY, PAIRS, PAIR_MODE, GZIP };
struct Refusal {
    Stage stage;
    enum Rule { WITH, NEEDS, ARGUMENT } rule;
    const char *option, *others, *reason;
};
const char *const PREP_OPTIONS[] = {"trim-quality", "trim-window", "trim-poly-x", "min-length", "max-n", "min-complexity", "adapter", "adapter2",
                                    "adapter-overlap", "adapter-errors", "mate-overlap", "mate-overlap-errors"};
const char ONLY_COUNTS[] = ": it serves runs that only count", FRAMES[] = ": frames do not combine with per-read post-stages",
           FRAGMENTS[] = ": a fragment's score is its mates' sum, so its hits at other thresholds do not follow from it",
           BEST_SCORES[] = ": the best hits need every read's scores",
           DEVICE_OUTPUT[] = ": it formats the POS / NEG records of single reads, and nothing else, on the device";
const Refusal REFUSALS[] = {
    // --best-hits first, so that a refusal names it whichever of --taxonomy, --abundance, --coverage it came with
    {Stage::FIRST, Refusal::NEEDS, "best-hits", "taxonomy,abundance,coverage", "at least one of '--taxonomy <FILE>', '--abundance', '--coverage': they are what it changes"},
    {Stage::FIRST, Refusal::WITH, "best-hits", "shard-depth", ": a subtree shard sees only its own genomes, and the best of a partial hit row is not the row's best"},
    {Stage::FIRST, Refusal::WITH, "device-parse", "best-hits", ONLY_COUNTS},
    {Stage::FIRST, Refusal::WITH, "best-hits", "frame", FRAMES},
    {Stage::FIRST, Refusal::WITH, "sweep", "reads2", FRAGMENTS},
    {Stage::FIRST, Refusal::WITH, "sweep", "shard-depth", ": a subtree shard sees only its own genomes, so the reads it would count are partial"},
    {Stage::FIRST, Refusal::WITH, "sweep", "frame", FRAMES},
    {Stage::FIRST, Refusal::WITH, "sweep", "interleaved", FRAGMENTS},
    {Stage::FIRST, Refusal::WITH, "device-parse", "sweep", ONLY_COUNTS},
    // then: the list of --sweep, each value against -f; the value of --lca
    {Stage::LCA, Refusal::NEEDS, "lca-reads", "lca", "'--lca <all|best>'"},
    {Stage::LCA, Refusal::WITH, "lca", "shard-depth", ": a subtree shard holds only its own part of the tree, and combining the shards' lowest common ancestors needs the whole tree's clades (not implemented)"},
    {Stage::LCA, Refusal::NEEDS, "abundance-iters", "abundance", "'--abundance'"},
    // then: the value of --abundance-iters
    {Stage::COVERAGE, Refusal::WITH, "abundance", "shard-depth", ": a subtree shard sees only its own genomes, so the hit rows it would log are partial (not implemented)"},
    {Stage::COVERAGE, Refusal::NEEDS, "coverage-precision", "coverage", "'--coverage'"},
    // then: the value of --coverage-precision
    // --device-output refuses everything --device-parse refuses but the two filters, before the other options' own checks, so that the
    // refusal names it; --deplete before the other options that turn preprocessing on
    {Stage::DEVICE_OUTPUT, Refusal::WITH, "device-output", "device-parse", ": that option serves runs that only count, this one parses the text itself"},
    {Stage::DEVICE_OUTPUT, Refusal::WITH, "device-output", "scores,lca-reads,interleaved,abundance,coverage,taxon-reads,best-hits,mate-correct,deplete,deplete-threshold", DEVICE_OUTPUT},
    {Stage::DEVICE_OUTPUT, Refusal::WITH, "device-output", "reads2,frame,shard-depth,taxonomy,sweep,trim-quality,trim-window,trim-poly-x,min-length,max-n,min-complexity,adapter,adapter2",
     DEVICE_OUTPUT},
    {Stage::DEVICE_OUTPUT, Refusal::WITH, "device-output", "adapter-overlap,adapter-errors,mate-overlap,mate-overlap-errors,mate-correct-quality", DEVICE_OUTPUT},
    {Stage::DEVICE_OUTPUT, Refusal::WITH, "device-output", "lca best", BEST_SCORES},
    {Stage::DEVICE_OUTPUT, Refusal::NEEDS, "device-output", "pos-filter,neg-filter", "'--pos-filter' or '--neg-filter' (or both): they are the outputs it makes"},
    // then: --device-output against the value of --block-size-reads
    {Stage::FRAME_STEP, Refusal::NEEDS, "frame-step", "frame", "'--frame <F>'"},
    // then: the values of --frame and --frame-step, the step against the frame
    {Stage::MODES, Refusal::WITH, "frame", "reads2,shard-depth,interleaved,scores,abundance,coverage,pos-filter,neg-filter,lca", ""},
    {Stage::MODES, Refusal::NEEDS, "device-inflate", "device-parse", "'--device-parse': the text it inflates on the device is parsed there"},
    {Stage::MODES, Refusal::WITH, "device-parse", "pos-filter,neg-filter,scores,lca-reads,interleaved,abundance,coverage,reads2,frame,shard-depth", ONLY_COUNTS},
    {Stage::MODES, Refusal::WITH, "device-parse", "lca best", BEST_SCORES},
    // --mate-correct is part of the mate overlap step, so it needs --mate-overlap and is refused wherever that is
    {Stage::MODES, Refusal::NEEDS, "mate-correct-quality", "mate-correct", "'--mate-correct'"},
    {Stage::MODES, Refusal::NEEDS, "mate-correct", "mate-overlap", "'--mate-overlap <O>': it corrects the bases on which the overlapping mates of a fragment disagree"},
    {Stage::MODES, Refusal::NEEDS, "deplete-threshold", "deplete", "'--deplete <DIR>'"},
    {Stage::MODES, Refusal::WITH, "any-prep", "device-parse,frame,shard-depth", ": preprocessing works on the batches the host reader parses and classifies every kept read on every replica"},
    // then: the values of the trimming options
    {Stage::ADAPTERS, Refusal::NEEDS, "adapter-overlap", "adapter", "'--adapter <SEQ>'"},
    {Stage::ADAPTERS, Refusal::NEEDS, "adapter-errors", "adapter", "'--adapter <SEQ>'"},
    {Stage::ADAPTERS, Refusal::NEEDS, "adapter2", "adapter", "'--adapter <SEQ>'"},
    {Stage::ADAPTERS, Refusal::NEEDS, "adapter2", "reads2,interleaved", "'--reads2 <FILE>' or '--interleaved': it serves the second mates"},
    // then: the values of --adapter-overlap and --adapter-errors, the adapters, each one's length against --adapter-overlap
    {Stage::MATES, Refusal::NEEDS, "mate-overlap-errors", "mate-overlap", "'--mate-overlap <O>'"},
    {Stage::MATES, Refusal::NEEDS, "mate-overlap", "reads2,interleaved", "'--reads2 <FILE>' or '--interleaved': it compares the two mates of a fragment"},
    // then: the values of the mate options; the screens of --deplete, each one's tree.bin
    {Stage::TAXONOMY, Refusal::NEEDS, "taxon-reads", "taxonomy", "'--taxonomy <FILE>'"},
    {Stage::TAXONOMY, Refusal::WITH, "taxonomy", "shard-depth", ": a subtree shard sees only its own genomes, so the hit rows it would count are partial (not implemented)"},
    {Stage::TAXONOMY, Refusal::WITH, "taxonomy", "frame", FRAMES},
    {Stage::TAXONOMY, Refusal::WITH, "device-parse", "taxonomy", ONLY_COUNTS},
    // then: the taxonomy's file against tree.bin; the value of --format
    {Stage::PAIRS, Refusal::ARGUMENT, "reads2", "interleaved", ""},
    // then: the value of --pair-mode
    {Stage::PAIR_MODE, Refusal::NEEDS, "pair-mode", "reads2,interleaved", "'--reads2' or '--interleaved'"},
    // --gzip-output last of all: it changes how two files are written and nothing else, so every other refusal comes first
    {Stage::GZIP, Refusal::NEEDS, "gzip-output", "pos-filter,neg-filter", "'--pos-filter' or '--neg-filter' (or both): theirs are the files it compresses"},
    {Stage::GZIP, Refusal::NEEDS, "gzip-level", "gzip-output", "'--gzip-output'"}};
    // then: the value of --gzip-level
// What the command line has of a table entry (see REFUSALS), as a message names it; empty: nothing
std::string given(const Args &a, const std::string &entry) {
    if (entry == "any-prep") {
        if (a.val.count("deplete")) return "deplete";
        for (const char *name : PREP_OPTIONS)
            if (a.val.count(name)) return name;
        return "";
    }
    const size_t space = entry.find(' ');
    const auto it = a.val.find(entry.substr(0, space));
    if (space != std::string::npos) return it != a.val.end() && it->second == entry.substr(space + 1) ? entry : "";
    return it != a.val.end() || a.flags.count(entry) ? entry : "";
}
[[noreturn]] void refuse_with(const std::string &option, const std::string &other, const std::string &reason, bool argument = false) {
    std::string upper = option;
    for (char &c : upper) c = (char)toupper((unsigned char)c);
    die("error: " + (argument ? "the argument '--" + option + " <" + upper + ">'" : "'--" + option + "'") + " cannot be used with '--" + other + "'" + reason);
}
// Refuses the command line by the first row of the stage that applies
void refuse_by_table(const Args &a, Stage stage) {
    for (const Refusal &row : REFUSALS) {
        const std::string option = row.stage == stage ? given(a, row.option) : "";
        if (option.empty()) continue;
        bool any = false;
        for (const std::string &entry : split_list(row.others)) {
            const std::string other = given(a, entry);
            if (other.empty()) continue;
            if (row.rule != Refusal::NEEDS) refuse_with(option, other, row.reason, row.rule == Refusal::ARGUMENT);
            any = true;
        }
        if (row.rule == Refusal::NEEDS && !any) die("error: '--" + option + "' needs " + row.reason);
    }
}

// Reads and checks the command line of `query`.  Everything here happens before any device is used and before the output directory
// is touched; the only files looked at are the screens' tree.bin (--deplete) and the database's leaf ids and the taxonomy (--taxonomy).
QueryOptions parse_query_options(const Args &a) {
    QueryOptions o;
    const auto has = [&](const char *name) { return a.flags.count(name) != 0 || a.val.count(name) != 0; };
    const auto number = [&](const char *name, const char *dflt, uint64_t lo, uint64_t hi, const char *what) { return (uint32_t)parse_uint(name, opt(a, name, dflt), lo, hi, what); };
    o.reads = req(a, "reads"), o.out = req(a, "out"), o.db_path = req(a, "db-path");
    o.threads = (unsigned)std::min<uint64_t>(to_u64(opt(a, "threads", "4"), "threads"), 256);
    (void)to_u64(opt(a, "cache-size", "10"), "cache-size");  // LRU of .bf files: the whole tree is resident in HBM
    o.block = to_u64(opt(a, "block-size-reads", "100"), "block-size-reads");
    const std::string threshold_typed = opt(a, "filter-threshold", "1.0");
    o.threshold = to_f32(threshold_typed, "filter-threshold");
    o.pos = has("pos-filter"), o.neg = has("neg-filter"), o.scores = has("scores"), o.best_hits = has("best-hits");
    refuse_by_table(a, Stage::FIRST);
    // --sweep T1,T2,..: one pass at -f also counts, per listed threshold, what a run of its own at that threshold would report
    // (PFQ_WANT_HITS | PFQ_WANT_SCORES | PFQ_WANT_SWEEP).  The values are parsed as -f is and kept as typed for the files.
    if ((o.sweep = has("sweep"))) {
        const std::string &spec = a.val.at("sweep");
        for (const std::string &item : split_list(spec)) {
            if (item.empty()) invalid("sweep", spec, "an empty item in the list of thresholds");
            const float v = to_f32(item, "sweep");
            if (v != v) invalid("sweep", item, "not a number");
            if (!o.sweep_thr.empty() && !(o.sweep_thr.back() < v))
                invalid("sweep", spec, "the thresholds must be strictly ascending ('" + o.sweep_typed.back() + "' before '" + item + "')");
            if (!(o.threshold <= v))
                die("error: '--sweep " + item + "' is below '--filter-threshold " + threshold_typed +
                    "' (-f): the one pass runs at -f and cannot answer a lower threshold; lower -f to the list's lowest value");
            o.sweep_thr.push_back(v), o.sweep_typed.push_back(item);
        }
        if (o.sweep_thr.size() > PFQ_SWEEP_MAX)
            invalid("sweep", spec, std::to_string(o.sweep_thr.size()) + " thresholds, at most " + std::to_string(PFQ_SWEEP_MAX));
    }
    // --lca all|best: every read (fragment) is also assigned to the lowest common ancestor of its hit genomes (best: of its best-scoring ones)
    const std::string lca = opt(a, "lca", "");
    if (has("lca") && lca != "all" && lca != "best") die("error: invalid value '" + lca + "' for '--lca' [possible values: all, best]");
    o.lca = lca == "all" ? 1 : lca == "best" ? 2 : 0, o.lca_reads = has("lca-reads");
    refuse_by_table(a, Stage::LCA);
    // --abundance: every call also logs its units' hit rows on the device; at the end an EM over the log estimates every genome's units
    o.abundance = has("abundance"), o.abundance_iters = to_u64(opt(a, "abundance-iters", "200"), "abundance-iters");
    if (o.abundance && (o.abundance_iters == 0 || o.abundance_iters > 0xffffffffull)) invalid("abundance-iters", opt(a, "abundance-iters", ""), "at least 1 iteration");
    refuse_by_table(a, Stage::COVERAGE);
    // --coverage: every call also sketches, per genome a read lists, the read's k-mers that genome's filter contains
    o.coverage = has("coverage"), o.coverage_precision = opt(a, "coverage-precision", "12");
    if (o.coverage) parse_uint("coverage-precision", o.coverage_precision, 4, 16, "4 to 16 (2^P registers per genome)");
    refuse_by_table(a, Stage::DEVICE_OUTPUT);
    // --device-output: the POS / NEG records of plain FASTA / FASTQ files are parsed, classified and formatted on the device
    if ((o.device_output = has("device-output"))) {
        if (o.block == 0) refuse_with("device-output", "block-size-reads 0", ": no read would be classified");
        if (o.block > PFQ_FMT_BLOCK_MAX)
            refuse_with("device-output", "block-size-reads " + std::to_string(o.block), ": the device decides POS / NEG per block of at most " + std::to_string(PFQ_FMT_BLOCK_MAX) + " reads");
    }
    refuse_by_table(a, Stage::FRAME_STEP);
    // --frame F [--frame-step S]: every sequence (a contig, a long read) is classified in overlapping frames of F bases every S
    // bases (pfq_query_frames) and SEGMENTS.tsv says where on it every genome matched; CLASSIFICATION.csv then counts sequences
    if (has("frame")) {
        o.frame = number("frame", "", 1, 0xffffffffull, "a positive number of bases");
        o.frame_step = has("frame-step") ? number("frame-step", "", 1, 0xffffffffull, "a positive number of bases") : std::max<uint32_t>(o.frame / 2, 1);
        if (o.frame_step > o.frame)
            die("error: '--frame-step " + std::to_string(o.frame_step) + "' is larger than '--frame " + std::to_string(o.frame) + "': frames would leave gaps");
    }
    // --device-parse: plain FASTA / FASTQ files are parsed on the device (pfq_text_parse); only where the run counts per genome
    // (and per clade) on replicas — per-read outputs, pairs, frames and shards keep the host reader
    // --device-inflate: blocked gzip (BGZF) files are inflated on the device as well (pfq_text_inflate); it rides on --device-parse
    o.device_parse = has("device-parse"), o.device_inflate = has("device-inflate");
    refuse_by_table(a, Stage::MODES);
    // --trim-quality Q, --trim-window W, --trim-poly-x P, --min-length L, --max-n N, --min-complexity C, the adapter and mate options
    // and --deplete: any of them turns read preprocessing on: every call trims and filters its reads on the device (pfq_prep_reads)
    // and classifies what is kept (pfq_prep_query).  --min-length then defaults to the database's k.
    if ((o.prep = !given(a, "any-prep").empty())) {
        o.params.trim_quality = number("trim-quality", "0", 0, 93, "a Phred quality from 0 (off) to 93");
        o.params.trim_window = number("trim-window", "4", 1, 1024, "a window of 1 to 1024 bases");
        o.params.poly_x = number("trim-poly-x", "0", 0, 0xffffffffull, "a number of bases (0: off)");
        o.params.min_length = has("min-length") ? number("min-length", "1", 1, 0xffffffffull, "at least 1 base (the default is the database's k)") : 0;
        o.params.max_n = has("max-n") ? number("max-n", "0", 0, 0xfffffffeull, "a number of N bases") : 0xffffffffu;
        o.params.min_complexity = number("min-complexity", "0", 0, 100, "a percentage from 0 (off) to 100");
    }
    refuse_by_table(a, Stage::ADAPTERS);
    // --adapter SEQ[,SEQ..] (reads and first mates), --adapter2 SEQ[,..] (second mates; without it they use --adapter's),
    // --adapter-overlap O, --adapter-errors E: every read is cut at the leftmost place an adapter matches (pfq.h "adapters")
    // before the steps above.  A SEQ is a sequence over ACGT or the name of a preset.
    if (has("adapter")) {
        o.adapter_overlap = number("adapter-overlap", "5", 1, PFQ_ADAPTER_LEN_MAX, "an overlap of 1 to 64 bases");
        o.adapter_errors = number("adapter-errors", "10", 0, 50, "a percentage of mismatches from 0 to 50");
        static const std::pair<const char *, const char *> presets[] = {
            {"illumina", "AGATCGGAAGAGC"}, {"nextera", "CTGTCTCTTATACACATCT"}, {"smallrna", "TGGAATTCTCGGGTGCCAAGG"}};
        for (int set = 0; set < 2; ++set) {
            const char *name = set ? "adapter2" : "adapter";
            if (!has(name)) continue;
            for (const std::string &item : split_list(a.val.at(name))) {  // (the parser joins a repeated option's values with ',')
                std::string seq = item;
                for (const auto &p : presets)
                    if (seq == p.first) seq = p.second;
                for (char &ch : seq) {
                    ch = (char)(ch & 0xDF);
                    if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') invalid(name, item, "a sequence over ACGT or one of illumina, nextera, smallrna");
                }
                if (seq.size() < o.adapter_overlap || seq.size() > PFQ_ADAPTER_LEN_MAX)
                    invalid(name, item, "an adapter has from --adapter-overlap (" + std::to_string(o.adapter_overlap) + ") to " + std::to_string(PFQ_ADAPTER_LEN_MAX) + " bases");
                if (o.adapters[set].size() == PFQ_ADAPTER_MAX) invalid(name, item, "at most " + std::to_string(PFQ_ADAPTER_MAX) + " adapters per option");
                o.adapters[set].push_back(seq);
            }
        }
    }
    refuse_by_table(a, Stage::MATES);
    // --mate-overlap O [--mate-overlap-errors E]: both mates of a fragment are cut at the insert length that the overlap of
    // the mates gives (pfq.h "mate overlap"), whatever the adapter's sequence; INSERT_SIZES.tsv counts the fragments per length
    if (has("mate-overlap")) {
        o.mate_overlap = number("mate-overlap", "30", 1, PFQ_OVERLAP_LEN_MAX, "an overlap of 1 to 512 bases");
        o.mate_overlap_errors = number("mate-overlap-errors", "10", 0, 50, "a percentage of mismatches from 0 to 50");
    }
    // --mate-correct [--mate-correct-quality HI[,LO]]: where the mates disagree inside their overlap, a base of quality LO or less
    // takes what the mate says if that one's quality is HI or more (pfq.h "mate correction"), before the steps above
    if (has("mate-correct")) {
        const std::string v = opt(a, "mate-correct-quality", "30,14");
        const size_t comma = v.find(',');
        uint64_t high = 0, low = 14;
        if (!strict_uint(v.substr(0, comma), 0, 93, high) || (comma != std::string::npos && !strict_uint(v.substr(comma + 1), 0, 93, low)) || high < 1 || low >= high)
            invalid("mate-correct-quality", v, "HI[,LO], Phred qualities with 1 <= HI <= 93 and LO < HI (default 30,14)");
        o.mate_correct_high = (uint32_t)high, o.mate_correct_low = (uint32_t)low;
    }
    // --deplete DIR [--deplete DIR2 ..] [--deplete-threshold T]: after the steps above every unit that hits one of the screens, a
    // database each, at T (default: -f) is taken out before the classification (pfq.h "depletion")
    if (has("deplete")) {
        o.deplete_dirs = split_list(a.val.at("deplete"));  // (the parser joins a repeated option's values with ',')
        if (o.deplete_dirs.size() > PrepRun::DEPLETE_MAX)
            die("error: '--deplete' given " + std::to_string(o.deplete_dirs.size()) + " times, at most " + std::to_string(PrepRun::DEPLETE_MAX) +
                " screens (a directory name must not hold a ',')");
        o.deplete_threshold_typed = opt(a, "deplete-threshold", threshold_typed);
        o.deplete_threshold = has("deplete-threshold") ? to_f32(a.val.at("deplete-threshold"), "deplete-threshold") : o.threshold;
        for (const std::string &dir : o.deplete_dirs) {
            FILE *f = fopen((dir + "/tree.bin").c_str(), "rb");
            if (!f) invalid("deplete", dir, "cannot read " + dir + "/tree.bin: " + strerror(errno));
            fclose(f);
        }
    }
    // --taxonomy FILE: every read (fragment) is also counted on the nodes of the user's taxonomy over the database's genomes
    // (PFQ_WANT_HITS | PFQ_WANT_TAXA).  The file is parsed and checked against tree.bin here.
    o.taxonomy = has("taxonomy"), o.taxon_reads = has("taxon-reads");
    refuse_by_table(a, Stage::TAXONOMY);
    if (o.taxonomy) {
        o.taxonomy_file = a.val.at("taxonomy");
        const char *const *ids = nullptr;
        uint64_t n_ids = 0;
        check(pfq_db_leaf_ids(o.db_path.c_str(), &ids, &n_ids));
        pfq_taxonomy_file tf{};
        check(pfq_taxonomy_read(o.taxonomy_file.c_str(), ids, n_ids, &tf));
    }
    o.format = to_fmt(opt(a, "format", "auto"));
    // paired-end reads: --reads2 (mates by record index across the two streams) or --interleaved (adjacent records); every
    // fragment is classified with PFQ_PAIRED, its set the union (--pair-mode either) or intersection (both) of its mates'
    o.interleaved = has("interleaved"), o.has_reads2 = has("reads2"), o.reads2 = opt(a, "reads2", "");
    refuse_by_table(a, Stage::PAIRS);
    const std::string pair_mode = opt(a, "pair-mode", "either");
    if (pair_mode != "either" && pair_mode != "both") die("error: invalid value '" + pair_mode + "' for '--pair-mode' [possible values: either, both]");
    o.pair_both = pair_mode == "both";
    refuse_by_table(a, Stage::PAIR_MODE);
    // --gzip-output [--gzip-level L]: POS / NEG as blocked gzip; L is zlib's level for the members the host makes
    refuse_by_table(a, Stage::GZIP);
    o.gzip_output = has("gzip-output");
    if (has("gzip-level")) o.gzip_level = (int)number("gzip-level", "6", 1, 9, "a zlib level from 1 to 9");
    // --devices 0,1,..|all (or PFQ_DEVICES): one replica of the database per listed GPU, each fed by its own host thread;
    // the per-genome counts are combined by one RCCL all-reduce at the end.  The reference has one rayon pool instead
    // (main.rs:269-272); results do not depend on how the reads are dealt.
    const std::string devices = opt(a, "devices", getenv("PFQ_DEVICES") ? getenv("PFQ_DEVICES") : "");
    if (devices == "all") {
        int n = 0;
        check(pfq_device_count(&n));
        for (int i = 0; i < n; ++i) o.devices.push_back(i);
    } else if (!devices.empty()) {
        for (const std::string &item : split_list(devices)) o.devices.push_back((int)to_u64(item, "devices"));
    }
    if (o.devices.empty()) o.devices.push_back(device_from_env());
    // --shard-depth D: the database is split into the subtree shards of its depth-E frontier (pfq_tree_open_subtree), E = D,
    // or the search depth when that is smaller (a shard cut below the pruning depth would put one pruned leaf into several
    // shards).  Shard i classifies EVERY read, on its own host thread; the shards' hits and counts are concatenated in
    // shard order.
    o.pruned = has("search-depth"), o.search_depth = opt(a, "search-depth", "");
    if ((o.sharded = has("shard-depth"))) {
        o.shard_depth = to_u64(a.val.at("shard-depth"), "shard-depth");
        if (o.pruned) o.shard_depth = std::min(o.shard_depth, to_u64(o.search_depth, "search-depth"));
    }
    return o;
}

// What preprocessing did and with which parameters: PREPROCESS.tsv, DEPLETION*.csv, INSERT_SIZES.tsv and one line on stderr
void write_prep_report(const QueryOptions &o, const PrepRun &pr, const std::vector<std::unique_ptr<ServedDb>> &screens) {
    const auto n = [](const std::atomic<uint64_t> &x) { return (unsigned long long)x.load(); };
    // PREPROCESS.tsv: the totals over all calls and replicas, then the parameters in force
    const std::string max_n = o.params.max_n == 0xffffffffu ? "off" : std::to_string(o.params.max_n);
    const std::pair<const char *, std::string> rows[] = {
        {"reads", std::to_string(n(pr.reads))}, {"reads_kept", std::to_string(n(pr.kept))}, {"reads_trimmed", std::to_string(n(pr.trimmed))},
        {"dropped_short", std::to_string(n(pr.reason[PFQ_PREP_SHORT]))}, {"dropped_n", std::to_string(n(pr.reason[PFQ_PREP_N]))},
        {"dropped_complexity", std::to_string(n(pr.reason[PFQ_PREP_COMPLEXITY]))}, {"dropped_mate", std::to_string(n(pr.reason[PFQ_PREP_MATE]))},
        {"bases", std::to_string(n(pr.bases))}, {"bases_kept", std::to_string(n(pr.bases_kept))},
        {"trim_quality", std::to_string(o.params.trim_quality)}, {"trim_window", std::to_string(o.params.trim_window)},
        {"trim_poly_x", std::to_string(o.params.poly_x)}, {"min_length", std::to_string(o.params.min_length)}, {"max_n", max_n},
        {"min_complexity", std::to_string(o.params.min_complexity)}};
    FILE *f = fopen((o.out + "/PREPROCESS.tsv").c_str(), "wb");
    if (!f) die("cannot create PREPROCESS.tsv in " + o.out);
    for (const auto &row : rows) fprintf(f, "%s\t%s\n", row.first, row.second.c_str());
    if (o.adapters_on()) {  // behind the rows above: what the adapter step found, its parameters, the reads per adapter
        fprintf(f, "adapter_reads\t%llu\nadapter_bases\t%llu\nadapter_overlap\t%u\nadapter_errors\t%u\n", n(pr.adapter_reads), n(pr.adapter_bases), o.adapter_overlap,
                o.adapter_errors);
        for (int set = 0; set < 2; ++set)
            for (size_t i = 0; i < o.adapters[set].size(); ++i)
                fprintf(f, "adapter%d.%s\t%llu\n", set + 1, o.adapters[set][i].c_str(), n(pr.adapter_found[set * PFQ_ADAPTER_MAX + i]));
    }
    if (o.mate_overlap) {  // behind the adapter rows: what the overlap step found and its parameters
        fprintf(f, "overlap_fragments\t%llu\noverlap_skipped\t%llu\noverlap_found\t%llu\noverlap_readthrough\t%llu\noverlap_reads\t%llu\noverlap_bases\t%llu\n",
                n(pr.overlap_fragments), n(pr.overlap_skipped), n(pr.overlap_found), n(pr.overlap_readthrough), n(pr.overlap_reads), n(pr.overlap_bases));
        fprintf(f, "mate_overlap\t%u\nmate_overlap_errors\t%u\n", o.mate_overlap, o.mate_overlap_errors);
    }
    if (o.mate_correct_high)  // behind the overlap rows: what the correction did and its parameters
        fprintf(f, "corrected_fragments\t%llu\ncorrected_bases\t%llu\ncorrect_unresolved\t%llu\ncorrect_no_quality\t%llu\nmate_correct_quality\t%u\nmate_correct_low\t%u\n",
                n(pr.corrected_fragments), n(pr.corrected_bases), n(pr.correct_unresolved), n(pr.correct_no_quality), o.mate_correct_high, o.mate_correct_low);
    for (size_t i = 0; i < o.deplete_dirs.size(); ++i)  // behind the overlap rows: per screen, in the order given
        fprintf(f, "deplete_db\t%s\ndeplete_threshold\t%s\ndepleted_units\t%llu\ndepleted_reads\t%llu\ndepleted_bases\t%llu\n", o.deplete_dirs[i].c_str(),
                o.deplete_threshold_typed.c_str(), n(pr.depleted_units[i]), n(pr.depleted_reads[i]), n(pr.depleted_bases[i]));
    if (fclose(f) != 0) die("short write to PREPROCESS.tsv");
    // DEPLETION.csv (several screens: DEPLETION_1.csv ..): what CLASSIFICATION.csv of a run of the block screen i saw against
    // that screen would hold; the replicas' counters are summed as the main database's are
    for (size_t i = 0; i < screens.size(); ++i)
        screens[i]->save_counts(o.out + (screens.size() == 1 ? std::string("/DEPLETION.csv") : "/DEPLETION_" + std::to_string(i + 1) + ".csv"));
    if (o.mate_overlap) {
        // INSERT_SIZES.tsv: the fragments per insert length, summed over all calls and replicas
        FILE *g = fopen((o.out + "/INSERT_SIZES.tsv").c_str(), "wb");
        if (!g) die("cannot create INSERT_SIZES.tsv in " + o.out);
        fprintf(g, "insert\tfragments\n");
        for (int i = 0; i <= PFQ_OVERLAP_INSERT_MAX; ++i)
            if (n(pr.insert_hist[i])) fprintf(g, "%d\t%llu\n", i, n(pr.insert_hist[i]));
        if (fclose(g) != 0) die("short write to INSERT_SIZES.tsv");
    }
    fprintf(stderr, "preprocessing: %llu reads, %llu kept (%llu trimmed), dropped: %llu short, %llu N, %llu low complexity, %llu mate; %llu of %llu bases kept",
            n(pr.reads), n(pr.kept), n(pr.trimmed), n(pr.reason[PFQ_PREP_SHORT]), n(pr.reason[PFQ_PREP_N]), n(pr.reason[PFQ_PREP_COMPLEXITY]),
            n(pr.reason[PFQ_PREP_MATE]), n(pr.bases_kept), n(pr.bases));
    if (o.adapters_on()) fprintf(stderr, "; adapters cut from %llu reads (%llu bases)", n(pr.adapter_reads), n(pr.adapter_bases));
    if (o.mate_overlap)
        fprintf(stderr, "; mates overlap in %llu of %llu fragments, %llu with read-through: %llu reads cut (%llu bases)", n(pr.overlap_found), n(pr.overlap_fragments),
                n(pr.overlap_readthrough), n(pr.overlap_reads), n(pr.overlap_bases));
    if (o.mate_correct_high)
        fprintf(stderr, "; %llu bases corrected in %llu fragments (%llu mismatches unresolved, %llu fragments without qualities)", n(pr.corrected_bases),
                n(pr.corrected_fragments), n(pr.correct_unresolved), n(pr.correct_no_quality));
    for (size_t i = 0; i < o.deplete_dirs.size(); ++i)
        fprintf(stderr, "; screen %s took %llu reads (%llu bases)", o.deplete_dirs[i].c_str(), n(pr.depleted_reads[i]), n(pr.depleted_bases[i]));
    fprintf(stderr, "\n");
}

int cmd_query(int argc, char **argv) {
    std::vector<Opt> opts = {{"reads", 'r', true}, {"out", 'o', true}, {"db-path", 'd', true}, {"threads", 't', true}, {"block-size-reads", 'b', true},
                             {"filter-threshold", 'f', true}, {"cache-size", 'c', true}, {"search-depth", 0, true}, {"pos-filter", 0, false}, {"neg-filter", 0, false},
                             {"format", 'F', true}, {"devices", 0, true}, {"shard-depth", 0, true}, {"scores", 0, false}, {"reads2", 0, true}, {"interleaved", 0, false},
                             {"pair-mode", 0, true}, {"lca", 0, true}, {"lca-reads", 0, false}, {"abundance", 0, false}, {"abundance-iters", 0, true},
                             {"coverage", 0, false}, {"coverage-precision", 0, true}, {"frame", 0, true}, {"frame-step", 0, true}, {"device-parse", 0, false},
                             {"device-inflate", 0, false}, {"device-output", 0, false}, {"taxonomy", 0, true}, {"taxon-reads", 0, false}, {"best-hits", 0, false},
                             {"sweep", 0, true}, {"trim-quality", 0, true}, {"trim-window", 0, true}, {"trim-poly-x", 0, true}, {"min-length", 0, true},
                             {"max-n", 0, true}, {"min-complexity", 0, true}, {"adapter", 0, true, true}, {"adapter2", 0, true, true}, {"adapter-overlap", 0, true},
                             {"adapter-errors", 0, true}, {"mate-overlap", 0, true}, {"mate-overlap-errors", 0, true}, {"deplete", 0, true, true},
                             {"deplete-threshold", 0, true}, {"mate-correct", 0, false}, {"mate-correct-quality", 0, true}, {"gzip-output", 0, false},
                             {"gzip-level", 0, true}};
    QueryOptions o = parse_query_options(parse(argc, argv, 2, opts));
    ServedDb db(o.db_path, o.devices, o.sharded, o.shard_depth);
    if (o.coverage) db.set_coverage_precision(o.coverage_precision);
    printf("Querying reads...\n");
    printf("Filtering settings: positive=%s; negative=%s\n", o.pos ? "true" : "false", o.neg ? "true" : "false");
    if (o.pruned) {
        uint64_t depth = to_u64(o.search_depth, "search-depth");
        if (!o.pos && !o.neg) printf("If using a search depth, use a filtering flag (--pos-filter or --neg-filter, or both!)\n");
        printf("Search depth settings: %llu\n", (unsigned long long)depth);
        db.prune(depth);
    }
    if (o.sweep) db.set_sweep(o.sweep_thr);  // (before any read is classified: a database that is not superset-verified is refused here)
    if (o.adapters_on()) {                   // every replica cuts the reads of its own calls
        std::vector<const char *> sets[2];
        for (int set = 0; set < 2; ++set)
            for (const std::string &s : o.adapters[set]) sets[set].push_back(s.c_str());
        for (pfq_tree *tree : db.trees)
            check(pfq_tree_set_adapters(tree, sets[0].data(), (uint32_t)sets[0].size(), sets[1].data(), (uint32_t)sets[1].size(), o.adapter_overlap, o.adapter_errors));
    }
    if (o.mate_overlap)
        for (pfq_tree *tree : db.trees) check(pfq_tree_set_mate_overlap(tree, o.mate_overlap, o.mate_overlap_errors));
    if (o.mate_correct_high)
        for (pfq_tree *tree : db.trees) check(pfq_tree_set_mate_correct(tree, o.mate_correct_high, o.mate_correct_low));
    // --deplete: every replica gets its own copy of every screen on its device (the screens' memory once per replica)
    PrepRun prep;
    std::vector<std::unique_ptr<ServedDb>> screens;
    for (const std::string &dir : o.deplete_dirs) {
        screens.emplace_back(new ServedDb(dir, o.devices, false, 0));
        for (size_t i = 0; i < db.trees.size(); ++i) prep.screens_of[db.trees[i]].push_back(screens.back()->trees[i]);
    }
    ReadQueue rq(o.reads, o.format);
    std::unique_ptr<ReadQueue> rq2;
    if (o.has_reads2) rq2.reset(new ReadQueue(o.reads2, o.format));
    // Page-locking costs ~1.7 s per GB here (hipHostMalloc), the pageable copy ~0.1 s per GB: pinned buffers only
    // pay off once every pooled buffer has been reused a few dozen times (inputs of >~ 10^9 reads).  Opt-in.
    g_pinned = getenv("PFQ_PINNED") && atoi(getenv("PFQ_PINNED")) != 0;
    rq.device_parse = o.device_parse || o.device_output;
    rq.device_inflate = o.device_inflate;
    // --block-size-reads 0: the reference's first block is empty (file_parser.rs:252-270: `0 > read_block.len()` is false),
    // so its loop (main.rs:334-368) never runs: no read is parsed or classified, the outputs are created empty
    // (paired: the mates' ids are compared; framed: SEGMENTS.tsv names the sequences; preprocessing: the qualities go to the device)
    if (o.block != 0) rq.start(o.per_read() || o.paired() || o.frame || o.prep, o.threads);
    if (o.block != 0 && rq2) rq2->start(true, o.threads);

    // create_and_overwrite_directory (main.rs:380-391): an existing output directory is deleted
    struct stat st;
    if (stat(o.out.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) rm_rf(o.out);
    mkdir(o.out.c_str(), 0777);
    Outputs outs(o, rq.peek_format() == Fmt::Fastq ? "fq" : "fa");
    uint64_t kmer_size = 0;
    if (o.scores || o.frame || o.prep) {
        pfq_info info{};
        check(pfq_tree_info(db.trees[0], &info));
        kmer_size = info.kmer_size;
    }
    if (o.prep && !o.params.min_length) o.params.min_length = (uint32_t)kmer_size;
    if (o.frame && o.frame < kmer_size)
        die("error: '--frame " + std::to_string(o.frame) + "' is shorter than the database's k-mers (k = " + std::to_string(kmer_size) + "): a frame must hold one");
    db.load_leaf_names();
    if (o.lca_reads) db.load_clade_names();
    if (o.taxonomy) db.set_taxonomy(o.taxonomy_file);

    const uint64_t t_loop0 = ReadQueue::now_ns();
    QueryLoop q{db, rq, outs, o, prep, kmer_size};
    if (o.block == 0) {
        // nothing to do: see above
    } else if (o.frame) {
        q.frames(o.frame, o.frame_step, o.out + "/SEGMENTS.tsv");
    } else if (o.paired()) {
        q.paired(rq2.get(), o.pair_both);
    } else if (o.device_parse) {
        q.counts_only_text();
    } else if (o.device_output) {
        q.device_output();
    } else if (!o.per_read()) {
        q.counts_only();
    } else {
        q.per_read();
    }
    if (getenv("PFQ_INGEST_TIMING")) {
        const double wall = (ReadQueue::now_ns() - t_loop0) * 1e-9;
        fprintf(stderr, "query loop: %llu reads in %.3f s = %.2f M reads/s on %zu device(s) (pfq_query_batch %.3f s, output %.3f s)\n",
                (unsigned long long)q.n_total.load(), wall, q.n_total.load() / wall * 1e-6, o.devices.size(), q.ns_gpu.load() * 1e-9,
                q.ns_out.load() * 1e-9);
        rq.report_timing();
        if (o.device_parse || o.device_output) q.report_device_parse();
        if (o.device_inflate) q.report_device_inflate();
        if (o.device_output) q.report_device_output();
        struct rusage ru;
        if (getrusage(RUSAGE_SELF, &ru) == 0)
            fprintf(stderr, "cpu: user %.2f s + system %.2f s so far (all threads) for %.2f s of query loop\n",
                    ru.ru_utime.tv_sec + ru.ru_utime.tv_usec * 1e-6, ru.ru_stime.tv_sec + ru.ru_stime.tv_usec * 1e-6, wall);
    }
    outs.close();
    if (!rq.pending_error.empty()) die(rq.pending_error);  // the reads before the malformed record were processed
    db.save_counts(o.out + "/CLASSIFICATION.csv");
    if (o.lca) db.save_clade_counts(o.out + "/CLADE_COUNTS.tsv");
    if (o.abundance) db.save_abundance(o.out + "/ABUNDANCE.tsv", (uint32_t)o.abundance_iters);
    if (o.coverage) db.save_coverage(o.out + "/COVERAGE.tsv");
    if (o.taxonomy) db.save_taxon_counts(o.out + "/TAXON_COUNTS.tsv", o.abundance, (uint32_t)o.abundance_iters);
    if (o.sweep) db.save_sweep(o.out, o.sweep_typed);
    if (o.prep) write_prep_report(o, prep, screens);
    db.close();
    printf("Finished.\n");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// build-balanced: synthetic balanced SBT over a genome directory (NOT the reference's greedy `build`)
// ---------------------------------------------------------------------------------------------------------------
uint64_t needed_bits(float rate, uint32_t items) {  // bloom_filter.rs:354-357, f32 arithmetic
    const float ln2 = 0.693147180559945309417232121458176568f;
    float ln22 = ln2 * ln2;
    float v = roundf((float)items * (logf(1.0f / rate) / ln22));
    return v <= 0 ? 0 : (uint64_t)v;
}
uint32_t optimal_num_hashes(uint64_t bits, uint32_t items) {  // bloom_filter.rs:342-350
    const float ln2 = 0.693147180559945309417232121458176568f;
    float v = roundf((float)bits / (float)items * ln2);
    uint32_t h = v <= 0 ? 0 : (uint32_t)v;
    return std::min<uint32_t>(std::max<uint32_t>(h, 2), 200);
}
int cmd_build_balanced(int argc, char **argv) {
    std::vector<Opt> opts = {{"genomes", 'g', true}, {"db-path", 'd', true}, {"threads", 't', true}, {"kmer-size", 'k', true},
                             {"cache-size", 'c', true}, {"false-pos-rate", 'f', true}, {"largest-genome", 'l', true},
                             {"format", 'F', true}, {"seed1", 0, true}, {"seed2", 0, true}};
    Args a = parse(argc, argv, 2, opts);
    const std::string genomes = req(a, "genomes"), db = req(a, "db-path");
    const uint64_t k = to_u64(opt(a, "kmer-size", "20"), "kmer-size");
    const float fpr = to_f32(opt(a, "false-pos-rate", "0.001"), "false-pos-rate");
    const uint32_t largest = (uint32_t)to_u64(opt(a, "largest-genome", "1000000"), "largest-genome");
    const uint64_t s1 = strtoull(opt(a, "seed1", "81985529216486895").c_str(), nullptr, 0);
    const uint64_t s2 = strtoull(opt(a, "seed2", "18364758544493064720").c_str(), nullptr, 0);
    ReadQueue rq(genomes, to_fmt(opt(a, "format", "auto")));
    rq.start(true, (unsigned)std::min<uint64_t>(to_u64(opt(a, "threads", "4"), "threads"), 256));
    Batch g;
    while (rq.fill(g, ~0ull, ~0ull)) {}  // block size 1 in the reference: one leaf per record (main.rs:148-200)
    if (!rq.pending_error.empty()) die(rq.pending_error);
    auto &seq = g.seq;
    auto &off = g.off;
    std::vector<std::string> ids;
    for (size_t r = 0; r < g.n(); ++r) ids.emplace_back(g.id(r));
    std::vector<const char *> idp;
    for (auto &s : ids) idp.push_back(s.c_str());
    const uint64_t nbits = needed_bits(fpr, largest);
    pfq_tree *tree = nullptr;
    seq.resize(seq.size() + 16);
    check(pfq_tree_build_balanced(seq.data(), off.data(), ids.size(), idp.data(), k, nbits, optimal_num_hashes(nbits, largest), s1,
                                  s2, fpr, largest, device_from_env(), &tree));
    mkdir(db.c_str(), 0777);
    check(pfq_tree_save(tree, db.c_str()));
    pfq_tree_close(tree);
    printf("Finished.\n");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// build / add (main.rs:148-247): one leaf per record, greedy placement by Hamming distance on the device
// ---------------------------------------------------------------------------------------------------------------
uint64_t random_seed() {  // HashSeed::new (hasher.rs:24-30) draws a random usize
    std::random_device rd;
    return ((uint64_t)rd() << 32) ^ (uint64_t)rd();
}
int insert_genomes(pfq_tree *tree, const std::string &genomes, FmtOverride ov, unsigned threads) {
    ReadQueue rq(genomes, ov);
    rq.start(true, threads);
    // the reference reads blocks of one record (ReadQueue::with_format(genomes, 1, …), main.rs:172,:229) and inserts
    // them in input order
    uint64_t n = 0;
    while (Segment *sg = rq.next_segment()) {
        for (size_t r = 0; r < sg->b.n(); ++r, ++n) {
            const std::string id(sg->b.id(r));
            check(pfq_tree_insert(tree, sg->b.seq.data() + sg->b.off[r], sg->b.off[r + 1] - sg->b.off[r], id.c_str(), nullptr));
        }
        if (!sg->err.empty()) die(sg->err);
        rq.recycle(sg);
    }
    return (int)n;
}
// ---------------------------------------------------------------------------------------------------------------
// recluster: the same leaves under a tree whose shape follows from the leaf filters (pfq_tree_recluster); no reference
// counterpart.  `build --cluster` is build followed by it, without the database in between.
// ---------------------------------------------------------------------------------------------------------------
const char *const MERGES_HEADER = "#node\tleft\tright\tleaves\tround\tscore_sum\tpairs\tsimilarity\n";
// The merge log of `made` = pfq_tree_recluster(src) as a dendrogram: one line per internal node in creation order.
void write_merges(pfq_tree *src, pfq_tree *made, const std::string &path) {
    const char *const *ids = nullptr;
    const uint64_t *counts = nullptr;
    uint64_t n_leaves = 0, n_merges = 0, n_clades = 0;
    check(pfq_leaf_counts(src, &ids, &counts, &n_leaves));
    std::vector<std::string> name(ids, ids + n_leaves);  // node -> name: src's leaves in order, then the new tree's internal nodes
    const pfq_merge *mg = nullptr;
    uint32_t rounds = 0;
    check(pfq_tree_merges(made, &mg, &n_merges, &rounds));
    // an internal node is the clade of the new tree with its leaf range: the new tree lists the leaves left subtree first
    const pfq_clade *clades = nullptr;
    check(pfq_tree_clades(made, &clades, &n_clades));
    std::map<std::pair<uint32_t, uint32_t>, std::string> by_range;
    for (uint64_t c = 0; c < n_clades; ++c)
        if (clades[c].n_leaves > 1) by_range[{clades[c].first_leaf, clades[c].n_leaves}] = clades[c].name;
    std::vector<uint32_t> first(n_leaves + n_merges, 0);
    if (n_merges) {
        uint32_t next_leaf = 0;
        std::vector<uint32_t> st{(uint32_t)(n_leaves + n_merges - 1)};
        while (!st.empty()) {  // pre-order: a node's first leaf is the next one to be numbered when the node is reached
            const uint32_t v = st.back();
            st.pop_back();
            first[v] = next_leaf;
            if (v < n_leaves) ++next_leaf;
            else {
                st.push_back(mg[v - n_leaves].right);
                st.push_back(mg[v - n_leaves].left);
            }
        }
    }
    name.resize(n_leaves + n_merges);
    for (uint64_t i = 0; i < n_merges; ++i) {
        auto it = by_range.find({first[mg[i].node], mg[i].n_leaves});
        if (it == by_range.end()) die("recluster: merge " + std::to_string(i) + " matches no node of the new tree");
        name[mg[i].node] = it->second;
    }
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) die("cannot create " + path + ": " + strerror(errno));
    fputs(MERGES_HEADER, f);
    for (uint64_t i = 0; i < n_merges; ++i) {
        const pfq_merge &m = mg[i];
        fprintf(f, "%s\t%s\t%s\t%u\t%u\t%llu\t%llu\t%.6f\n", name[m.node].c_str(), name[m.left].c_str(), name[m.right].c_str(), m.n_leaves, m.round,
                (unsigned long long)m.score_sum, (unsigned long long)m.pairs, (double)m.score_sum / ((double)m.pairs * 1048576.0));
    }
    if (fclose(f) != 0) die("short write to " + path);
}
// a path as far as it can be resolved, without trailing slashes: two spellings of one directory compare equal
std::string resolved(const std::string &p) {
    char buf[PATH_MAX];
    if (realpath(p.c_str(), buf)) return buf;
    std::string s = p;
    while (s.size() > 1 && s.back() == '/') s.pop_back();
    return s;
}
int cmd_recluster(int argc, char **argv) {
    std::vector<Opt> opts = {{"db-path", 'd', true}, {"out", 'o', true}, {"merges", 0, true}, {"device", 0, true}};
    Args a = parse(argc, argv, 2, opts);
    // every option is checked before a device is touched
    const std::string db = req(a, "db-path"), out = req(a, "out");
    if (out.empty()) die("error: invalid value '' for '--out': the directory of the new database");
    if (resolved(db) == resolved(out))
        die("error: invalid value '" + out + "' for '--out': the same directory as '--db-path' (the new database is written beside the old one, not over it)");
    const bool want_merges = a.val.count("merges") != 0;
    if (want_merges && a.val.at("merges").empty()) die("error: invalid value '' for '--merges': a file name");
    const int device = a.val.count("device") ? (int)to_u64(a.val.at("device"), "device") : device_from_env();

    const uint64_t t0 = ReadQueue::now_ns();
    pfq_tree *src = nullptr, *made = nullptr;
    check(pfq_tree_open(db.c_str(), device, &src));
    check(pfq_tree_recluster(src, &made));
    mkdir(out.c_str(), 0777);
    check(pfq_tree_save(made, out.c_str()));
    if (want_merges) write_merges(src, made, a.val.at("merges"));
    const pfq_merge *mg = nullptr;
    uint64_t n_merges = 0;
    uint32_t rounds = 0;
    check(pfq_tree_merges(made, &mg, &n_merges, &rounds));
    pfq_tree_close(made);
    pfq_tree_close(src);
    printf("Reclustered %llu genomes in %u rounds into %s, %.3f s\n", (unsigned long long)(n_merges + 1), rounds, out.c_str(), (ReadQueue::now_ns() - t0) * 1e-9);
    return 0;
}

int cmd_build(int argc, char **argv) {
    std::vector<Opt> opts = {{"genomes", 'g', true}, {"db-path", 'd', true}, {"threads", 't', true}, {"kmer-size", 'k', true},
                             {"cache-size", 'c', true}, {"false-pos-rate", 'f', true}, {"largest-genome", 'l', true},
                             {"format", 'F', true}, {"seed1", 0, true}, {"seed2", 0, true}, {"cluster", 0, false}};
    Args a = parse(argc, argv, 2, opts);
    const std::string genomes = req(a, "genomes"), db = req(a, "db-path");
    const uint64_t k = to_u64(opt(a, "kmer-size", "20"), "kmer-size");
    const float fpr = to_f32(opt(a, "false-pos-rate", "0.001"), "false-pos-rate");
    const uint32_t largest = (uint32_t)to_u64(opt(a, "largest-genome", "1000000"), "largest-genome");
    (void)to_u64(opt(a, "cache-size", "10"), "cache-size");  // every filter stays in HBM while the tree is built
    const unsigned threads = (unsigned)std::min<uint64_t>(to_u64(opt(a, "threads", "4"), "threads"), 256);
    // --seed1/--seed2 are ours: the reference always draws the two hash seeds at random (bloom_tree.rs:114)
    const uint64_t s1 = a.val.count("seed1") ? strtoull(a.val.at("seed1").c_str(), nullptr, 0) : random_seed();
    const uint64_t s2 = a.val.count("seed2") ? strtoull(a.val.at("seed2").c_str(), nullptr, 0) : random_seed();
    printf("Building the SBT...\n");
    mkdir(db.c_str(), 0777);  // BloomTree::new creates the directory (bloom_tree.rs:107)
    pfq_tree *tree = nullptr;
    check(pfq_tree_create(k, fpr, largest, s1, s2, 0, device_from_env(), &tree));
    insert_genomes(tree, genomes, to_fmt(opt(a, "format", "auto")), threads);
    if (a.flags.count("cluster")) {  // --cluster: what `recluster` would make of the database this build would have saved
        pfq_tree *made = nullptr;
        check(pfq_tree_recluster(tree, &made));
        pfq_tree_close(tree);
        tree = made;
    }
    check(pfq_tree_save(tree, db.c_str()));
    pfq_tree_close(tree);
    printf("Finished.\n");
    return 0;
}
int cmd_add(int argc, char **argv) {
    std::vector<Opt> opts = {{"genomes", 'g', true}, {"db-path", 'd', true}, {"threads", 't', true}, {"cache-size", 'c', true},
                             {"format", 'F', true}};
    Args a = parse(argc, argv, 2, opts);
    const std::string genomes = req(a, "genomes"), db = req(a, "db-path");
    (void)to_u64(opt(a, "cache-size", "10"), "cache-size");
    const unsigned threads = (unsigned)std::min<uint64_t>(to_u64(opt(a, "threads", "4"), "threads"), 256);
    printf("Adding new genomes to the SBT...\n");
    pfq_tree *tree = nullptr;
    check(pfq_tree_open(db.c_str(), device_from_env(), &tree));
    insert_genomes(tree, genomes, to_fmt(opt(a, "format", "auto")), threads);
    check(pfq_tree_save(tree, db.c_str()));
    pfq_tree_close(tree);
    printf("Finished.\n");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// ingest-check: parse the input exactly like `query` does and print what was read (no GPU involved).  Used by the
// CPU tests to pin the parallel reader against a sequential one and against the reference's parsing rules.
// ---------------------------------------------------------------------------------------------------------------
int cmd_ingest_check(int argc, char **argv) {
    std::vector<Opt> opts = {{"reads", 'r', true}, {"threads", 't', true}, {"format", 'F', true}, {"dump", 0, false},
                             {"count", 0, false}, {"block-size-reads", 'b', true}, {"reads2", 0, true}, {"interleaved", 0, false}};
    Args a = parse(argc, argv, 2, opts);
    // --reads2 / --interleaved: the fragments exactly as `query` pairs them, mates adjacent (-b counts fragments)
    const bool interleaved = a.flags.count("interleaved") != 0, has_reads2 = a.val.count("reads2") != 0;
    if (interleaved && has_reads2) die("error: the argument '--reads2 <READS2>' cannot be used with '--interleaved'");
    const bool paired = interleaved || has_reads2;
    const FmtOverride ov = to_fmt(opt(a, "format", "auto"));
    ReadQueue rq(req(a, "reads"), ov);
    std::unique_ptr<ReadQueue> rq2;
    if (has_reads2) rq2.reset(new ReadQueue(a.val.at("reads2"), ov));
    const bool count_only = a.flags.count("count") != 0;  // what `query` without filtering keeps: bases and offsets only
    if (count_only && paired) die("error: '--count' cannot be used with '--reads2' or '--interleaved' (mates keep their ids)");
    const unsigned threads = (unsigned)std::min<uint64_t>(to_u64(opt(a, "threads", "4"), "threads"), 256);
    rq.start(!count_only, threads);
    if (rq2) rq2->start(true, threads);
    PairSource src{rq, rq2.get(), {}, {}, 0, {}, false};
    const uint64_t block = std::max<uint64_t>(1, to_u64(opt(a, "block-size-reads", "1000000"), "block-size-reads"));
    const bool dump = a.flags.count("dump") != 0;
    uint64_t n = 0, bytes = 0, h = 0xcbf29ce484222325ull;
    auto mix = [&](const void *p, size_t len) {
        const unsigned char *c = (const unsigned char *)p;
        for (size_t i = 0; i < len; ++i) h = (h ^ c[i]) * 0x100000001b3ull;
        h = (h ^ 0xff) * 0x100000001b3ull;
    };
    Batch b;
    bool more = true;
    while (more) {
        b.clear();
        more = paired ? src.next(b, block) : rq.fill(b, block, ~0ull);
        if (count_only) {
            n += b.n();
            bytes += b.seq.size();
            continue;
        }
        for (size_t r = 0; r < b.n(); ++r) {
            const std::string_view id = b.id(r);
            const uint64_t o = b.off[r], len = b.off[r + 1] - o;
            mix(id.data(), id.size());
            mix(b.seq.data() + o, len);
            const std::string_view q = b.quality(r);
            if (b.has_qual[r]) mix(q.data(), q.size());
            if (dump) {
                printf("%c%.*s\x01%.*s\x01%.*s\n", b.has_qual[r] ? '@' : '>', (int)id.size(), id.data(), (int)len,
                       (const char *)b.seq.data() + o, (int)q.size(), q.data());
            }
            ++n;
            bytes += len;
        }
    }
    printf("reads=%llu bases=%llu fnv=%016llx\n", (unsigned long long)n, (unsigned long long)bytes, (unsigned long long)h);
    rq.report_timing();
    if (!src.err.empty()) die(src.err);
    if (!rq.pending_error.empty()) die(rq.pending_error);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// compare: which genomes of a database (or of two) are related, from the leaf filters (pfq_tree_similarity); no reference
// counterpart.  SIMILARITY.tsv in --out, one line per pair of leaves whose larger containment reaches --min-containment.
// ---------------------------------------------------------------------------------------------------------------
const char *const SIMILARITY_HEADER =
    "#genome_a\tgenome_b\tbits_a\tbits_b\tshared_bits\tkmers_a\tkmers_b\tshared_kmers\tjaccard\tcontainment_a\tcontainment_b\tani\n";
int cmd_compare(int argc, char **argv) {
    std::vector<Opt> opts = {{"db-path", 'd', true}, {"out", 'o', true}, {"against", 0, true}, {"min-containment", 0, true}, {"device", 0, true}};
    Args a = parse(argc, argv, 2, opts);
    // every option is checked before a device is touched
    const std::string db = req(a, "db-path"), out = req(a, "out");
    const bool two = a.val.count("against") != 0;
    const std::string mc = opt(a, "min-containment", "0.1");
    char *end = nullptr;
    const double min_c = strtod(mc.c_str(), &end);
    if (mc.empty() || !end || *end || !(min_c >= 0.0 && min_c <= 1.0))
        die("error: invalid value '" + mc + "' for '--min-containment': a number from 0 to 1 (0 writes every pair)");
    const int device = a.val.count("device") ? (int)to_u64(a.val.at("device"), "device") : device_from_env();

    const uint64_t t0 = ReadQueue::now_ns();
    pfq_tree *ta = nullptr, *tb = nullptr;
    check(pfq_tree_open(db.c_str(), device, &ta));
    if (two) check(pfq_tree_open(a.val.at("against").c_str(), device, &tb));
    pfq_tree *const other = two ? tb : ta;
    pfq_info info{};
    check(pfq_tree_info(ta, &info));
    auto names_of = [](pfq_tree *t) {
        const char *const *ids = nullptr;
        const uint64_t *counts = nullptr;
        uint64_t n = 0;
        check(pfq_leaf_counts(t, &ids, &counts, &n));
        return std::vector<std::string>(ids, ids + n);
    };
    const std::vector<std::string> names_a = names_of(ta), names_b = two ? names_of(tb) : names_a;
    const uint64_t na = names_a.size(), nb = names_b.size();
    {  // one pair first: two databases that cannot be compared are refused, in the library's words, before --out is touched
        const uint32_t zero = 0;
        pfq_similarity probe{};
        check(pfq_tree_similarity(ta, &zero, 1, other, &zero, 1, &probe));
    }
    // the directory convention of query's --out (main.rs:380-391): an existing output directory is deleted
    struct stat st;
    if (stat(out.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) rm_rf(out);
    mkdir(out.c_str(), 0777);
    const std::string tsv = out + "/SIMILARITY.tsv";
    FILE *f = fopen(tsv.c_str(), "wb");
    if (!f) die("cannot create " + tsv + ": " + strerror(errno));
    fputs(SIMILARITY_HEADER, f);
    // Panels of at most 1024 leaves of a by as many of b as stay under the library's 2^26 pairs a call; one database against
    // itself: only the panels on or above the diagonal, and of those the pairs a < b.  The file is ordered by a, then b: a panel
    // that holds all of its rows' columns (every panel, up to 65 536 leaves of b) is written row by row as it comes; only where
    // the columns are cut into several panels are a row's lines kept until its last panel is in.
    constexpr uint64_t PANEL_A = 1024, MAX_PAIRS = 1ull << 26;
    uint64_t compared = 0, written = 0;
    std::vector<uint32_t> la, lb;
    std::vector<std::string> rows;
    char line[256];
    for (uint64_t a0 = 0; a0 < na; a0 += PANEL_A) {
        const uint64_t a1 = std::min(na, a0 + PANEL_A), pb = MAX_PAIRS / (a1 - a0);
        la.resize(a1 - a0);
        for (uint64_t i = a0; i < a1; ++i) la[i - a0] = (uint32_t)i;
        const uint64_t b_first = two ? 0 : a0;
        const bool direct = nb - b_first <= pb;  // one panel of columns
        rows.assign(direct ? 1 : a1 - a0, std::string());
        for (uint64_t b0 = b_first; b0 < nb; b0 += pb) {
            const uint64_t b1 = std::min(nb, b0 + pb);
            lb.resize(b1 - b0);
            for (uint64_t j = b0; j < b1; ++j) lb[j - b0] = (uint32_t)j;
            pfq_similarity sm{};
            check(pfq_tree_similarity(ta, la.data(), la.size(), other, lb.data(), lb.size(), &sm));
            for (uint64_t i = a0; i < a1; ++i) {
                std::string &row = rows[direct ? 0 : i - a0];
                for (uint64_t j = two ? b0 : std::max(b0, i + 1); j < b1; ++j) {
                    const uint64_t at = (i - a0) * sm.n_b + (j - b0);
                    const double ka = sm.kmers_a[i - a0], kb = sm.kmers_b[j - b0], sh = sm.shared_kmers[at], jac = sm.jaccard[at];
                    const double ca = ka > 0.0 ? sh / ka : 0.0, cb = kb > 0.0 ? sh / kb : 0.0;
                    ++compared;
                    if (!(std::max(ca, cb) >= min_c)) continue;
                    const double ani = jac > 0.0 ? 1.0 + std::log(2.0 * jac / (1.0 + jac)) / (double)info.kmer_size : 0.0;
                    snprintf(line, sizeof line, "\t%llu\t%llu\t%u\t%.1f\t%.1f\t%.1f\t%.6f\t%.6f\t%.6f\t%.6f\n", (unsigned long long)sm.bits_a[i - a0],
                             (unsigned long long)sm.bits_b[j - b0], sm.shared_bits[at], ka, kb, sh, jac, ca, cb, ani);
                    row += names_a[i] + "\t" + names_b[j] + line;
                    ++written;
                }
                if (direct) {
                    fwrite(row.data(), 1, row.size(), f);
                    row.clear();
                }
            }
        }
        if (!direct)
            for (const std::string &r : rows) fwrite(r.data(), 1, r.size(), f);
    }
    if (fclose(f) != 0) die("short write to " + tsv);
    if (tb) pfq_tree_close(tb);
    pfq_tree_close(ta);
    printf("Compared %llu x %llu genomes: %llu pairs compared, %llu written to %s, %.3f s\n", (unsigned long long)na, (unsigned long long)nb,
           (unsigned long long)compared, (unsigned long long)written, tsv.c_str(), (ReadQueue::now_ns() - t0) * 1e-9);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// taxonomy: the node table a taxonomy file gives over a database's genomes (tree.bin and the file only: no device)
// ---------------------------------------------------------------------------------------------------------------
int cmd_taxonomy(int argc, char **argv) {
    std::vector<Opt> opts = {{"db-path", 'd', true}, {"taxonomy", 0, true}, {"out", 'o', true}};
    Args a = parse(argc, argv, 2, opts);
    const std::string db_path = req(a, "db-path"), file = req(a, "taxonomy"), out = req(a, "out");
    const char *const *ids = nullptr;
    uint64_t n_ids = 0;
    check(pfq_db_leaf_ids(db_path.c_str(), &ids, &n_ids));
    pfq_taxonomy_file tf{};
    check(pfq_taxonomy_read(file.c_str(), ids, n_ids, &tf));
    fprintf(stderr, "taxonomy: %llu taxa from %llu lines; %llu lines for genomes that are not in the database; %llu of %llu genomes without a line sit under the root\n",
            (unsigned long long)tf.n_taxa, (unsigned long long)tf.lines_considered, (unsigned long long)tf.lines_other,
            (unsigned long long)tf.leaves_without_line, (unsigned long long)tf.n_leaves);
    const pfq_taxon *tx = nullptr;
    uint64_t n = 0;
    check(pfq_taxonomy_nodes(n_ids, ids, tf.n_taxa, tf.taxon_parent, tf.taxon_names, tf.leaf_taxon, &tx, &n));
    mkdir(out.c_str(), 0777);
    const std::string tsv = out + "/TAXA.tsv";
    FILE *f = fopen(tsv.c_str(), "wb");
    if (!f) die("cannot create " + tsv + ": " + strerror(errno));
    fputs("#node\tparent\tdepth\tkind\tgenomes\tname\n", f);
    for (uint64_t v = 0; v < n; ++v) {
        const std::string parent = tx[v].parent == PFQ_NO_CLADE ? "-" : std::to_string(tx[v].parent);
        fprintf(f, "%llu\t%s\t%u\t%s\t%u\t%s\n", (unsigned long long)v, parent.c_str(), tx[v].depth, tx[v].leaf == PFQ_NO_CLADE ? "taxon" : "genome",
                tx[v].n_leaves, tx[v].name);
    }
    if (fclose(f) != 0) die("short write to " + tsv);
    return 0;
}

// bgzf: a plain or gzip file rewritten as blocked gzip (BGZF) with zlib: members of 65 280 text bytes, each with its compressed
// size in a 'BC' extra subfield, then the 28-byte end marker.  What pfq_gz_scan takes and every htslib tool reads.
int cmd_bgzf(int argc, char **argv) {
    std::vector<Opt> opts = {{"in", 'i', true}, {"out", 'o', true}, {"level", 0, true}};
    Args a = parse(argc, argv, 2, opts);
    const std::string in = req(a, "in"), out = req(a, "out");
    int level = 6;
    if (a.val.count("level")) {
        char *end = nullptr;
        const long v = strtol(a.val["level"].c_str(), &end, 10);
        if (!*a.val["level"].c_str() || *end || v < 0 || v > 9) die("error: '--level' must be 0 .. 9, not '" + a.val["level"] + "'");
        level = (int)v;
    }
    constexpr size_t BLOCK = BGZF_TEXT;
    gzFile f = gzopen(in.c_str(), "rb");  // (transparent for plain files)
    if (!f) die("Failed to open '" + in + "': " + strerror(errno));
    gzbuffer(f, 1 << 20);
    FILE *o = fopen(out.c_str(), "wb");
    if (!o) die("cannot create " + out + ": " + strerror(errno));
    std::vector<unsigned char> text(BLOCK), member(BGZF_ROOM);
    uint64_t n_members = 0, n_text = 0, n_out = 0;
    auto put_member = [&](size_t n) {
        const size_t size = bgzf_member(text.data(), n, level, member.data());
        if (fwrite(member.data(), 1, size, o) != size) die("short write to " + out);
        ++n_members;
        n_text += n;
        n_out += size;
    };
    while (true) {
        size_t have = 0;
        while (have < BLOCK) {
            const int got = gzread(f, text.data() + have, (unsigned)(BLOCK - have));
            if (got < 0) die("read error (corrupt gzip?)");
            if (got == 0) break;
            have += (size_t)got;
        }
        if (!have) break;
        put_member(have);
        if (have < BLOCK) break;
    }
    put_member(0);  // the end marker
    gzclose(f);
    if (fclose(o) != 0) die("short write to " + out);
    fprintf(stderr, "bgzf: %llu bytes of text in %llu members and the end marker, %llu bytes written\n", (unsigned long long)n_text,
            (unsigned long long)(n_members - 1), (unsigned long long)n_out);
    return 0;
}

// asked: --help / -h was given, and the text ends with the options that came after the wording of the bare usage message was
// recorded (tests/golden/cli_query_refusals.json holds that message byte for byte)
void usage(bool asked = false) {
    std::string header_cols(SIMILARITY_HEADER);  // the column line as the file has it, tabs spelt out
    header_cols.pop_back();
    for (size_t p = 0; (p = header_cols.find('\t', p)) != std::string::npos;) header_cols.replace(p, 1, "<TAB>");
    std::string merges_cols(MERGES_HEADER);
    merges_cols.pop_back();
    for (size_t p = 0; (p = merges_cols.find('\t', p)) != std::string::npos;) merges_cols.replace(p, 1, "<TAB>");
    fprintf(stderr,
            "A fast, simple and memory efficient metagenomic filtering tool. (MI355X query path)\n\n"
            "Usage: phage_filter [-v...|-q...] <COMMAND>\n\nCommands:\n"
            "  query           Queries a set of reads. (ran after building the bloom tree)\n"
            "  build           Builds the BloomTree.\n"
            "  add             Adds genomes to an already built BloomFilter.\n"
            "  compare         Says which genomes of a database are related, and how closely, from their Bloom filters\n"
            "  recluster       Writes a database with the same genomes under a tree rebuilt by their similarity\n"
            "  taxonomy        Checks a taxonomy file against a database and writes the node table it gives (no GPU)\n"
            "  bgzf            Rewrites a plain or gzip file as blocked gzip: bgzf -i IN -o OUT [--level 0..9] (no GPU)\n"
            "  build-balanced  Builds a balanced synthetic BloomTree on the GPU (benchmark databases)\n"
            "  ingest-check    Parses reads like `query` and prints what was read (no GPU)\n\n"
            "query takes the reference's options, plus --devices <0,1,..|all>: one replica of the database per GPU, reads\n"
            "dealt over them, per-genome counts combined by one RCCL all-reduce (default: device $PFQ_DEVICE or 0), and\n"
            "--shard-depth <D>: the database split into the subtree shards of its depth-D frontier (depth min(D, --search-depth)),\n"
            "shard i on device i mod N of the N listed; every shard sees every read and loads only its own .bf files, so a\n"
            "database larger than one GPU's memory can be queried.  Needs at least N shards.  Same outputs as the whole tree\n"
            "--scores: also write READ_SCORES.tsv into --out: per read record and genome it hits, how many of the read's k-mers\n"
            "the genome's filter contains (\"#read_id<TAB>kmers<TAB>genome<TAB>matched_kmers\", best genome first)\n"
            "--reads2 <R2>: paired-end reads, R1 from -r and R2 from here (files or directories; mates by record index), or\n"
            "--interleaved: the mates are adjacent records of -r.  Mate ids must agree once a trailing /1 (R1) and /2 (R2) are\n"
            "stripped; a mismatch or one stream ending first is fatal after the fragments before it.  Every mate is judged on\n"
            "its own; the fragment's genomes are the union of its mates' (--pair-mode either, the default) or their\n"
            "intersection (--pair-mode both).  CLASSIFICATION.csv counts fragments; -b counts fragments.  A fragment with\n"
            "genomes goes to POS, both mates alike, each under its own id with the fragment's \" |g1,g2\":\n"
            "POS_FILTERING_1/_2 and NEG_FILTERING_1/_2 (--interleaved: POS_FILTERING / NEG_FILTERING, mates adjacent).\n"
            "With --scores: one line per fragment and genome, R1's id, both mates' k-mers and matched k-mers summed.\n"
            "--lca <all|best>: also assign every read to the lowest common ancestor (LCA) of the genomes it hits in the tree,\n"
            "the smallest group of genomes the read cannot tell apart, and write CLADE_COUNTS.tsv into --out: one row per node\n"
            "with reads at or below it, nodes numbered in pre-order (\"#clade<TAB>parent<TAB>depth<TAB>genomes<TAB>name<TAB>\n"
            "reads_here<TAB>reads_below\"; parent is - for the root; paired input: fragments).  The other outputs stay as they are.\n"
            "--lca best: the LCA of the genomes with the read's highest --scores value only (ties stay ambiguous); it asks the\n"
            "library for hits and scores, READ_SCORES.tsv is still written with --scores only.  Not with --shard-depth: a\n"
            "shard holds only its own part of the tree.  With --devices the replicas' counts are summed.\n"
            "--lca-reads (needs --lca): also write READ_LCA.tsv, one line per record with hits in input order (per fragment:\n"
            "R1's id): \"#read_id<TAB>hits<TAB>clade<TAB>name\", hits = the number of genomes hit (also with --lca best)\n"
            "--abundance: also estimate how many reads (paired input: fragments) every genome produced, and write ABUNDANCE.tsv\n"
            "into --out.  A read that hits several related genomes counts once for each of them in CLASSIFICATION.csv; here an\n"
            "EM over all reads' hit lists shares it among them in proportion to the genomes' estimated abundances, so a relative\n"
            "of a genome that is present keeps little more than the reads only it explains.  \"#genome<TAB>unique<TAB>estimated\n"
            "<TAB>fraction\", a second # line with the run's totals, then one row per genome with estimated > 0 (unique: reads that\n"
            "hit this genome alone).  Reads that hit every genome or none are left out.  Every query call then asks the library\n"
            "for the hit lists, the counts-only mode (no filter, no --scores) too, which so runs at the hit-list rate.  The other\n"
            "outputs stay as they are.  Not with --shard-depth: a shard sees only its own genomes.  With --devices the replicas'\n"
            "logs are merged before the estimate.  --abundance-iters <N> (needs --abundance): at most N EM iterations (default 200)\n"
            "--coverage: also count, per genome, the distinct k-mers its reads (paired input: fragments, both mates) matched, and\n"
            "write COVERAGE.tsv into --out: 5 000 reads piled onto one shared gene and 5 000 reads that tile a genome look the same\n"
            "in CLASSIFICATION.csv; here the first shows few distinct k-mers under many reads.  \"#genome<TAB>units<TAB>matched_kmers\n"
            "<TAB>distinct_kmers<TAB>genome_kmers<TAB>breadth<TAB>duplication\", one line per genome in CLASSIFICATION.csv's order, zeros\n"
            "included: units = reads that list the genome, matched_kmers = their k-mers the genome's filter contains, distinct_kmers =\n"
            "a HyperLogLog estimate of the distinct ones among them, genome_kmers = the genome's own distinct k-mers estimated from\n"
            "its filter's fill (0.0: filter full, not estimable), breadth = distinct_kmers / genome_kmers (not clamped), duplication =\n"
            "matched_kmers / distinct_kmers.  Every query call then asks the library for the hit lists, as with --abundance.  The other\n"
            "outputs stay as they are.  Works with --shard-depth (the shards' lines follow one another) and with --devices (the\n"
            "replicas' sketches are merged first).  --coverage-precision <P> (needs --coverage): 2^P one-byte registers per genome,\n"
            "4 to 16 (default 12: 4 KiB per genome, standard error 1.6 %%)\n"
            "--frame <F> [--frame-step <S>]: for contigs and long reads.  Every sequence is cut into overlapping frames of F bases\n"
            "every S bases (default S = max(F / 2, 1); the last frame is flush with the sequence's end), every frame is classified like a\n"
            "read at -f, runs of consecutive frames that hit a genome become segments, and SEGMENTS.tsv in --out says where each lies:\n"
            "\"sequence<TAB>genome<TAB>begin<TAB>end<TAB>match_begin<TAB>match_end<TAB>frames<TAB>kmers<TAB>matched<TAB>longest_run\", one line per\n"
            "segment in input order, then by first frame and genome; coordinates are 0-based and half-open; kmers / matched: k-mer\n"
            "positions of [begin, end) and those the genome's filter contains, match_begin / match_end: from the first to the end of the\n"
            "last of them, longest_run: the longest stretch of consecutive ones.  Sequences without segments have no line.\n"
            "CLASSIFICATION.csv then counts sequences, one per genome with a segment.  Works with --devices (whole sequences are dealt to\n"
            "the replicas; the files do not depend on the device list, -t or the batch size).  Not with --reads2, --interleaved,\n"
            "--scores, --lca, --abundance, --coverage, --shard-depth, --pos-filter or --neg-filter; F must be at least the database's k\n"
            "--device-parse: plain (not gzip) FASTA / FASTQ files are parsed on the GPU: the host threads only read file bytes, kernels\n"
            "find the lines, check that the records are ordinary (FASTQ: four lines each) and gather the sequences.  Where the text is\n"
            "anything else (multi-line FASTQ, malformed records) the host reader takes over from exactly that record, so every output and\n"
            "every error is what the run without the option gives.  For runs that only count: with -f, -b, -t, --search-depth, --devices,\n"
            "-F and --lca all.  Not with --pos-filter, --neg-filter, --scores, --lca best, --lca-reads, --reads2, --interleaved,\n"
            "--abundance, --coverage, --frame or --shard-depth\n"
            "--device-inflate (needs --device-parse): blocked gzip files (BGZF: what bgzip, the sequencers' converters and\n"
            "`phage_filter bgzf` write) are inflated on the GPU too: the host threads read chunks of whole members, found by walking the\n"
            "members' headers, and every member is inflated by a wave of its own.  Where the file has anything else (bytes that are no\n"
            "member, a member the device does not follow to the letter, records that are not ordinary, a file that ends inside a\n"
            "record) the streaming host reader takes over from exactly the first record not taken, so every output and every error is\n"
            "what the run without the option gives.  Other gzip files keep the host reader, as they do under --device-output\n"
            "--device-output (needs --pos-filter and / or --neg-filter): the POS / NEG records of plain (not gzip) FASTA / FASTQ files are\n"
            "parsed, classified and formatted on the GPU: the host threads only read file bytes and write the output streams.  The\n"
            "device writes the blocks of -b reads whose ids are all different; blocks with a repeated id, the reads at the edges of a\n"
            "chunk, gzip files and everything the host reader takes over go through the host formatter, so every output and every\n"
            "error is what the run without the option gives.  -b at most 8192.  With -f, -b, -t, --search-depth, --devices, -F and\n"
            "--lca all.  Not with --device-parse, and not with anything --device-parse refuses other than the two filters\n"
            "--taxonomy <FILE>: the tree's shape is an index, not a classification; this lays a taxonomy of your own over the database's\n"
            "genomes and counts the reads (paired input: fragments) at every rank.  FILE has one line per genome, \"genome<TAB>lineage\",\n"
            "the lineage a ';'-separated list of names from the top rank down (\"Caudoviricetes;Autographiviridae;Teseptimavirus\"; empty:\n"
            "directly under the root; further columns are ignored, as are empty lines and lines that begin with #).  A taxon is its whole\n"
            "path.  Lines for genomes that are not in the database are skipped and genomes without a line sit under the root; both are\n"
            "counted on stderr.  The file is checked before any GPU is used; an error names its line.  TAXON_COUNTS.tsv in --out:\n"
            "\"#node<TAB>parent<TAB>depth<TAB>kind<TAB>genomes<TAB>name<TAB>reads_here<TAB>reads_below<TAB>reads_any\", one line per node with\n"
            "reads_any > 0, nodes in pre-order, every genome a node (kind genome) under its taxon (kind taxon).  reads_here: reads whose\n"
            "genomes all lie under this node and under no deeper one (Kraken's clade report); reads_below: the sum of that over the node's\n"
            "subtree; reads_any: reads with at least one genome under the node, each counted once — what CLASSIFICATION.csv means, at every\n"
            "rank (for a genome line it is that file's count).  With --abundance one more column, estimated: the sum of ABUNDANCE.tsv's\n"
            "estimates over the genomes under the node.  Every query call then asks the library for the hit lists, as with --abundance.\n"
            "The other outputs stay as they are.  With --devices the replicas' counts are summed.  Not with --shard-depth, --frame or\n"
            "--device-parse.  --taxon-reads (needs --taxonomy): also write READ_TAXA.tsv, one line per record with hits in input order\n"
            "(per fragment: R1's id): \"#read_id<TAB>hits<TAB>node<TAB>name\"\n"
            "--best-hits (needs --taxonomy, --abundance or --coverage): below -f 1 a read from one strain also passes that strain's\n"
            "relatives, although its scores say which genome fits best.  With this option TAXON_COUNTS.tsv, READ_TAXA.tsv, ABUNDANCE.tsv\n"
            "(and the estimated column of TAXON_COUNTS.tsv) and COVERAGE.tsv are computed from every read's (fragment's) best-scoring\n"
            "genomes: those of its hits that contain the most of its k-mers, ties kept.  The reduction runs on the GPU; every query call\n"
            "then asks the library for hits and scores (READ_SCORES.tsv is still written with --scores only).  CLASSIFICATION.csv, POS / NEG,\n"
            "READ_SCORES.tsv, CLADE_COUNTS.tsv, READ_LCA.tsv and the hits column of READ_TAXA.tsv (the size of the whole hit set) stay as\n"
            "they are.  At -f 1 it changes nothing.  Works with --reads2 / --interleaved and --devices.  Not with --shard-depth, --frame or\n"
            "--device-parse\n"
            "--sweep <T1,T2,..> (1 to 16 thresholds, strictly ascending, none below -f): choosing -f otherwise costs one whole run per\n"
            "candidate.  With this option the one pass at -f also counts, per listed threshold, what a run of its own at that threshold\n"
            "would report, from the hits and scores the GPU already holds.  THRESHOLDS.tsv: \"#threshold<TAB>reads<TAB>reads_hit<TAB>\n"
            "reads_unique<TAB>assignments<TAB>genomes_hit\", one line per threshold: the reads POS filtering would keep, those that name one\n"
            "genome only, the (read, genome) pairs and the genomes with a read.  THRESHOLD_GENOMES.tsv: \"#genome<TAB>threshold<TAB>reads\n"
            "<TAB>unique_reads\", one line per genome and threshold with reads, genomes in CLASSIFICATION.csv's order: reads is that run's\n"
            "CLASSIFICATION.csv count.  Every other output stays as it is.  Works with --devices.  Needs a database whose parent filters\n"
            "contain their children's (every database build, add and recluster make).  Not with --reads2, --interleaved, --shard-depth,\n"
            "--frame or --device-parse\n"
            "--trim-quality <Q> --trim-window <W> --trim-poly-x <P> --min-length <L> --max-n <N> --min-complexity <C>: nobody classifies raw\n"
            "reads; any of these trims and filters every read on the GPU before it is classified, as a trimmer in front of the run would:\n"
            "leading bases below Phred Q go, the read is cut at the first window of W bases (default 4) whose mean quality is below Q and\n"
            "then back to its last base of at least Q; a tail of P or more equal bases (poly-G) goes; then a read shorter than L (default:\n"
            "the database's k, so that no read without a k-mer counts at every genome; at least 1), with more than N bases other than A C G\n"
            "T, or with fewer than C percent of its adjacent bases differing is dropped.  FASTA reads have no qualities: the other steps\n"
            "apply.  With --reads2 / --interleaved a fragment is dropped when either mate is.  Every output is, byte for byte, that of the\n"
            "same command without these options on an input that holds only the kept reads, each cut to what was kept, ids unchanged;\n"
            "PREPROCESS.tsv in --out adds \"key<TAB>value\" lines: reads, reads_kept, reads_trimmed, dropped_short, dropped_n,\n"
            "dropped_complexity, dropped_mate, bases, bases_kept, then the parameters in force; the totals are also printed on stderr.\n"
            "Works with every other output, with pairs and with --devices.  Not with --device-parse, --frame or --shard-depth\n"
            "--adapter <SEQ[,SEQ..]> [--adapter2 <SEQ[,SEQ..]>] [--adapter-overlap <O>] [--adapter-errors <E>]: a library whose inserts are\n"
            "shorter than its reads reads through into the 3' adapter, and such a read matches no genome; these cut every read, on the GPU\n"
            "and before the steps above, at the leftmost place where an adapter matches over at least O bases (default 5; at the read's\n"
            "end a part of the adapter is enough) with at most E percent mismatches (default 10; no insertions or deletions).  --adapter\n"
            "serves reads and first mates, --adapter2 second mates (needs --reads2 or --interleaved; without it they use --adapter's); both\n"
            "may be repeated, up to 8 adapters of O to 64 bases each.  A SEQ is a sequence over ACGT or a name: illumina\n"
            "(AGATCGGAAGAGC), nextera (CTGTCTCTTATACACATCT), smallrna (TGGAATTCTCGGGTGCCAAGG).  They turn the preprocessing above on\n"
            "(--min-length defaults to k) and are refused where it is, and with --device-output.  PREPROCESS.tsv then also holds\n"
            "adapter_reads, adapter_bases, adapter_overlap, adapter_errors and one adapter1.<SEQ> / adapter2.<SEQ> line with the reads cut\n"
            "by each adapter; a read cut by an adapter and kept counts in reads_trimmed\n"
            "--mate-overlap <O> [--mate-overlap-errors <E>]: paired reads say where their adapters begin themselves: when the insert is\n"
            "shorter than the reads, the mates are reverse complements of each other over the whole insert, and what follows is adapter,\n"
            "whatever its sequence.  On the GPU and before the steps above, the insert of every fragment is the largest length at which the\n"
            "mates overlap over at least O bases (1 to 512) with at most E percent mismatches (default 10; no insertions or deletions), and\n"
            "both mates are cut there; a fragment with a mate of more than 512 bases is left alone.  Needs --reads2 or --interleaved.\n"
            "Works with --adapter: each read is cut where the first of the two says.  Turns the preprocessing above on (--min-length\n"
            "defaults to k) and is refused where it is, and with --device-output.  PREPROCESS.tsv then also holds overlap_fragments (the\n"
            "fragments looked at), overlap_skipped, overlap_found, overlap_readthrough (insert shorter than a mate), overlap_reads,\n"
            "overlap_bases (reads and bases cut), mate_overlap and mate_overlap_errors, and INSERT_SIZES.tsv in --out holds\n"
            "\"insert<TAB>fragments\", one line per insert length found, ascending\n"
            "--mate-correct [--mate-correct-quality <HI[,LO]>]: inside the overlap every base was read twice.  Where the mates disagree\n"
            "there, a base with Phred quality LO or less (default 14; an N too) takes what its mate says, and the mate's quality, if\n"
            "that one is ACGT with quality HI or more (default 30); other disagreements stay as they are.  On the GPU, as part of the\n"
            "--mate-overlap step, which it needs, and before trimming: at -f 1.0 one wrong base hides a read from every genome, and the 3'\n"
            "end of the second mate is where they are.  The insert and the cuts are found on the reads as they came; trimming, --deplete,\n"
            "the classification, --scores, POS and NEG records see the corrected bases and qualities.  A read without qualities (FASTA, or\n"
            "a quality line of another length) is never corrected.  Refused where --mate-overlap is.  PREPROCESS.tsv then also holds\n"
            "corrected_fragments, corrected_bases, correct_unresolved (disagreements left), correct_no_quality (fragments with\n"
            "disagreements but without qualities), mate_correct_quality and mate_correct_low\n"
            "--deplete <DIR> [--deplete <DIR2> ..] [--deplete-threshold <T>]: reads of the host, of PhiX and of the lab's usual\n"
            "contaminants are thrown away before anything is counted: every DIR is a database (a screen), and behind the steps above every\n"
            "read that hits a genome of a screen at T (default: the run's -f) is taken out on the GPU before the classification, which so\n"
            "sees what query -d DIR --neg-filter would have left, without writing and parsing it.  Up to 4 screens, applied in the order\n"
            "given (a DIR must not hold a ','); a screen has its own k, filter size and seeds; a read shorter than a screen's k hits all of\n"
            "its genomes, as everywhere, and goes.  With --reads2 / --interleaved a fragment goes when either mate hits.  Every replica\n"
            "(--devices) opens its own copy of every screen next to the database: the screens' memory is spent once per replica.  Turns the\n"
            "preprocessing above on (--min-length defaults to the database's k), combines with every option of it, and is refused where\n"
            "it is, and with --device-output.  Every output is, byte for byte, that of the same command without the option on an input\n"
            "that holds only the remaining records, each cut to what preprocessing kept.  PREPROCESS.tsv then also holds, per screen in\n"
            "order, deplete_db, deplete_threshold, depleted_units, depleted_reads and depleted_bases, and DEPLETION.csv in --out (several\n"
            "screens: DEPLETION_1.csv, DEPLETION_2.csv ..) is the CLASSIFICATION.csv of the reads a screen saw against that screen\n"
            "taxonomy -d <DB> --taxonomy <FILE> -o <OUT>: checks FILE against DB's tree.bin without a GPU and writes OUT/TAXA.tsv,\n"
            "\"#node<TAB>parent<TAB>depth<TAB>kind<TAB>genomes<TAB>name\", every node of the table query --taxonomy would count on\n"
            "ingest-check takes --reads2 / --interleaved too and prints the fragments' records, mates adjacent\n"
            "compare -d <DB> -o <OUT> [--against <DB2>] [--min-containment <C>] [--device <N>]: a phage database is full of strains and\n"
            "near-duplicates; this says which of its genomes are related.  For two genomes' filters the set bits and the shared set bits\n"
            "(counted on the GPU, all pairs at once) estimate how many k-mers each genome has and how many they share.  SIMILARITY.tsv in\n"
            "--out (an existing directory is replaced, as by query):\n\"%s\"\n"
            "(<TAB> between the columns), one line per pair: without --against the pairs a < b of the database in CLASSIFICATION.csv's order,\n"
            "with --against every (genome of DB, genome of DB2); the two databases must share k, filter size, hashes and seeds (build\n"
            "--seed1 / --seed2).  bits: set bits of the filters; kmers: each genome's distinct k-mers estimated from its filter's fill;\n"
            "shared_kmers: those both have; jaccard = shared / union; containment_a = shared_kmers / kmers_a, the share of a's k-mers that b\n"
            "has; ani = 1 + ln(2 J / (1 + J)) / k, the Mash distance turned round (0 where jaccard is 0).  Only pairs whose larger containment\n"
            "is at least C are written (default 0.1; --min-containment 0 writes all), ordered by a, then b\n"
            "recluster -d <DB> -o <NEWDB> [--merges <FILE>] [--device <N>]: build and add place a genome by the order it arrives in, and\n"
            "nothing ever moves.  This writes NEWDB (not DB itself) with the same genomes and the same filters under a tree rebuilt from\n"
            "the filters alone: average-linkage clustering of the genomes' chance-corrected similarities, on the GPU, so that strains\n"
            "sit under one node (--lca, --search-depth and large databases rely on that).  query gives the same genomes for every read\n"
            "on both.  --merges writes the dendrogram, one line per internal node in the order they were made:\n\"%s\"\n"
            "(<TAB> between the columns; similarity = score_sum / (pairs * 2^20), from 0 to 1: cut the tree where it drops).  Up to 16384\n"
            "genomes.  build --cluster: build, then recluster, in one run; the database equals that of the two commands byte for byte\n",
            header_cols.c_str(), merges_cols.c_str());
    if (asked)
        fprintf(stderr,
            "--gzip-output (needs --pos-filter and / or --neg-filter): the POS / NEG files are written as blocked gzip (BGZF, what bgzip\n"
            "writes): POS_FILTERING.fq.gz and so on, each ending with the 28-byte end marker.  zcat of each file is, byte for byte, the file\n"
            "the same command writes without the option; every other output is unchanged.  Under --device-output the GPU deflates the\n"
            "records it formats, where they lie; everything else is deflated by the host threads with zlib.  Where the members begin\n"
            "may depend on -t, -b and --devices; the text does not.  --gzip-level <1..9> (default 6) is zlib's level for the members the\n"
            "host makes: the GPU's deflate has no levels.  --device-parse --device-inflate reads such files back on the GPU\n");
}

}  // namespace

int main(int argc, char **argv) {
    // global -v/-q may precede the subcommand (clap-verbosity-flag, main.rs:49-50)
    int first = 1;
    while (first < argc && argv[first][0] == '-' && strcmp(argv[first], "--help") != 0 && strcmp(argv[first], "-h") != 0) ++first;
    if (first >= argc) {
        usage();
        return 2;
    }
    std::string cmd = argv[first];
    // shift so the subcommand sits at argv[1]
    std::vector<char *> av{argv[0], argv[first]};
    for (int i = 1; i < argc; ++i)
        if (i != first) av.push_back(argv[i]);
    if (cmd == "query") return cmd_query((int)av.size(), av.data());
    if (cmd == "build-balanced") return cmd_build_balanced((int)av.size(), av.data());
    if (cmd == "ingest-check") return cmd_ingest_check((int)av.size(), av.data());
    if (cmd == "build") return cmd_build((int)av.size(), av.data());
    if (cmd == "add") return cmd_add((int)av.size(), av.data());
    if (cmd == "compare") return cmd_compare((int)av.size(), av.data());
    if (cmd == "recluster") return cmd_recluster((int)av.size(), av.data());
    if (cmd == "taxonomy") return cmd_taxonomy((int)av.size(), av.data());
    if (cmd == "bgzf") return cmd_bgzf((int)av.size(), av.data());
    usage(cmd == "--help" || cmd == "-h");
    return 2;
}
