"""pfq_query_frames restated in plain Python (include/pfq.h "frames and segments"): the frame starts, the per-frame leaf sets
from the oracle's query_batch, the segments with their k-mer-resolution fields from get_kmers / bf_contains, and the sequence
counts.  Nothing here knows how the library computes any of it."""
from oracle import pfq_oracle as orc

FIELDS = ("leaf", "first_frame", "n_frames", "begin", "end", "match_begin", "match_end", "kmers", "matched", "longest_run")


def frame_starts(L, F, S):
    """(start, length) of every frame of a sequence of L bases."""
    if L <= F:
        return [(0, L)]
    n = -(-(L - F) // S) + 1
    return [(min(j * S, L - F), F) for j in range(n)]


def run_fields(mask):
    """(matched, first, last, longest_run) of a list of booleans; first / last are None without a match."""
    hits = [p for p, m in enumerate(mask) if m]
    best = cur = 0
    for m in mask:
        cur = cur + 1 if m else 0
        best = max(best, cur)
    return len(hits), (hits[0] if hits else None), (hits[-1] if hits else None), best


def part(mask):
    """The partial result of a stretch of positions: (len, matched, first, last, prefix_run, suffix_run, best_run)."""
    matched, first, last, best = run_fields(mask)
    pre = next((p for p, m in enumerate(mask) if not m), len(mask))
    suf = next((p for p, m in enumerate(reversed(mask)) if not m), len(mask))
    return (len(mask), matched, first, last, pre, suf, best)


def join(a, b):
    """The partial result of stretch a followed by stretch b."""
    alen, am, af, al, apre, asuf, abest = a
    blen, bm, bf, bl, bpre, bsuf, bbest = b
    return (alen + blen, am + bm,
            af if am else (alen + bf if bm else None),
            alen + bl if bm else al,
            alen + bpre if apre == alen else apre,
            blen + asuf if bsuf == blen else bsuf,
            max(abest, bbest, asuf + bpre))


def frame_sets(ot, seqs, F, S, thr):
    """Per sequence the list of its frames' leaf-column sets: every frame classified as a read of its own."""
    frames, owner = [], []
    for i, x in enumerate(seqs):
        for s, n in frame_starts(len(x), F, S):
            frames.append(x[s:s + n])
            owner.append(i)
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    ohits, _, _ = orc.query_batch(ot, frames, thr, threads=8)
    for v in range(ot.n_nodes):
        ot.mapped_reads[v] = 0
    col = {v: c for c, v in enumerate(ot.leaves_dfs())}
    sets = [set() for _ in frames]
    for r, v in ohits:
        sets[r].add(col[v])
    out = [[] for _ in seqs]
    for i, s in zip(owner, sets):
        out[i].append(s)
    return out


class Ref:
    """Segments of sequences against an oracle tree; the oracle's answers per (leaf, k-mer) are kept."""

    def __init__(self, ot):
        self.ot = ot
        self.rows = [ot.filter_of[v] for v in ot.leaves_dfs()]
        self._in = {}

    def contains(self, leaf, kmer):
        key = (leaf, kmer)
        if key not in self._in:
            self._in[key] = orc.bf_contains(self.ot, self.rows[leaf], kmer)
        return self._in[key]

    def mask(self, x, leaf, begin, end):
        return [self.contains(leaf, c) for c in orc.get_kmers(x[begin:end], self.ot.kmer_size)]

    def segments_of(self, x, sets, F, S):
        """The segments of one sequence x whose frames have the leaf sets `sets`: dicts with FIELDS, in ABI order."""
        k, fr, segs = self.ot.kmer_size, frame_starts(len(x), F, S), []
        assert len(fr) == len(sets)
        for j0, h in enumerate(sets):
            for l in sorted(h):
                if j0 and l in sets[j0 - 1]:
                    continue
                j1 = j0
                while j1 + 1 < len(sets) and l in sets[j1 + 1]:
                    j1 += 1
                begin, end = fr[j0][0], fr[j1][0] + fr[j1][1]
                mask = self.mask(x, l, begin, end)
                assert len(mask) == max(end - begin - k + 1, 0)
                matched, first, last, best = run_fields(mask)
                segs.append(dict(leaf=l, first_frame=j0, n_frames=j1 - j0 + 1, begin=begin, end=end,
                                 match_begin=begin + first if matched else begin, match_end=begin + last + k if matched else begin,
                                 kmers=len(mask), matched=matched, longest_run=best))
        return segs

    def query(self, seqs, F, S, thr):
        """(per-sequence segment lists, frames in all, the leaf counters' increase) of one call."""
        all_sets = frame_sets(self.ot, seqs, F, S, thr)
        per_seq = [self.segments_of(x, sets, F, S) for x, sets in zip(seqs, all_sets)]
        counts = [0] * len(self.rows)
        for segs in per_seq:
            for l in {s["leaf"] for s in segs}:
                counts[l] += 1
        return per_seq, sum(len(s) for s in all_sets), counts, all_sets


def as_tuples(segs):
    return [tuple(int(s[f]) for f in FIELDS) for s in segs]
