"""Read preprocessing (pfq.h "read preprocessing") restated plainly: one read at a time, no cleverness, then the pair rule and
the totals.  The device kernels, the CLI and the tests' expectations are all compared with this file."""
from typing import List, Optional, Sequence, Tuple

KEPT, SHORT, N, COMPLEXITY, MATE = 0, 1, 2, 3, 4
REASONS = ("kept", "short", "n", "complexity", "mate")
ACGT = frozenset(b"ACGT")


def up(c: int) -> int:
    return c & 0xDF


def trim_read(s: bytes, q: Optional[bytes], trim_quality: int = 0, trim_window: int = 4, poly_x: int = 0) -> Tuple[int, int]:
    """Steps 1 - 3: the kept interval as (begin, len); an empty one is (0, 0)."""
    L = len(s)
    b, e = 0, L
    if trim_quality > 0 and q is not None:
        assert len(q) == L
        p = [max(x - 33, 0) for x in q]
        good = [j for j in range(L) if p[j] >= trim_quality]
        if not good:
            return 0, 0
        b = good[0]
        w = min(trim_window, L - b)
        e = L
        for i in range(b, L - w + 1):
            if sum(p[i:i + w]) < trim_quality * w:
                e = i
                break
        good = [j for j in range(b, e) if p[j] >= trim_quality]
        if not good:
            return 0, 0
        e = good[-1] + 1
    if poly_x > 0 and e > b:
        c = up(s[e - 1])
        r = 0
        while e - 1 - r >= b and up(s[e - 1 - r]) == c:
            r += 1
        if r >= poly_x:
            e -= r
    return (b, e - b) if e > b else (0, 0)


def reason_of(s: bytes, begin: int, length: int, min_length: int = 0, max_n: Optional[int] = None, min_complexity: int = 0) -> int:
    """Step 4 on the kept interval."""
    kept = s[begin:begin + length]
    if length < min_length:
        return SHORT
    if max_n is not None and sum(1 for c in kept if up(c) not in ACGT) > max_n:
        return N
    if min_complexity > 0:
        d = sum(1 for j in range(length - 1) if up(kept[j]) != up(kept[j + 1]))
        if 100 * d < min_complexity * max(length - 1, 0):
            return COMPLEXITY
    return KEPT


def prep_read(s: bytes, q: Optional[bytes], trim_quality: int = 0, trim_window: int = 4, poly_x: int = 0, min_length: int = 0,
              max_n: Optional[int] = None, min_complexity: int = 0) -> Tuple[int, int, int]:
    """(begin, len, reason) of one read, before the pair rule."""
    begin, length = trim_read(s, q, trim_quality, trim_window, poly_x)
    return begin, length, reason_of(s, begin, length, min_length, max_n, min_complexity)


def prep_block(reads: Sequence[bytes], quals: Optional[Sequence[Optional[bytes]]] = None, paired: bool = False, **params) -> dict:
    """A block of reads: quals[i] None = read i has no qualities.  The per-read results, the pair rule, the totals and the kept,
    trimmed reads — what the device call reports and what its CSR holds.  Equal (read, quality) inputs are worked out once."""
    n = len(reads)
    if paired:
        assert n % 2 == 0
    memo = {}
    begin, length, reason = [], [], []
    for i in range(n):
        key = (reads[i], None if quals is None else quals[i])
        if key not in memo:
            memo[key] = prep_read(key[0], key[1], **params)
        b, l, why = memo[key]
        begin.append(b)
        length.append(l)
        reason.append(why)
    if paired:
        for i in range(0, n, 2):
            if (reason[i] != KEPT) != (reason[i + 1] != KEPT):
                reason[i if reason[i] == KEPT else i + 1] = MATE
    kept = [i for i in range(n) if reason[i] == KEPT]
    kept_reads = [reads[i][begin[i]:begin[i] + length[i]] for i in kept]
    return {"n_reads": n, "n_kept": len(kept), "bases_in": sum(map(len, reads)), "bases_kept": sum(map(len, kept_reads)),
            "n_trimmed": sum(1 for i in kept if length[i] < len(reads[i])),
            "n_reason": {name: sum(1 for why in reason if why == c) for c, name in enumerate(REASONS)},
            "begin": begin, "len": length, "reason": reason, "kept": kept, "kept_reads": kept_reads}


def add_totals(parts: List[dict]) -> dict:
    out = {k: sum(p[k] for p in parts) for k in ("n_reads", "n_kept", "bases_in", "bases_kept", "n_trimmed")}
    out["n_reason"] = {name: sum(p["n_reason"][name] for p in parts) for name in REASONS}
    return out
