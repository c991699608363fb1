"""The adapter step (pfq.h "adapters") restated plainly, one position at a time, then read preprocessing (prep_ref) on the cut
reads with the totals of the original ones.  The device kernel, the CLI and the tests' expectations are compared with this file."""
from typing import Optional, Sequence, Tuple

import prep_ref

NO_ADAPTER = 0xFF
ADAPTER_MAX = 8


def matches(s: bytes, p: int, adapter: bytes, O: int, E: int) -> bool:
    """Does `adapter` match the read at position p < len(s)?"""
    o = min(len(adapter), len(s) - p)
    if o < O:
        return False
    mm = 0
    for i in range(o):
        if prep_ref.up(s[p + i]) != adapter[i]:
            mm += 1
            if 100 * mm > E * o:                                      # (mm only grows: the answer is known)
                return False
    return True


def find_cut(s: bytes, adapters: Sequence[bytes], O: int, E: int) -> Tuple[int, int]:
    """(cut, which): the smallest matching position and the lowest adapter that matches there; (len(s), 0xff) if none."""
    adapters = [a.upper() for a in adapters]
    for p in range(len(s)):
        for i, a in enumerate(adapters):
            if matches(s, p, a, O, E):
                return p, i
    return len(s), NO_ADAPTER


def prep_block(reads: Sequence[bytes], quals: Optional[Sequence[Optional[bytes]]], set1: Sequence[bytes], set2: Sequence[bytes] = (), O: int = 5,
               E: int = 10, paired: bool = False, **params) -> dict:
    """prep_ref.prep_block of the cut reads, with begin / len relative to the original reads (they are: a cut only removes a
    suffix), bases_in and n_trimmed by the original lengths, and what the adapter step itself reports."""
    n = len(reads)
    memo = {}
    cut, which = [], []
    for i, s in enumerate(reads):
        second = paired and i % 2 == 1 and len(set2) > 0
        key = (s, second)
        if key not in memo:
            memo[key] = find_cut(s, set2 if second else set1, O, E)
        cut.append(memo[key][0])
        which.append(memo[key][1])
    cut_reads = [s[:c] for s, c in zip(reads, cut)]
    cut_quals = None if quals is None else [None if q is None else q[:c] for q, c in zip(quals, cut)]
    res = prep_ref.prep_block(cut_reads, cut_quals, paired=paired, **params)
    res["bases_in"] = sum(map(len, reads))
    res["n_trimmed"] = sum(1 for i in res["kept"] if res["len"][i] < len(reads[i]))
    found = [0] * (2 * ADAPTER_MAX)
    for i in range(n):
        if which[i] != NO_ADAPTER:
            found[which[i] + (ADAPTER_MAX if paired and i % 2 == 1 and len(set2) > 0 else 0)] += 1
    res.update(cut=cut, which=which, cut_reads=cut_reads, cut_quals=cut_quals, n_found=sum(1 for s, c in zip(reads, cut) if c < len(s)),
               bases_cut=sum(len(s) - c for s, c in zip(reads, cut)), found=found)
    return res
