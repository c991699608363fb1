"""The mate overlap step (pfq.h "mate overlap") restated plainly, one hypothesis and one pair of bases at a time, then read
preprocessing (prep_ref, adapter_ref) on the cut mates with the totals of the original ones.  The device kernel, the CLI and the
tests' expectations are compared with this file."""
from typing import Optional, Sequence, Tuple

import adapter_ref
import prep_ref

NO_INSERT = 0xFFFFFFFF
LEN_MAX = 512
INSERT_MAX = 1024
COMP = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}
TOTALS = ("n_fragments", "n_analysed", "n_skipped", "n_overlapped", "n_readthrough", "reads_cut", "bases_cut")


def find_insert(a: bytes, b: bytes, O: int, E: int) -> Tuple[int, int]:
    """(insert, mismatches): the largest matching I in [O, L1 + L2 - O]; (NO_INSERT, 0) if none matches."""
    L1, L2 = len(a), len(b)
    x = [prep_ref.up(c) if prep_ref.up(c) in COMP else -1 for c in a]           # -1, -2: outside ACGT, equal to nothing
    y = [COMP.get(prep_ref.up(c), -2) for c in b]                     # comp(up(b[j]))
    for I in range(L1 + L2 - O, O - 1, -1):
        lo, hi = max(0, I - L2), min(I, L1)
        o = hi - lo
        if o < O:
            continue
        mm = 0
        for i in range(lo, hi):
            if x[i] != y[I - 1 - i]:
                mm += 1
                if 100 * mm > E * o:                                  # (mm only grows: the answer is known)
                    break
        if 100 * mm <= E * o:
            return I, mm
    return NO_INSERT, 0


def fragment(a: bytes, b: bytes, O: int, E: int) -> Tuple[bool, int, int, int, int]:
    """(analysed, insert, mismatches, ocut of mate 1, ocut of mate 2)."""
    if len(a) > LEN_MAX or len(b) > LEN_MAX:
        return False, NO_INSERT, 0, len(a), len(b)
    insert, mm = find_insert(a, b, O, E)
    return True, insert, mm, min(len(a), insert), min(len(b), insert)


def prep_block(reads: Sequence[bytes], quals: Optional[Sequence[Optional[bytes]]], O: int, E: int, set1: Sequence[bytes] = (), set2: Sequence[bytes] = (),
               adapter_O: int = 5, adapter_E: int = 10, **params) -> dict:
    """A paired block: prep_ref.prep_block of the mates cut at min(adapter cut, ocut), with begin / len relative to the original
    reads, bases_in and n_trimmed by the original lengths, what the overlap step itself reports and, under "adapters", what
    the adapter step reports on its own (None without adapters)."""
    n = len(reads)
    assert n % 2 == 0
    memo = {}
    insert, mm, ocut = [], [], []
    tot = dict.fromkeys(TOTALS, 0)
    hist = [0] * (INSERT_MAX + 1)
    for f in range(n // 2):
        a, b = reads[2 * f], reads[2 * f + 1]
        if (a, b) not in memo:
            memo[(a, b)] = fragment(a, b, O, E)
        analysed, ins, m, c1, c2 = memo[(a, b)]
        insert.append(ins)
        mm.append(m)
        ocut += [c1, c2]
        tot["n_fragments"] += 1
        tot["n_analysed" if analysed else "n_skipped"] += 1
        if ins != NO_INSERT:
            tot["n_overlapped"] += 1
            tot["n_readthrough"] += 1 if ins < max(len(a), len(b)) else 0
            hist[ins] += 1
        tot["reads_cut"] += (c1 < len(a)) + (c2 < len(b))
        tot["bases_cut"] += len(a) - c1 + len(b) - c2
    adapters = adapter_ref.prep_block(reads, None, set1, set2, adapter_O, adapter_E, paired=True) if len(set1) else None
    cut = [min(c, adapters["cut"][i]) if adapters else c for i, c in enumerate(ocut)]
    cut_reads = [s[:c] for s, c in zip(reads, cut)]
    cut_quals = None if quals is None else [None if q is None else q[:c] for q, c in zip(quals, cut)]
    res = prep_ref.prep_block(cut_reads, cut_quals, paired=True, **params)
    res["bases_in"] = sum(map(len, reads))
    res["n_trimmed"] = sum(1 for i in res["kept"] if res["len"][i] < len(reads[i]))
    res.update(tot)
    res.update(insert=insert, mismatches=mm, ocut=ocut, cut=cut, hist=hist, cut_reads=cut_reads, cut_quals=cut_quals, adapters=adapters)
    return res
