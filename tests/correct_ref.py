"""The mate correction (pfq.h "mate correction") restated plainly, one pair of one hypothesis at a time, on top of
overlap_ref.find_insert; then read preprocessing on the corrected mates with the overlap and adapter results of the original
ones.  The device kernels, the CLI and the tests' expectations are compared with this file."""
from typing import List, Optional, Sequence, Tuple

import overlap_ref
import prep_ref

COMP = overlap_ref.COMP
TOTALS = ("n_fragments_corrected", "n_bases", "n_unresolved", "n_no_quality")
HIGH, LOW = 30, 14


def phred(q: int) -> int:
    return max(q - 33, 0)


def correct_fragment(a: bytes, b: bytes, q1: Optional[bytes], q2: Optional[bytes], O: int, E: int, high: int = HIGH, low: int = LOW):
    """(a, b, q1, q2 corrected, patches [(mate, pos, base, qual, old_base, old_qual)] ascending by (mate, pos), unresolved pairs,
    no_quality: the fragment had an insert with mismatches but a mate without qualities)."""
    analysed, I, mm, _, _ = overlap_ref.fragment(a, b, O, E)
    if not analysed or I == overlap_ref.NO_INSERT or mm == 0:
        return a, b, q1, q2, [], 0, False
    if q1 is None or q2 is None:
        return a, b, q1, q2, [], 0, True
    L1, L2 = len(a), len(b)
    na, nb, nq1, nq2 = bytearray(a), bytearray(b), bytearray(q1), bytearray(q2)
    patches, unresolved = [], 0
    for i in range(max(0, I - L2), min(I, L1)):
        j = I - 1 - i
        ua, ub = prep_ref.up(a[i]), prep_ref.up(b[j])
        if ua in COMP and ub in COMP and ua == COMP[ub]:
            continue                                                  # not a pair that mm(I) counts
        p1, p2 = phred(q1[i]), phred(q2[j])
        if ua in COMP and p1 >= high and p2 <= low:
            nb[j], nq2[j] = COMP[ua], q1[i]
            patches.append((1, j, COMP[ua], q1[i], b[j], q2[j]))
        elif ub in COMP and p2 >= high and p1 <= low:
            na[i], nq1[i] = COMP[ub], q2[j]
            patches.append((0, i, COMP[ub], q2[j], a[i], q1[i]))
        else:
            unresolved += 1
    return bytes(na), bytes(nb), bytes(nq1), bytes(nq2), sorted(patches), unresolved, False


def correct_block(reads: Sequence[bytes], quals: Optional[Sequence[Optional[bytes]]], O: int, E: int, high: int = HIGH, low: int = LOW) -> dict:
    """The corrected reads and quals of a paired block, the patch list [(read, pos, base, qual, old_base, old_qual)] ascending by
    (read, pos) and the totals."""
    n = len(reads)
    assert n % 2 == 0
    out_reads: List[bytes] = []
    out_quals: List[Optional[bytes]] = []
    patches: List[Tuple[int, int, int, int, int, int]] = []
    tot = {"n_fragments_corrected": 0, "n_bases": [0, 0], "n_unresolved": 0, "n_no_quality": 0}
    memo = {}
    for f in range(n // 2):
        key = (reads[2 * f], reads[2 * f + 1], None if quals is None else quals[2 * f], None if quals is None else quals[2 * f + 1])
        if key not in memo:
            memo[key] = correct_fragment(*key, O, E, high, low)
        a, b, q1, q2, pt, unresolved, no_quality = memo[key]
        out_reads += [a, b]
        out_quals += [q1, q2]
        patches += [(2 * f + m, pos, base, qual, ob, oq) for m, pos, base, qual, ob, oq in pt]
        tot["n_fragments_corrected"] += 1 if pt else 0
        for m in (0, 1):
            tot["n_bases"][m] += sum(1 for x in pt if x[0] == m)
        tot["n_unresolved"] += unresolved
        tot["n_no_quality"] += 1 if no_quality else 0
    res = dict(tot)
    res.update(reads=out_reads, quals=None if quals is None else out_quals, patches=patches)
    return res


def apply_patches(reads: Sequence[bytes], quals: Sequence[Optional[bytes]], patches) -> Tuple[List[bytes], List[Optional[bytes]]]:
    """What a caller that holds the original records does with the patch list."""
    rs = [bytearray(s) for s in reads]
    qs = [None if q is None else bytearray(q) for q in quals]
    for read, pos, base, qual, old_base, old_qual in patches:
        assert rs[read][pos] == old_base and qs[read][pos] == old_qual
        rs[read][pos], qs[read][pos] = base, qual
    return [bytes(s) for s in rs], [None if q is None else bytes(q) for q in qs]


def prep_block(reads: Sequence[bytes], quals: Optional[Sequence[Optional[bytes]]], O: int, E: int, high: int = HIGH, low: int = LOW, set1: Sequence[bytes] = (),
               set2: Sequence[bytes] = (), adapter_O: int = 5, adapter_E: int = 10, **params) -> dict:
    """A paired block with the correction: what overlap_ref.prep_block reports of the overlap and adapter steps on the original
    mates, and prep_ref.prep_block of the corrected mates cut at the original min(adapter cut, ocut); under "corrections" the
    result of correct_block."""
    orig = overlap_ref.prep_block(reads, quals, O, E, set1, set2, adapter_O, adapter_E, **params)
    cor = correct_block(reads, quals, O, E, high, low)
    cut = orig["cut"]
    cut_reads = [s[:c] for s, c in zip(cor["reads"], cut)]
    cut_quals = None if quals is None else [None if q is None else q[:c] for q, c in zip(cor["quals"], cut)]
    res = prep_ref.prep_block(cut_reads, cut_quals, paired=True, **params)
    res["bases_in"] = sum(map(len, reads))
    res["n_trimmed"] = sum(1 for i in res["kept"] if res["len"][i] < len(reads[i]))
    for k in (*overlap_ref.TOTALS, "insert", "mismatches", "ocut", "cut", "hist", "adapters"):
        res[k] = orig[k]
    res.update(cut_reads=cut_reads, cut_quals=cut_quals, corrections=cor)
    return res
