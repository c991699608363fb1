"""Depletion (pfq.h "depletion") restated plainly on top of the CPU oracle: the kept, trimmed reads of tests/prep_ref.py are
classified against the screen's OracleTree by oracle.pfq_oracle.query_batch, one read on its own; a unit (a read, or with
`paired` two consecutive reads) is removed iff its row — the read's leaf set, the union ("either") or the intersection (`both`)
of its mates' — is not empty.  A read without a k-mer of the screen passes every leaf by the classifier's own rule.  The device
call, the CLI and the tests' expectations are compared with this file; it never asks the device classifier."""
from typing import List, Optional, Sequence

from oracle import pfq_oracle as orc

DEPLETED = 5


def leaf_sets(screen, reads: Sequence[bytes], threshold: float) -> List[set]:
    """Per read its leaf columns on the screen (DFS order); the oracle's node counters are left as they were.  Equal reads are
    asked once."""
    distinct = sorted(set(reads))
    at = {r: i for i, r in enumerate(distinct)}
    saved = list(screen.mapped_reads)
    hits, _, _ = orc.query_batch(screen, distinct, threshold) if distinct else ([], 0, 0.0)
    screen.mapped_reads[:] = saved
    col = {v: i for i, v in enumerate(screen.leaves_dfs())}
    sets = [set() for _ in distinct]
    for r, v in hits:
        sets[r].add(col[v])
    return [sets[at[r]] for r in reads]


def deplete(kept_reads: Sequence[bytes], screen, threshold: float, paired: bool = False, both: bool = False,
            kept: Optional[Sequence[int]] = None, reason: Optional[Sequence[int]] = None) -> dict:
    """kept_reads: the prepared block (prep_ref.prep_block's "kept_reads", or an earlier call's "survivors"); kept / reason: the
    indices of those reads in the block given to the prep and that block's reasons (None: the reads number themselves and all
    were kept).  Returns removed (a flag per unit), rows (the units' leaf sets), survivors, kept, reason, the totals of the call
    and leaf_counts: what the call adds to the screen's leaf counters, by leaf column."""
    n = len(kept_reads)
    per = 2 if paired else 1
    assert n % per == 0 and (both <= paired)
    kept = list(range(n)) if kept is None else list(kept)
    reason = [0] * n if reason is None else list(reason)
    assert len(kept) == n
    sets = leaf_sets(screen, kept_reads, threshold)
    if paired:
        rows = [sets[2 * u] & sets[2 * u + 1] if both else sets[2 * u] | sets[2 * u + 1] for u in range(n // 2)]
    else:
        rows = sets
    removed = [bool(row) for row in rows]
    n_leaves = len(screen.leaves_dfs())
    leaf_counts = [0] * n_leaves
    for row in rows:
        for c in row:
            leaf_counts[c] += 1
    stay = [i for i in range(n) if not removed[i // per]]
    for i in range(n):
        if removed[i // per]:
            reason[kept[i]] = DEPLETED
    survivors = [kept_reads[i] for i in stay]
    return {"removed": removed, "rows": rows, "survivors": survivors, "kept": [kept[i] for i in stay], "reason": reason,
            "n_units": n // per, "units_removed": sum(removed), "reads_removed": n - len(stay),
            "bases_removed": sum(len(kept_reads[i]) for i in range(n) if removed[i // per]),
            "n_kept": len(stay), "bases_kept": sum(map(len, survivors)), "leaf_counts": leaf_counts}


TOTALS = ("n_units", "units_removed", "reads_removed", "bases_removed", "n_kept", "bases_kept")
