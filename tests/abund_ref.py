"""Plain-Python restatement of the abundance estimate (include/pfq.h, "abundance"): Python ints only, no library.

A log is built from hit rows (one ascending list of leaf indices per unit) with `classify`, and `estimate` runs the integer EM
over it.  The result is a function of the multiset of rows; `estimate` sorts nothing and needs no order."""
from collections import Counter

Q = 16
ONE = 1 << Q


def classify(rows, n_leaves, mult=None):
    """The log the library keeps for these rows: class counters, unique[], and the ambiguous rows as a Counter of tuples
    (identical rows add the same terms, so they are folded here; the library keeps them one by one).  `mult`: per row, how
    many units have it (one each without)."""
    log = {"n_leaves": n_leaves, "n_units": 0, "n_unhit": 0, "n_unique": 0, "n_ambiguous": 0, "n_all_leaves": 0, "n_entries": 0,
           "unique": [0] * n_leaves, "rows": Counter()}
    add(log, rows, mult)
    return log


def add(log, rows, mult=None):
    L = log["n_leaves"]
    for i, r in enumerate(rows):
        r = tuple(int(x) for x in r)
        m = 1 if mult is None else int(mult[i])
        log["n_units"] += m
        if len(r) == 0:
            log["n_unhit"] += m
        elif len(r) == 1:                      # (so a tree of one leaf has no "all leaves" class)
            log["n_unique"] += m
            log["unique"][r[0]] += m
        elif len(r) == L:
            log["n_all_leaves"] += m
        else:
            log["n_ambiguous"] += m
            log["n_entries"] += m * len(r)
            log["rows"][r] += m
    return log


def estimate(log, max_iters=200, tol=65, start=None):
    """dict like BloomTree.abundance(): mass, unique (lists of ints), the counters, iterations, converged, last_delta.
    `start`: another a[] than the uniform 1 << 16 (tests of the D == 0 rule only)."""
    assert max_iters >= 1
    L = log["n_leaves"]
    out = {k: log[k] for k in ("n_units", "n_unhit", "n_unique", "n_ambiguous", "n_all_leaves", "n_entries")}
    out["unique"] = list(log["unique"])
    if log["n_units"] == 0:                    # nothing logged: nothing to iterate
        out.update(mass=[0] * L, iterations=1, converged=1, last_delta=0)
        return out
    a = list(start) if start is not None else [ONE] * L
    it, delta, converged = 0, 0, False
    while it < max_iters and not converged:
        new = [u << Q for u in log["unique"]]
        for r, mult in log["rows"].items():
            D = sum(a[l] for l in r)
            if D > 0:
                for l in r:
                    new[l] += mult * ((a[l] << Q) // D)
        delta = max((abs(x - y) for x, y in zip(new, a)), default=0)
        a = new
        it += 1
        converged = delta <= tol
    out.update(mass=a, iterations=it, converged=int(converged), last_delta=delta)
    return out


def tsv_lines(est, names):
    """ABUNDANCE.tsv as the CLI writes it, without the two header lines: (genome, unique, estimated, fraction) per leaf with
    mass > 0; unique and estimated as strings, fraction as a float."""
    total = sum(est["mass"])
    out = []
    for l, m in enumerate(est["mass"]):
        if m:
            milli = (m * 1000 + 32768) >> 16
            out.append((names[l], str(est["unique"][l]), f"{milli // 1000}.{milli % 1000:03d}", m / total))
    return out
