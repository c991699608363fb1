"""The threshold sweep (include/pfq.h "threshold sweep") in plain Python: what the flagged calls must leave in the library's
counters, from the units' rows, the rows' scores, the reads' lengths, k and the list of thresholds.  Nothing here knows the
library; need() is the oracle's."""
import numpy as np

from oracle import pfq_oracle as orc


def needs(thresholds, length, k):
    """need_t for a read of `length` bases: the oracle's need() of every (f32) threshold and the read's k-mers."""
    n = max(length - k + 1, 0)
    return [orc.need(float(np.float32(t)), n) for t in thresholds]


def passed(score, need):
    """p(e): the thresholds of the ascending list whose need the score reaches."""
    return sum(1 for x in need if score >= x)


def unit(row, scores, need):
    """(p per entry, top, arg, second) of one unit: `row` its leaves in ascending order, `scores` aligned with it."""
    p = [passed(int(s), need) for s in scores]
    if not p:
        return p, 0, None, 0
    top = max(p)
    arg = row[p.index(top)]
    rest = sorted(p, reverse=True)
    return p, top, arg, (rest[1] if len(rest) > 1 else 0)


def derived_rows(row, scores, need):
    """The unit's row at every threshold of the list: the entries with p > t."""
    p = [passed(int(s), need) for s in scores]
    return [{l for l, x in zip(row, p) if x > t} for t in range(len(need))]


def sweep(rows, scores, lengths, k, thresholds, n_leaves, mult=None):
    """The state and the read-out after the units `rows` (per unit its leaves, ascending; `scores` flat, aligned with the rows
    one after the other; `lengths` the reads' lengths).  mult: unit i counts mult[i] times.  Also `top` and `second` per unit."""
    T, L = len(thresholds), n_leaves
    pas = np.zeros((T + 1, L), dtype=np.uint64)
    uniq = np.zeros((T, L), dtype=np.uint64)
    tops = np.zeros(T + 1, dtype=np.uint64)
    top_of, second_of = [], []
    need_memo, j, n_units = {}, 0, 0
    for i, row in enumerate(rows):
        m = np.uint64(1 if mult is None else int(mult[i]))
        if lengths[i] not in need_memo:
            need_memo[lengths[i]] = needs(thresholds, lengths[i], k)
        p, top, arg, second = unit(row, scores[j:j + len(row)], need_memo[lengths[i]])
        j += len(row)
        for l, x in zip(row, p):
            pas[x, l] += m
        tops[top] += m
        for t in range(second, top):
            uniq[t, arg] += m
        n_units += int(m)
        top_of.append(top)
        second_of.append(second)
    assert j == len(scores)
    out = {"pass": pas, "uniq": uniq, "tops": tops, "n_units": n_units, "n_leaves": L,
           "thresholds": np.array(thresholds, dtype=np.float32), "top": np.array(top_of), "second": np.array(second_of)}
    out.update(read_out(pas, uniq, tops))
    return out


def read_out(pas, uniq, tops):
    """The derived arrays, in integers."""
    T = len(uniq)
    above = np.cumsum(pas[::-1], axis=0, dtype=np.uint64)[::-1]      # above[p] = sum of pass[p ..]
    leaf_units = above[1:T + 1]
    tops_above = np.cumsum(tops[::-1], dtype=np.uint64)[::-1]
    return {"leaf_units": leaf_units, "leaf_unique": uniq.copy(), "units_hit": tops_above[1:T + 1],
            "units_unique": uniq.sum(axis=1, dtype=np.uint64), "entries": leaf_units.sum(axis=1, dtype=np.uint64),
            "genomes_hit": (leaf_units > 0).sum(axis=1).astype(np.uint64)}


def absorb(a, b):
    """Two replicas' states: a plain sum."""
    assert np.array_equal(a["thresholds"], b["thresholds"]) and a["n_leaves"] == b["n_leaves"]
    out = {k: a[k] + b[k] for k in ("pass", "uniq", "tops", "n_units")}
    out.update(n_leaves=a["n_leaves"], thresholds=a["thresholds"])
    out.update(read_out(out["pass"], out["uniq"], out["tops"]))
    return out


READ_OUT = ("leaf_units", "leaf_unique", "units_hit", "units_unique", "entries", "genomes_hit")


def same(got, want, tag=None):
    """tree.sweep() against a reference state: every array exactly."""
    assert got["n_units"] == want["n_units"] and got["n_leaves"] == want["n_leaves"], (tag, got["n_units"], want["n_units"])
    assert got["thresholds"].dtype == np.float32 and np.array_equal(got["thresholds"], want["thresholds"]), tag
    for k in READ_OUT:
        assert got[k].dtype == np.uint64 and got[k].shape == want[k].shape, (tag, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (tag, k, np.argwhere(got[k] != want[k])[:10])
