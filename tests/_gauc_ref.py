"""Inputs and host references shared by the grouped-AUC tests (test_gauc_host.py, test_gpu_gauc.py).

Two independent references: ``ref_table`` is the kernels' integer formulation (exact Python-sized
integers per group), ``direct_auc`` is utils.compute_auc's float64 rank-sum arithmetic applied per
group, vectorised with lexsort.  The tests require them to agree bit for bit on every mixed group.
"""
import functools

import numpy as np

SCORES = ("uniform", "sevenths", "all_equal")
GROUPS = ("one", "singletons", "small", "wide", "skewed")
SIZES = (1, 2, 63, 64, 65, 4099, 70001)


def _labels(rng, n):
    y = (rng.random(n) < 0.17).astype(np.float32)
    if n >= 2:                     # about 17 % positives, both classes present
        y[0], y[-1] = 1.0, 0.0
    return y


def scores(family, n, seed=0):
    """(labels, probabilities): the score families of test_gpu_metrics.py."""
    rng = np.random.default_rng(1000 * seed + n)
    y = _labels(rng, n)
    if family == "uniform":
        p = rng.random(n, dtype=np.float32)
    elif family == "sevenths":
        p = (rng.integers(0, 7, n) / 6.0).astype(np.float32)
    elif family == "all_equal":
        p = np.full(n, 0.5, dtype=np.float32)
    else:
        raise AssertionError(family)
    return y, p


def group_ids(family, n, seed=0):
    """int64 ids in [0, 2^32)."""
    rng = np.random.default_rng(77 + 1000 * seed + n)
    if family == "one":
        return np.full(n, 7, dtype=np.int64)
    if family == "singletons":
        return (rng.permutation(n).astype(np.int64) * 3 + 1)
    if family == "small":
        return rng.integers(0, max(1, n // 8), n).astype(np.int64)
    if family == "wide":           # every byte of the id varies; the extremes of the range are present
        pool = rng.integers(0, 1 << 32, max(1, n // 16), dtype=np.uint64).astype(np.int64)
        special = np.array([0, 1 << 31, (1 << 32) - 1], dtype=np.int64)
        k = min(len(pool), 3)
        pool[:k] = special[:k]
        ids = pool[rng.integers(0, len(pool), n)]
        ids[:k] = pool[:k]          # each special id is drawn at least once
        return ids
    if family == "skewed":         # one group above 65 535 samples at n = 70 001, beside many small ones
        ids = rng.integers(0, max(1, n // 64), n).astype(np.int64)
        ids[rng.random(n) < 0.95] = 5
        return ids
    raise AssertionError(family)


def _sorted(y, p, ids):
    p = np.asarray(p, dtype=np.float32)
    bits = np.where(p == 0, 0, p.view(np.uint32)).astype(np.uint64)
    key = (bits << np.uint64(1)) | (np.asarray(y) == 1).astype(np.uint64)
    comp = (np.asarray(ids).astype(np.uint64) << np.uint64(31)) | key
    comp = np.sort(comp)
    gid = comp >> np.uint64(31)
    starts = np.flatnonzero(np.r_[True, gid[1:] != gid[:-1]]) if len(comp) else np.zeros(0, np.int64)
    return comp, gid, starts


def ref_table(y, p, ids):
    """{"group", "u2", "n_pos", "n_neg"} int64 arrays, ascending id: the integer formulation."""
    comp, gid, starts = _sorted(y, p, ids)
    n = len(comp)
    if n == 0:
        z = np.zeros(0, np.int64)
        return {"group": z, "u2": z, "n_pos": z, "n_neg": z}
    pos = (comp & np.uint64(1)).astype(np.int64)
    negs = np.r_[0, np.cumsum(1 - pos)]
    run = comp >> np.uint64(1)
    lower = np.searchsorted(run, run, side="left")
    upper = np.searchsorted(run, run, side="right")
    gstart = np.repeat(starts, np.diff(np.r_[starts, n]))
    contrib = pos * (2 * (negs[lower] - negs[gstart]) + (negs[upper] - negs[lower]))
    ends = np.r_[starts[1:], n]
    n_neg = negs[ends] - negs[starts]
    return {"group": gid[starts].astype(np.int64), "u2": np.add.reduceat(contrib, starts).astype(np.int64),
            "n_pos": (ends - starts - n_neg).astype(np.int64), "n_neg": n_neg.astype(np.int64)}


def direct_auc(y, p, ids):
    """(ids ascending, per-group AUC in float64; NaN for a single-class group): compute_auc's own
    arithmetic -- average ranks of ties, (rank sum of the positives - n_pos (n_pos + 1) / 2) /
    (n_pos n_neg) -- inside every group at once."""
    y = np.asarray(y, dtype=np.float64)
    s = np.asarray(p, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    n = len(y)
    order = np.lexsort((s, ids))
    ys, ss, gs = y[order], s[order], ids[order]
    starts = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
    ends = np.r_[starts[1:], n]
    gstart = np.repeat(starts, ends - starts)
    tie = np.flatnonzero(np.r_[True, (gs[1:] != gs[:-1]) | (ss[1:] != ss[:-1])])
    tie_end = np.r_[tie[1:], n]
    t_lo = np.repeat(tie, tie_end - tie) - gstart                 # 0-based position of the tie inside its group
    t_hi = np.repeat(tie_end, tie_end - tie) - gstart
    rank = (t_lo + t_hi + 1) / 2.0
    n_pos = np.add.reduceat(ys, starts)
    n_neg = (ends - starts) - n_pos
    rsum = np.add.reduceat(np.where(ys == 1, rank, 0.0), starts)
    with np.errstate(invalid="ignore", divide="ignore"):
        auc = (rsum - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg)
    auc[(n_pos == 0) | (n_neg == 0)] = np.nan
    return gs[starts], auc


@functools.lru_cache(maxsize=None)
def case(score_family, group_family, n):
    """(y, p, ids, reference table) of one test case, computed once and shared (treat as read-only)."""
    y, p = scores(score_family, n)
    ids = group_ids(group_family, n)
    for a in (y, p, ids):
        a.setflags(write=False)
    return y, p, ids, ref_table(y, p, ids)
