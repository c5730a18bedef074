"""Host reference shared by the DeLong tests (test_delong_host.py, test_gpu_delong.py); numpy only.

``placements`` and ``record`` are the integer definitions written out with np.searchsorted on the fp32
probabilities and Python integers; ``brute`` is DeLong's estimator as the paper states it -- the m x n
matrix psi(X_i, Y_j) in {0, 1/2, 1}, the structural components V10 / V01 as its row / column means, the
two-pass sample covariances S10 / S01 and S = S10 / m + S01 / n -- in float64, for N <= 2000.
"""
import functools

import numpy as np

from tests._calib_ref import case  # noqa: F401  (the score families: "ctr", "sevenths", "edges", "uniform", ...)

MASK32 = (1 << 32) - 1


def placements(y, p):
    """int64 [N]: for a positive 2 * #negatives below + #negatives equal, for a negative 2 * #positives
    above + #positives equal, on the float32 probabilities (-0.0 equals 0.0)."""
    y = np.asarray(y)
    p = np.asarray(p, dtype=np.float32)
    pos = y == 1
    sp, sn = np.sort(p[pos]), np.sort(p[~pos])
    out = np.empty(len(p), dtype=np.int64)
    lo, hi = np.searchsorted(sn, p[pos], "left"), np.searchsorted(sn, p[pos], "right")
    out[pos] = 2 * lo + (hi - lo)
    lo, hi = np.searchsorted(sp, p[~pos], "left"), np.searchsorted(sp, p[~pos], "right")
    out[~pos] = 2 * (len(sp) - hi) + (hi - lo)
    return out


def record(y, pa, pb=None):
    """fbn_delong_reduce's 8 words as Python integers (pb None: the set against itself)."""
    pos = np.asarray(y) == 1
    a = [int(v) for v in placements(y, pa)]
    b = a if pb is None else [int(v) for v in placements(y, pb)]
    p1 = [u * v for u, v, k in zip(a, b, pos) if k]         # Python integers: exact at any size
    p0 = [u * v for u, v, k in zip(a, b, pos) if not k]
    return [int(pos.sum()), int((~pos).sum()), sum(u for u, k in zip(a, pos) if k), sum(v for v, k in zip(b, pos) if k),
            sum(x & MASK32 for x in p1), sum(x >> 32 for x in p1), sum(x & MASK32 for x in p0), sum(x >> 32 for x in p0)]


def brute(y, pa, pb):
    """{"auc_a", "auc_b", "auc_var", "var_b", "cov", "delta_var"} by the O(m n) definition in float64."""
    y = np.asarray(y)
    assert len(y) <= 2000
    pos = y == 1
    m, n = int(pos.sum()), int((~pos).sum())
    V10, V01, auc = [], [], []
    for p in (pa, pb):
        p = np.asarray(p, dtype=np.float32).astype(np.float64)
        X, Y = p[pos][:, None], p[~pos][None, :]
        psi = (X > Y).astype(np.float64) + 0.5 * (X == Y)
        V10.append(psi.mean(axis=1))
        V01.append(psi.mean(axis=0))
        auc.append(psi.mean())

    def s(u, v, k):                                         # two-pass sample covariance
        return float(((u - u.mean()) * (v - v.mean())).sum() / (k - 1))

    S = [[s(V10[r], V10[c], m) / m + s(V01[r], V01[c], n) / n for c in range(2)] for r in range(2)]
    # the contrast (1, -1) S (1, -1)' taken on the components' differences: the same number as S00 + S11 -
    # 2 S01 without that sum's cancellation
    d10, d01 = V10[0] - V10[1], V01[0] - V01[1]
    return {"auc_a": float(auc[0]), "auc_b": float(auc[1]), "auc_var": S[0][0], "var_b": S[1][1], "cov": S[0][1],
            "delta_var": s(d10, d10, m) / m + s(d01, d01, n) / n}


def noisy(p, seed, sigma=0.02, decimals=3):
    """A second score set over the same samples: p plus noise, rounded (so that it ties), in [0, 1]."""
    rng = np.random.default_rng(77 + seed)
    q = np.clip(np.asarray(p, dtype=np.float32).astype(np.float64) + rng.normal(0.0, sigma, len(p)), 0.0, 1.0)
    return np.round(q, decimals).astype(np.float32)


@functools.lru_cache(maxsize=None)
def second_scores(family, n):
    """noisy() of case(family, n)'s scores, computed once and shared (read-only)."""
    q = noisy(case(family, n)[1], n)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def case_record(family, n):
    """record() of case(family, n) against itself, computed once and shared (read-only)."""
    y, p = case(family, n)
    return tuple(record(y, p))


@functools.lru_cache(maxsize=None)
def case_placements(family, n):
    y, p = case(family, n)
    out = placements(y, p)
    out.setflags(write=False)
    return out


def closed_form(m, n):
    """The record of m positives at 1.0 and n negatives at 0.0: every a_i = 2 n, every b_j = 2 m."""
    return [m, n, 2 * m * n, 2 * m * n, sum_low(m, 4 * n * n), sum_high(m, 4 * n * n),
            sum_low(n, 4 * m * m), sum_high(n, 4 * m * m)]


def sum_low(count, prod):
    """count equal products: the sum of their low 32 bits."""
    return count * (prod & MASK32)


def sum_high(count, prod):
    return count * (prod >> 32)
