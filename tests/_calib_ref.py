"""Inputs and the host reference shared by the calibration tests (test_calibration_host.py,
test_gpu_calibration.py).

``ref_table`` is the definition written out on the host: a numpy sort of the keys ``(bits(p) << 1) | y``,
then Python-integer sums per bin of ``fx(p) = rint((double)p * 2^32)`` and ``fx2(p) = rint((double)p *
(double)p * 2^32)`` for both planes -- equal width (``min(B - 1, floor((double)p * B))``) and equal mass
(ranks ``[floor(b n / B), floor((b + 1) n / B))`` of the sorted keys).  ``direct`` is an independent plain
float64 computation of the scalars from (y, p), with per-bin means and ``math.fsum``.
"""
import functools
import itertools
import math

import numpy as np

from tests._gauc_ref import _labels, scores as _gauc_scores

FAMILIES = ("uniform", "sevenths", "all_equal", "hundredths", "ctr", "edges")
# a wave of 64, a workgroup / prefix block of 256 (2047 .. 2049: also the sort's tile), several blocks, one
# top-level chunk of the two-level prefix (256 blocks of 256 = 65 536 samples) and one sample past it
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4099, 65537, 70001)
BINS = (1, 2, 6, 10, 16, 100, 1024)
COLS = ("n", "n_pos", "sum_p", "sum_p_pos", "sum_p2")
ONE = 1 << 32


def _edges():
    v = [0.0, -0.0, 1.0]
    for k in range(1, 16):
        x = np.float32(k / 16)
        v += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(2))]
    v += [2.0 ** -33, 3 * 2.0 ** -33, 2.0 ** -149]          # fx ties to 0, fx ties to 2, the smallest denormal
    return np.array(v, dtype=np.float32)


def scores(family, n, seed=0):
    """(labels, probabilities) as float32 arrays."""
    if family in ("uniform", "sevenths", "all_equal"):
        return _gauc_scores(family, n, seed)
    rng = np.random.default_rng(5000 * seed + n + 17)
    if family == "hundredths":
        return _labels(rng, n), (rng.integers(0, 101, n) / 100.0).astype(np.float32)
    if family == "ctr":                                    # scores pile up near 0.03; the model under-predicts
        p = rng.beta(2.0, 60.0, n).astype(np.float32)
        y = (rng.random(n) < np.minimum(1.0, 1.3 * p.astype(np.float64))).astype(np.float32)
        return y, p
    if family == "edges":
        e = _edges()
        return _labels(rng, n), e[np.arange(n) % len(e)].copy()
    raise AssertionError(family)


def keys_of(y, p):
    """The uint32 keys fbn_eval_pack writes: (bits(p) << 1) | y, with -0.0 as 0.0."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    bits = np.where(p == 0, np.uint32(0), p.view(np.uint32)).astype(np.uint32)
    return (bits << np.uint32(1)) | (np.asarray(y) == 1).astype(np.uint32)


def width_bin(p, bins):
    """The equal-width rule, the product taken in float64."""
    return np.minimum(bins - 1, np.floor(np.asarray(p, dtype=np.float32).astype(np.float64) * bins).astype(np.int64))


def _prefix(values):
    return [0] + list(itertools.accumulate(values))          # Python integers: exact at any size


def _sorted_sums(y, p):
    """The sorted scores and the prefix sums (Python integers) of {y, fx, y fx, fx2} along the sorted keys."""
    k = np.sort(keys_of(y, p))
    pf = (k >> np.uint32(1)).astype(np.uint32).view(np.float32)
    pd = pf.astype(np.float64)
    pos = [int(v) for v in (k & np.uint32(1))]
    fx = [int(v) for v in np.rint(pd * 2.0 ** 32)]          # exact products; rint is round-half-even
    fx2 = [int(v) for v in np.rint(pd * pd * 2.0 ** 32)]
    return pf, (_prefix(pos), _prefix(fx), _prefix(f if c else 0 for f, c in zip(fx, pos)), _prefix(fx2))


def _plane(pf, prefix, bounds):
    nb = len(bounds) - 1
    out = {c: np.zeros(nb, dtype=np.int64) for c in COLS}
    out["p_lo"] = np.full(nb, np.nan, dtype=np.float32)
    out["p_hi"] = np.full(nb, np.nan, dtype=np.float32)
    for b in range(nb):
        lo, hi = int(bounds[b]), int(bounds[b + 1])
        if hi <= lo:
            continue
        out["n"][b] = hi - lo
        for c, pre in zip(COLS[1:], prefix):
            out[c][b] = pre[hi] - pre[lo]
        out["p_lo"][b], out["p_hi"][b] = pf[lo], pf[hi - 1]
    return out


def ref_table(y, p, bins, _sums=None):
    """{"width": plane, "mass": plane}; a plane is a dict of length-`bins` arrays: n, n_pos, sum_p,
    sum_p_pos, sum_p2 (int64, summed as Python integers) and p_lo, p_hi (float32, NaN when empty)."""
    pf, prefix = _sums if _sums is not None else _sorted_sums(y, p)
    n = len(pf)
    wb = width_bin(pf, bins)                                # non-decreasing along the sorted keys
    assert np.all(np.diff(wb) >= 0)
    wbounds = np.searchsorted(wb, np.arange(bins + 1), side="left")
    wbounds[bins] = n
    mbounds = [(b * n) // bins for b in range(bins + 1)]
    return {"width": _plane(pf, prefix, wbounds), "mass": _plane(pf, prefix, mbounds)}


def direct(y, p, bins):
    """The scalars in plain float64 from (y, p): per-bin means and math.fsum (no fixed point)."""
    y = np.asarray(y, dtype=np.float64)
    pd = np.asarray(p, dtype=np.float32).astype(np.float64)
    n, n_pos = len(y), int(y.sum())
    order = np.argsort(keys_of(y, p), kind="stable")

    def ece(bin_of):
        gaps, worst = [], 0.0
        for b in range(bins):
            sel = bin_of == b
            if sel.any():
                gap = abs(math.fsum(y[sel]) - math.fsum(pd[sel]))
                gaps.append(gap)
                worst = max(worst, gap / int(sel.sum()))
        return math.fsum(gaps) / n, worst

    mass_bin = np.empty(n, dtype=np.int64)
    for b in range(bins):
        mass_bin[order[(b * n) // bins:((b + 1) * n) // bins]] = b
    e_w, mce = ece(width_bin(p, bins))
    e_m, _ = ece(mass_bin)
    r = n_pos / n
    return {"ece": e_w, "mce": mce, "ece_mass": e_m,
            "pcoc": math.fsum(pd) / n_pos if n_pos else float("nan"),
            "brier": math.fsum((pd - y) ** 2) / n,
            "entropy": 0.0 if n_pos in (0, n) else -(r * math.log(r) + (1 - r) * math.log(1 - r))}


@functools.lru_cache(maxsize=None)
def case(family, n):
    """(y, p) of one test case, computed once and shared (read-only)."""
    y, p = scores(family, n)
    y.setflags(write=False)
    p.setflags(write=False)
    return y, p


@functools.lru_cache(maxsize=None)
def _case_sums(family, n):
    return _sorted_sums(*case(family, n))


@functools.lru_cache(maxsize=None)
def table(family, n, bins):
    """The reference table of case(family, n), computed once and shared (treat as read-only)."""
    y, p = case(family, n)
    return ref_table(y, p, bins, _sums=_case_sums(family, n))


def same_table(got, ref):
    """None, or a description of the first difference: integer columns by value and dtype, the bin ends bitwise."""
    for plane in ("width", "mass"):
        for c in COLS:
            a = np.asarray(got[plane][c])
            if a.dtype != np.int64 or not np.array_equal(a, ref[plane][c]):
                return f"{plane}.{c}"
        for c in ("p_lo", "p_hi"):
            a = np.asarray(got[plane][c])
            if a.dtype != np.float32 or a.tobytes() != ref[plane][c].tobytes():
                return f"{plane}.{c}"
    return None
