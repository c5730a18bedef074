"""Inputs and the host reference shared by the isotonic calibrator's tests (test_isotonic_host.py,
test_gpu_isotonic.py).

``fit_ref`` is the definition written out on the host: a numpy sort of the keys ``(bits(p) << 1) | y``,
one (samples, positives) pair per run of equal score bits, then pool-adjacent-violators over Python
integers, pooling while the earlier block's rate is ``>=`` the later one's.  ``hull_ref`` is the other
form of the same definition: the lower convex hull of the cumulative diagram with
collinear points dropped, decided by integer cross products.  ``apply_ref`` is the apply rule in numpy
float64, one rounded operation at a time, rounded once to float32.
"""
import functools
from fractions import Fraction

import numpy as np

from tests import _calib_ref
from tests._calib_ref import keys_of

CALIB_FAMILIES = _calib_ref.FAMILIES
DEGENERATE = ("separable", "reversed", "all_pos", "all_neg")


def farey_sequence(m):
    """The fractions (a, b) of F_m in ascending order, 0/1 .. 1/1."""
    out, (a, b, c, d) = [(0, 1)], (0, 1, 1, m)
    while c <= m:
        k = (m + b) // d
        a, b, c, d = c, d, k * c - a, k * d - b
        out.append((a, b))
    return out


def _from_pieces(pieces, distinct=None):
    """pieces: (a, b) in score order.  distinct None: the b samples of a piece share one score; "neg_first" /
    "pos_first": every sample its own score, the piece's negatives (positives) first."""
    n = sum(b for _, b in pieces)
    y = np.zeros(n, dtype=np.float32)
    g = np.zeros(n, dtype=np.int64)
    at = 0
    for k, (a, b) in enumerate(pieces):
        if distinct == "neg_first":
            y[at + b - a:at + b] = 1.0
        else:
            y[at:at + a] = 1.0
        g[at:at + b] = k
        at += b
    rank = np.arange(n) if distinct else g
    p = ((rank + 1).astype(np.float64) / (int(rank[-1]) + 2)).astype(np.float32)   # increasing, distinct while below 2^23
    assert np.all(np.diff(p[np.concatenate(([True], np.diff(rank) > 0))]) > 0)
    return y, p


def scores(family, n=None):
    """(labels, probabilities) as float32 arrays, in a shuffled order (the fit does not depend on it)."""
    if family in CALIB_FAMILIES:
        return _calib_ref.case(family, n)
    name, _, arg = family.partition(":")
    if name == "farey":                                    # every group is a block
        y, p = _from_pieces(farey_sequence(int(arg)))
    elif name == "farey_repeat":                           # r locally convex pieces: the tile-hull-and-compact design stalls here
        m, r = (int(v) for v in arg.split(","))
        y, p = _from_pieces(farey_sequence(m) * r)
    elif name == "distinct_convex":                        # Farey slopes, all scores distinct, negatives first in a piece
        y, p = _from_pieces(farey_sequence(int(arg)), "neg_first")
    elif name == "distinct_blocks":                        # ... positives first: every piece is one block of distinct scores
        y, p = _from_pieces(farey_sequence(int(arg)), "pos_first")
    elif name in DEGENERATE:
        n = int(arg)
        p = ((np.arange(n) + 1.0) / (n + 1)).astype(np.float32)
        h = n // 2
        y = {"separable": (np.arange(n) >= h), "reversed": (np.arange(n) < max(1, h)),
             "all_pos": np.ones(n, bool), "all_neg": np.zeros(n, bool)}[name].astype(np.float32)
    else:
        raise AssertionError(family)
    perm = np.random.default_rng(len(y)).permutation(len(y))
    return y[perm].copy(), p[perm].copy()


def groups_of(y, p):
    """(score bits, samples, positives) per run of equal score bits of the sorted keys: uint32, int lists."""
    k = np.sort(keys_of(y, p))
    bits = (k >> np.uint32(1)).astype(np.uint32)
    if len(k) == 0:
        return bits, [], []
    first = np.flatnonzero(np.concatenate(([True], bits[1:] != bits[:-1])))
    end = np.concatenate((first[1:], [len(k)]))
    cpos = np.concatenate(([0], np.cumsum((k & np.uint32(1)).astype(np.int64))))
    return bits[first], [int(e - f) for f, e in zip(first, end)], [int(cpos[e] - cpos[f]) for f, e in zip(first, end)]


def _blocks(bits, spans, ns, poss):
    """spans: (first group, last group) per block."""
    lo = np.array([bits[a] for a, _ in spans], dtype=np.uint32).view(np.float32)
    hi = np.array([bits[b] for _, b in spans], dtype=np.uint32).view(np.float32)
    return {"lo": lo, "hi": hi, "n": np.array(ns, dtype=np.int64), "n_pos": np.array(poss, dtype=np.int64)}


def fit_ref(y, p):
    """{"lo", "hi" (float32), "n", "n_pos" (int64)} of the K blocks: PAV over Python integers, pooling on >=."""
    bits, cnt, pos = groups_of(y, p)
    st = []                                                # [first group, last group, n, pos]
    for g, (c, s) in enumerate(zip(cnt, pos)):
        st.append([g, g, c, s])
        while len(st) >= 2 and st[-2][3] * st[-1][2] >= st[-1][3] * st[-2][2]:
            b = st.pop()
            st[-1][1], st[-1][2], st[-1][3] = b[1], st[-1][2] + b[2], st[-1][3] + b[3]
    return _blocks(bits, [(a, b) for a, b, _, _ in st], [v[2] for v in st], [v[3] for v in st])


def hull_ref(y, p):
    """The same blocks from the definition: the lower hull of P_0 .. P_G, collinear points dropped."""
    bits, cnt, pos = groups_of(y, p)
    N, S = [0], [0]
    for c, s in zip(cnt, pos):
        N.append(N[-1] + c)
        S.append(S[-1] + s)
    h = []
    for c in range(len(N)):
        while len(h) >= 2:
            a, b = h[-2], h[-1]
            if (S[b] - S[a]) * (N[c] - N[b]) >= (S[c] - S[b]) * (N[b] - N[a]):
                h.pop()
            else:
                break
        h.append(c)
    spans = [(h[j], h[j + 1] - 1) for j in range(len(h) - 1)]
    return _blocks(bits, spans, [N[h[j + 1]] - N[h[j]] for j in range(len(h) - 1)],
                   [S[h[j + 1]] - S[h[j]] for j in range(len(h) - 1)])


def same_blocks(got, ref):
    """None, or the first column that differs: the scores bitwise, the counts by value and dtype."""
    for c in ("lo", "hi"):
        a = np.asarray(got[c])
        if a.dtype != np.float32 or a.tobytes() != ref[c].tobytes():
            return c
    for c in ("n", "n_pos"):
        a = np.asarray(got[c])
        if a.dtype != np.int64 or not np.array_equal(a, ref[c]):
            return c
    return None


def table_of(blocks, status=0):
    """The uint64 words fbn_isotonic_fit writes: K, then per block bits(lo) | bits(hi) << 32 and n | pos << 32,
    then the status word."""
    K = len(blocks["n"])
    t = np.zeros(2 * K + 2, dtype=np.uint64)
    t[0] = K
    t[1:2 * K + 1:2] = blocks["lo"].view(np.uint32).astype(np.uint64) | (blocks["hi"].view(np.uint32).astype(np.uint64) << np.uint64(32))
    t[2:2 * K + 2:2] = blocks["n"].astype(np.uint64) | (blocks["n_pos"].astype(np.uint64) << np.uint64(32))
    t[2 * K + 1] = status
    return t


def values(blocks):
    return blocks["n_pos"].astype(np.float64) / blocks["n"].astype(np.float64)


def apply_ref(blocks, p, mode="interp"):
    """The apply rule in numpy float64, each operation rounded on its own; float32 out.
    NaN passes through with its bits."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    x = p.astype(np.float64)
    lo, hi, v = blocks["lo"].astype(np.float64), blocks["hi"].astype(np.float64), values(blocks)
    K = len(v)
    assert K >= 1 and mode in ("interp", "step")
    nan = np.isnan(x)
    j = np.searchsorted(hi, np.where(nan, 0.0, x), side="left")           # the first block with hi >= x; K: none
    jc = np.minimum(j, K - 1)
    r = v[jc]
    if mode == "interp":
        gap = (j < K) & (jc > 0) & ~(x >= lo[jc])
        jp = np.maximum(jc - 1, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (x - hi[jp]) / (lo[jc] - hi[jp])
            ri = np.minimum(v[jp] + t * (v[jc] - v[jp]), v[jc])
        r = np.where(gap, ri, r)
    out = r.astype(np.float32)
    out[nan] = p[nan]
    return out


def max_blocks(n):
    """floor((3n)^(2/3) / 2) + 2 in Python integers: the integer cube root of 9 n^2, halved."""
    m = 9 * n * n
    r = int(round(m ** (1.0 / 3.0)))
    while r * r * r > m:
        r -= 1
    while (r + 1) ** 3 <= m:
        r += 1
    return r // 2 + 2


def max_blocks_exact(n):
    """The most blocks n samples can give: block rates are distinct fractions in [0, 1], a rate of reduced
    denominator b needs a block of at least b samples, and phi(b) rates have denominator b (b = 1: 0 and 1)
    -- so take denominators in ascending order while the samples last."""
    from math import gcd
    k, b = 0, 1
    while n >= b:
        rates = 2 if b == 1 else sum(1 for a in range(1, b) if gcd(a, b) == 1)
        take = min(rates, n // b)
        k += take
        n -= take * b
        b += 1
    return k


def probes(blocks, extra=()):
    """Sorted float32 probe scores: every lo / hi and its float32 neighbours, 0, 1, the smallest denormal, mid-gaps."""
    e = np.concatenate((blocks["lo"], blocks["hi"])).astype(np.float32)
    mid = ((blocks["hi"][:-1].astype(np.float64) + blocks["lo"][1:].astype(np.float64)) / 2).astype(np.float32)
    v = np.concatenate((e, np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(2)), mid,
                        np.array([0.0, 1.0, 2.0 ** -149, 0.25, 0.5], dtype=np.float32), np.asarray(extra, dtype=np.float32)))
    v = v[(v >= 0) & (v <= 1)]
    return np.sort(v.astype(np.float32))


@functools.lru_cache(maxsize=None)
def case(family, n=None):
    """(y, p, reference blocks) of one test case, computed once and shared (read-only)."""
    y, p = scores(family, n)
    ref = fit_ref(y, p)
    for a in (y, p, *ref.values()):
        a.setflags(write=False)
    return y, p, ref


def rate(blocks, j):
    return Fraction(int(blocks["n_pos"][j]), int(blocks["n"][j]))
