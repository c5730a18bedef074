"""Float64 reference of the diversity kernels (csrc/diversify.hip, Recommender.diversify /
list_diversity) and the judges their tests use.

Greedy MMR in f32 does not return the float64 greedy list: at a near-tie the two runs pick different
slots, the penalties of every later step differ, and the lists never meet again (4 of 36 random cases in
a numpy simulation).  A device list is therefore not compared with ``mmr_ref``'s list.
``mmr_conditional_check`` replays the DEVICE's own picks in float64 instead: at every step, given the
slots the device picked before, the device's pick must be a best slot up to the error of its own
arithmetic.  Every step of every list is judged.
"""
import numpy as np

from tests._knn_ref import tol_scores


def f32(x) -> float:
    """The float32 nearest to x, as a Python float."""
    return float(np.float32(x))


def lam_pair(lam):
    """(lam, 1 - lam) as the kernel holds them: lam rounded to f32, oml = 1.0f - lam in f32."""
    lam32 = np.float32(lam)
    return float(lam32), float(np.float32(1.0) - lam32)


def tol_mmr(D: int, lam: float, rel_max: float) -> float:
    """|device score - exact score| of one slot at one step, both for the same earlier picks.  The
    penalty is a maximum of D-term chains, each within tol_scores(D) of its exact dot, so the exact and
    the device maximum differ by at most that, scaled by 1 - lam.  The score then takes three f32
    roundings -- oml * pen, the fused lam * rel - that, and lam * rel alone at step 0 -- each at most
    2^-24 of a magnitude bounded by max(1, lam * rel_max) + 1; 4 * 2^-24 * max(1, lam * rel_max) covers
    them."""
    return (1.0 - lam) * tol_scores(D) + 4.0 * 2.0 ** -24 * max(1.0, lam * rel_max)


def live_ref(pos, M, item_id=None, seq=None, exclude=False):
    """The slots fbn_mmr_select may pick: a position inside the catalogue and, with exclude, an item that
    is neither the padding item nor a non-padding id of the user's history."""
    pos = np.asarray(pos, dtype=np.int64)
    live = (pos >= 0) & (pos < M)
    if exclude:
        ids = np.asarray(item_id, dtype=np.int64)[np.clip(pos, 0, M - 1)]
        hist = np.asarray([] if seq is None else seq, dtype=np.int64)
        live &= (ids != 0) & ~np.isin(ids, hist[hist != 0])
    return live


def _sims(Xn, pos, live):
    """[C, C] exact dots between the candidates' rows (zero rows for slots that are not live)."""
    Xn = np.asarray(Xn, dtype=np.float64)
    rows = np.where(live[:, None], Xn[np.clip(pos, 0, Xn.shape[0] - 1)], 0.0)
    return rows @ rows.T


def mmr_ref(Xn, pos, rel, live, lam, K):
    """The exact greedy list of one user: -> (slot [K] with -1 behind, mmr [K], pen [K]).  Scores in
    float64 from the f32 values of lam and 1 - lam; equal scores go to the smaller slot."""
    pos, rel, live = np.asarray(pos, dtype=np.int64), np.asarray(rel, dtype=np.float64), np.asarray(live, dtype=bool)
    assert not np.isnan(rel[live]).any()
    lam, oml = lam_pair(lam)
    S = _sims(Xn, pos, live)
    open_ = live.copy()
    pen = np.full(len(pos), -np.inf)
    slots, mmrs, pens = np.full(K, -1, dtype=np.int64), np.full(K, -np.inf), np.zeros(K)
    for t in range(min(K, int(live.sum()))):
        score = lam * rel if t == 0 else lam * rel - oml * pen
        score = np.where(open_, score, -np.inf)
        cand = np.flatnonzero(open_)
        j = int(cand[np.argmax(score[cand])])            # argmax returns the first (smallest) of equals
        slots[t], mmrs[t], pens[t] = j, score[j], 0.0 if t == 0 else pen[j]
        open_[j] = False
        pen = np.maximum(pen, S[j])
    return slots, mmrs, pens


def mmr_sim_f32(Xn, pos, rel, live, lam, K):
    """A numpy simulation of the kernel's arithmetic in f32 (chains as a rounded a * b + c per term, which
    differs from the fused operation only by a rare double rounding): -> (slot, mmr, pen) as mmr_ref."""
    X = np.asarray(Xn, dtype=np.float32)
    pos, live = np.asarray(pos, dtype=np.int64), np.asarray(live, dtype=bool)
    rel = np.asarray(rel, dtype=np.float32)
    lam32 = np.float32(lam)
    oml32 = np.float32(1.0) - lam32
    rows = np.where(live[:, None], X[np.clip(pos, 0, X.shape[0] - 1)], np.float32(0)).astype(np.float64)
    open_ = live.copy()
    pen = np.full(len(pos), -np.inf, dtype=np.float32)
    slots, mmrs, pens = np.full(K, -1, dtype=np.int64), np.full(K, -np.inf), np.zeros(K)
    for t in range(min(K, int(live.sum()))):
        if t == 0:
            score = lam32 * rel
        else:
            with np.errstate(invalid="ignore"):
                prod = (oml32 * pen).astype(np.float32)
                score = (np.float64(lam32) * rel.astype(np.float64) - prod.astype(np.float64)).astype(np.float32)
        cand = np.flatnonzero(open_)
        j = int(cand[np.argmax(score[cand])])
        slots[t], mmrs[t], pens[t] = j, float(score[j]), 0.0 if t == 0 else float(pen[j])
        open_[j] = False
        acc = np.zeros(len(pos), dtype=np.float32)
        for k in range(rows.shape[1]):
            acc = (rows[:, k] * rows[j, k] + acc.astype(np.float64)).astype(np.float32)
        pen = np.maximum(pen, acc)
    return slots, mmrs, pens


def mmr_conditional_check(Xn, pos, rel, live, lam, K, dev_slot, dev_mmr, dev_pen, tol, tol_pen,
                          dev_index=None, dev_rel=None):
    """Judge one user's device list given the device's own earlier picks.  At every step t, with S the
    slots the device picked before: the pick is live and unpicked; its exact score is within 2 * tol of
    the best exact score among the live unpicked slots (each of the two compared device scores is within
    tol of its exact one); dev_mmr is within tol of the pick's exact score and dev_pen within tol_pen of
    its exact penalty (0 at t = 0); behind min(K, live slots) picks the tail is -1 / -inf / 0; no slot is
    picked twice.  dev_index / dev_rel, when given, must be the pick's position and relevance as given.
    Returns the number of steps judged; raises AssertionError with the reason otherwise."""
    pos, rel, live = np.asarray(pos, dtype=np.int64), np.asarray(rel, dtype=np.float64), np.asarray(live, dtype=bool)
    dev_slot = np.asarray(dev_slot, dtype=np.int64)
    dev_mmr, dev_pen = np.asarray(dev_mmr, dtype=np.float64), np.asarray(dev_pen, dtype=np.float64)
    assert len(dev_slot) == K and len(dev_mmr) == K and len(dev_pen) == K
    lam, oml = lam_pair(lam)
    S = _sims(Xn, pos, live)
    n = min(K, int(live.sum()))
    assert (dev_slot[n:] == -1).all() and np.isneginf(dev_mmr[n:]).all() and (dev_pen[n:] == 0).all(), \
        "the tail is not empty slots"
    if dev_index is not None:
        assert (np.asarray(dev_index)[n:] == -1).all(), "the tail is not empty slots"
    if dev_rel is not None:
        assert np.isneginf(np.asarray(dev_rel, dtype=np.float64)[n:]).all(), "the tail is not empty slots"
    open_ = live.copy()
    pen = np.full(len(pos), -np.inf)
    for t in range(n):
        j = int(dev_slot[t])
        assert 0 <= j < len(pos), f"step {t}: slot {j} is outside the list"
        assert live[j], f"step {t}: slot {j} is not eligible"
        assert open_[j], f"step {t}: slot {j} is picked twice"
        score = lam * rel if t == 0 else lam * rel - oml * pen
        best = score[open_].max()
        assert score[j] >= best - 2 * tol, f"step {t}: slot {j} scores {score[j]!r}, the best open slot {best!r}"
        assert abs(dev_mmr[t] - score[j]) <= tol, f"step {t}: mmr {dev_mmr[t]!r} against {score[j]!r}"
        want_pen = 0.0 if t == 0 else pen[j]
        assert abs(dev_pen[t] - want_pen) <= tol_pen, f"step {t}: penalty {dev_pen[t]!r} against {want_pen!r}"
        if dev_index is not None:
            assert int(dev_index[t]) == int(pos[j]), f"step {t}: index is not the slot's position"
        if dev_rel is not None:
            assert float(dev_rel[t]) == float(rel[j]), f"step {t}: relevance is not the slot's"
        open_[j] = False
        pen = np.maximum(pen, S[j])
    return n


def ild_ref(Xn, list_pos):
    """-> (ild, n_pairs) of one list of catalogue positions: the exact mean of 1 - <a, b> over the pairs
    of its live entries (0 <= m < M); a position listed twice is two entries."""
    Xn = np.asarray(Xn, dtype=np.float64)
    p = np.asarray(list_pos, dtype=np.int64)
    p = p[(p >= 0) & (p < Xn.shape[0])]
    n = len(p)
    if n < 2:
        return 0.0, 0
    G = Xn[p] @ Xn[p].T
    iu = np.triu_indices(n, 1)
    return float((1.0 - G[iu]).mean()), n * (n - 1) // 2


def random_case(seed, D, C, M=None, dead=0.1):
    """One user's random case: -> (Xn f32 [M, D] of unit rows, pos [C] with repeats and dead slots,
    rel f32 [C] in [0, 1), live [C])."""
    rng = np.random.default_rng(seed)
    M = M if M is not None else max(8, C // 2)
    X = rng.standard_normal((M, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    pos = rng.integers(0, M, size=C)
    pos[rng.random(C) < dead] = -1
    rel = rng.random(C).astype(np.float32)
    return X.astype(np.float32), pos, rel, live_ref(pos, M)
