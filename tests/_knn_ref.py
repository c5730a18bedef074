"""Float64 reference of the retrieval stage (csrc/retrieve.hip, Recommender.similar_items / retrieve) and
the band comparator its tests judge a selected list with.

Selection is fbn_rec_topk's: eligible items ordered by score, equal scores to the smaller catalogue
position; padding items (id 0) and the ids of the exclusion list are not eligible.  A float32 score
cannot decide the order of two items whose exact scores are closer than its own error, so a device list
is compared against the exact one up to a band of +-tol around the K-th exact score (``band_check``).
"""
import numpy as np


def tol_scores(D: int) -> float:
    """|S - exact| of a D-term f32 fmaf chain between vectors of norm 1 + a few ulp: D * 2^-24 * |a| |x|,
    with a factor 2 for the norms."""
    return 2.0 * D * 2.0 ** -24


def tol_unit(D: int) -> float:
    """Per component of a normalised row, relative to the row's largest: the sum of squares is off by at
    most D ulp, halved by the root; the hardware root, reciprocal and multiply add a few ulp."""
    return (D / 2 + 4) * 2.0 ** -24


def normalize_ref(X, row_of=None):
    """-> (Xn float64 [M, D], flag): rows x / |x|, the zero row kept, a row index outside the source a
    zero row that sets the flag."""
    X = np.asarray(X, dtype=np.float64)
    flag = False
    if row_of is not None:
        row_of = np.asarray(row_of, dtype=np.int64)
        ok = (row_of >= 0) & (row_of < X.shape[0])
        flag = bool((~ok).any())
        X = np.where(ok[:, None], X[np.clip(row_of, 0, X.shape[0] - 1)], 0.0)
    nrm = np.sqrt((X * X).sum(axis=1, keepdims=True))
    return np.divide(X, nrm, out=np.zeros_like(X), where=nrm > 0), flag


def pool_ref(item_seq, pos_of_id, Xn):
    """-> (Qn float64 [U, D], n_used int [U]): the normalised sum of Xn[pos_of_id[id]] over the slots
    whose id is not 0, lies inside pos_of_id and maps to a catalogue position; repeats count each time."""
    seq = np.asarray(item_seq, dtype=np.int64)
    pos_of_id = np.asarray(pos_of_id, dtype=np.int64)
    Xn = np.asarray(Xn, dtype=np.float64)
    U = seq.shape[0]
    Q = np.zeros((U, Xn.shape[1]))
    n_used = np.zeros(U, dtype=np.int64)
    for u in range(U):
        for i in seq[u]:
            if i != 0 and 0 <= i < pos_of_id.shape[0] and 0 <= pos_of_id[i] < Xn.shape[0]:
                Q[u] += Xn[pos_of_id[i]]
                n_used[u] += 1
    return normalize_ref(Q)[0], n_used


def positions_ref(item_id, V):
    """id -> smallest catalogue position, -1 for an id the catalogue lacks (Recommender._pos)."""
    pos = np.full(V, -1, dtype=np.int64)
    for m in range(len(item_id) - 1, -1, -1):
        if 0 <= item_id[m] < V:
            pos[item_id[m]] = m
    return pos


def scores_ref(A, Xn):
    return np.asarray(A, dtype=np.float64) @ np.asarray(Xn, dtype=np.float64).T


def eligible_ref(item_id, exclude_ids=()):
    """The positions fbn_rec_topk may return with exclude on: no padding item, no id of exclude_ids."""
    item_id = np.asarray(item_id, dtype=np.int64)
    ex = np.asarray([i for i in exclude_ids if i != 0], dtype=np.int64)
    return (item_id != 0) & ~np.isin(item_id, ex)


def select_ref(scores, eligible, k):
    """The k best eligible positions of one row of exact scores, best first, ties to the smaller
    position; -1 fills a short list."""
    idx = np.flatnonzero(eligible)
    order = idx[np.lexsort((idx, -scores[idx]))][:k]
    return np.concatenate([order, np.full(k - len(order), -1, dtype=np.int64)])


def rank_ref(scores, eligible, t):
    """fbn_rec_rank's rank of position t (the target stays eligible): 1 + the eligible items above it."""
    el = eligible.copy()
    el[t] = False
    above = (scores > scores[t]) | ((scores == scores[t]) & (np.arange(len(scores)) < t))
    return 1 + int((el & above).sum())


def band_check(scores, eligible, dev_index, dev_score, tol):
    """Judge one device list (positions and scores, length K) against one row of exact scores.

    With tau the K-th best exact eligible score: every eligible item above tau + tol must be present,
    none below tau - tol may be, every returned score is within tol of the exact one, the list is ordered
    by its own scores (equal scores: ascending position), holds no item twice and nothing ineligible,
    and is exactly as long as min(K, eligible items) with -1 / -inf behind.  Items within tol of tau are
    undecided; their number is returned.  Raises AssertionError with the reason otherwise."""
    scores = np.asarray(scores, dtype=np.float64)
    dev_index = np.asarray(dev_index, dtype=np.int64)
    dev_score = np.asarray(dev_score, dtype=np.float64)
    K = len(dev_index)
    idx = np.flatnonzero(eligible)
    n = min(K, len(idx))
    got = dev_index[:n]
    assert (dev_index[n:] == -1).all() and np.isneginf(dev_score[n:]).all(), "the tail is not empty slots"
    assert (got >= 0).all() and (got < len(scores)).all(), "an empty or out-of-range slot inside the list"
    assert len(set(got.tolist())) == n, "an item is returned twice"
    assert eligible[got].all(), "an ineligible item is returned"
    assert (np.abs(dev_score[:n] - scores[got]) <= tol).all(), "a returned score is off by more than tol"
    for a in range(n - 1):
        assert dev_score[a] > dev_score[a + 1] or (dev_score[a] == dev_score[a + 1] and got[a] < got[a + 1]), \
            "the list is not in key order"
    if n == 0:
        return 0
    tau = np.sort(scores[idx])[::-1][n - 1] if len(idx) > K else -np.inf
    must = idx[scores[idx] > tau + tol]
    assert np.isin(must, got).all(), "an item above the band is missing"
    assert (scores[got] >= tau - tol).all(), "an item below the band is returned"
    return int((np.abs(scores[idx] - tau) <= tol).sum()) if np.isfinite(tau) else 0
