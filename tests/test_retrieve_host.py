"""Host side of the retrieval stage: the float64 reference and band comparator (tests/_knn_ref.py), the
argument checks of the three fbn_knn_* entry points (they precede any device call: null pointers, no
GPU) and the ValueErrors of the four Recommender methods, raised before anything is launched."""
import numpy as np
import pytest
import torch

from tests import _knn_ref as ref

FBN_ERR_ARG = 1


def _lib():
    from ctr_recommendation_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------- the comparator
def _row(seed=3, M=300, D=16):
    rng = np.random.default_rng(seed)
    Xn, _ = ref.normalize_ref(rng.standard_normal((M, D)))
    ids = np.arange(1, M + 1)
    ids[17] = 0
    el = ref.eligible_ref(ids, [ids[5]])
    return ref.scores_ref(Xn[5:6], Xn)[0], el


def test_reference_selection_excludes_and_breaks_ties_by_position():
    s, el = _row()
    assert not el[17] and not el[5] and el.sum() == 298
    s = s.copy()
    s[40] = s[200] = 2.0                                  # two equal best scores
    top = ref.select_ref(s, el, 5)
    assert top[:2].tolist() == [40, 200]
    assert ref.rank_ref(s, el, 200) == 2 and ref.rank_ref(s, el, 40) == 1
    few = ref.select_ref(s, np.arange(len(s)) < 3, 5)     # three eligible items: a -1 tail
    assert few[3:].tolist() == [-1, -1] and set(few[:3].tolist()) == {0, 1, 2}


def test_comparator_accepts_the_exact_list_and_a_swap_inside_the_band():
    s, el = _row()
    K, tol = 10, ref.tol_scores(16)
    top = ref.select_ref(s, el, K + 1)
    assert ref.band_check(s, el, top[:K], s[top[:K]].astype(np.float32), tol) >= 1
    # move the (K+1)-th item to within tol/4 below the K-th: either may be returned
    s2 = s.copy()
    s2[top[K]] = s2[top[K - 1]] - tol / 4
    swapped = top[:K].copy()
    swapped[K - 1] = top[K]
    dev = s2[swapped].copy()
    dev[K - 1] = s2[top[K - 1]] + tol / 4                 # the device saw it just above
    assert ref.band_check(s2, el, swapped, dev, tol) == 2
    assert ref.band_check(s2, el, top[:K], s2[top[:K]], tol) == 2


def test_comparator_rejects_planted_wrong_answers():
    s, el = _row()
    K, tol = 10, ref.tol_scores(16)
    top = ref.select_ref(s, el, K)
    good = s[top]
    worst = int(np.flatnonzero(el)[np.argmin(s[el])])
    bad = top.copy()
    bad[K - 1] = worst                                    # an item far below the band, best item 3 kept
    with pytest.raises(AssertionError):
        ref.band_check(s, el, bad, s[bad], tol)
    bad = np.concatenate([top[:3], top[4:], ref.select_ref(s, el, K + 1)[K:]])   # the 4th best is missing
    with pytest.raises(AssertionError, match="above the band"):
        ref.band_check(s, el, bad, s[bad], tol)
    with pytest.raises(AssertionError, match="off by more"):
        ref.band_check(s, el, top, good + 8 * tol, tol)
    bad = top.copy()
    bad[0] = 17                                           # the padding item
    with pytest.raises(AssertionError, match="ineligible"):
        ref.band_check(s, el, bad, s[bad], tol)
    bad = top.copy()
    bad[[2, 3]] = bad[[3, 2]]                             # right set, wrong order
    with pytest.raises(AssertionError, match="key order"):
        ref.band_check(s, el, bad, s[bad], tol)
    with pytest.raises(AssertionError, match="tail"):
        ref.band_check(s, np.arange(len(s)) < 3, top, good, tol)     # 3 eligible items, 10 returned


def test_normalised_sum_orders_as_the_mean_cosine():
    """<sum_i x_i / |sum_i x_i|, y> = (L / |sum_i x_i|) * mean_i <x_i, y>: one positive factor per user."""
    rng = np.random.default_rng(5)
    Xn, _ = ref.normalize_ref(rng.standard_normal((400, 32)))
    ids = np.arange(1, 401)
    pos = ref.positions_ref(ids, 500)
    seq = np.array([[3, 9, 9, 0, 250, 499, 77], [0, 0, 0, 0, 0, 0, 0]])     # 499: not in the catalogue
    Qn, n_used = ref.pool_ref(seq, pos, Xn)
    assert n_used.tolist() == [5, 0] and not Qn[1].any()
    hist = Xn[[2, 8, 8, 249, 76]]
    mean_cos = (hist @ Xn.T).mean(axis=0)
    s = ref.scores_ref(Qn[:1], Xn)[0]
    factor = 5 / np.linalg.norm(hist.sum(axis=0))
    assert factor > 0 and np.allclose(s, factor * mean_cos, rtol=0, atol=1e-14)
    assert (np.argsort(-s, kind="stable") == np.argsort(-mean_cos, kind="stable")).all()


# ---------------------------------------------------------------------------------------- entry points
def test_knn_entry_points_check_their_arguments_on_the_host():
    h = _lib()
    dims = b"16,32,64,128,256"
    # bad D, with the list in the message and the entry point's own name
    assert h.fbn_knn_normalize(None, 48, None, 10, None, 10, 48, None, None) == FBN_ERR_ARG
    assert b"fbn_knn_normalize" in h.fbn_last_error() and dims in h.fbn_last_error()
    assert h.fbn_knn_query_pool(None, 4, 20, None, 100, None, 10, 24, None, None, None) == FBN_ERR_ARG
    assert b"fbn_knn_query_pool" in h.fbn_last_error() and dims in h.fbn_last_error()
    assert h.fbn_knn_scores(None, 512, None, None, 10, 4, 0, 10, 512, None, None) == FBN_ERR_ARG
    assert b"fbn_knn_scores" in h.fbn_last_error() and dims in h.fbn_last_error()
    # L = 33
    assert h.fbn_knn_query_pool(None, 4, 33, None, 100, None, 10, 16, None, None, None) == FBN_ERR_ARG
    assert b"fbn_knn_query_pool" in h.fbn_last_error() and b"0..32" in h.fbn_last_error()
    # a chunk that leaves the catalogue
    assert h.fbn_knn_scores(None, 16, None, None, 1000, 4, 700, 301, 16, None, None) == FBN_ERR_ARG
    assert b"fbn_knn_scores" in h.fbn_last_error() and b"m0 + Mc <= M" in h.fbn_last_error()
    assert h.fbn_knn_scores(None, 16, None, None, 1000, 4, -1, 10, 16, None, None) == FBN_ERR_ARG
    # fbn_rec_topk's limits
    assert h.fbn_knn_scores(None, 16, None, None, 1000, 65536, 0, 10, 16, None, None) == FBN_ERR_ARG
    assert b"65535" in h.fbn_last_error()
    assert h.fbn_knn_scores(None, 16, None, None, 1 << 20, 4096, 0, 1 << 20, 16, None, None) == FBN_ERR_ARG
    assert b"31 bits" in h.fbn_last_error()
    # ldq < D
    assert h.fbn_knn_scores(None, 64, None, None, 1000, 4, 0, 10, 128, None, None) == FBN_ERR_ARG
    assert b"ldq >= D" in h.fbn_last_error()
    assert h.fbn_knn_normalize(None, 64, None, 10, None, 10, 128, None, None) == FBN_ERR_ARG
    assert b"ldx >= D" in h.fbn_last_error()
    # nothing to do: no launch, no error
    assert h.fbn_knn_normalize(None, 16, None, 0, None, 0, 16, None, None) == 0
    assert h.fbn_knn_query_pool(None, 0, 20, None, 100, None, 10, 16, None, None, None) == 0
    assert h.fbn_knn_scores(None, 16, None, None, 1000, 0, 0, 10, 16, None, None) == 0
    assert h.fbn_knn_scores(None, 16, None, None, 1000, 4, 1000, 0, 16, None, None) == 0


# ---------------------------------------------------------------------------------------- the methods
def test_chunks_are_multiples_of_1024_or_as_small_as_asked():
    from ctr_recommendation_amd.recommend import _knn_chunks, DEFAULT_KNN_CHUNK_BYTES
    assert _knn_chunks(1037, 3, 4 * 3 * 400) == [(0, 400), (400, 400), (800, 237)]
    assert _knn_chunks(1037, 3, DEFAULT_KNN_CHUNK_BYTES) == [(0, 1037)]
    ch = _knn_chunks(91718, 8192, DEFAULT_KNN_CHUNK_BYTES)
    assert all(mc % 1024 == 0 and 4 * 8192 * mc <= DEFAULT_KNN_CHUNK_BYTES for _, mc in ch[:-1])
    assert [m0 for m0, _ in ch] == list(np.cumsum([0] + [mc for _, mc in ch[:-1]])) and sum(mc for _, mc in ch) == 91718
    assert all(q * mc < 2 ** 31 for q in (1, 65535) for _, mc in _knn_chunks(3_000_000_000 // 4, q, 1 << 40))


def test_methods_raise_value_errors_before_any_launch():
    """The checks come first in each method, so they are reached on an object that has no device, no
    weights and no catalogue at all."""
    from ctr_recommendation_amd.recommend import Recommender, _check_knn
    rec = object.__new__(Recommender)
    items, seq = torch.arange(1, 5), torch.ones((3, 20), dtype=torch.int64)
    assert _check_knn("content", 10, by="index", items=items) == 4
    assert _check_knn("id", 256, item_seq=seq) == 3
    for kw in ({"space": "cosine"}, {"by": "slot"}):
        with pytest.raises(ValueError):
            rec.similar_items(items, 10, **kw)
    for k in (0, 257):
        with pytest.raises(ValueError, match="1..256"):
            rec.similar_items(items, k)
        with pytest.raises(ValueError, match="1..256"):
            rec.retrieve(seq, k)
        with pytest.raises(ValueError, match="1..256"):
            rec.recommend(seq, k)
        with pytest.raises(ValueError, match="1..256"):
            rec.recommend(seq, 10, n_candidates=k)
        with pytest.raises(ValueError):
            rec.evaluate_retrieval([], ns=(k,))
    for bad in (items.reshape(2, 2), items.float(), items[:0], [1, 2]):
        with pytest.raises(ValueError, match="items"):
            rec.similar_items(bad, 10)
    for bad in (seq[0], seq.float(), seq[:0], None):
        with pytest.raises(ValueError, match="item_seq"):
            rec.retrieve(bad, 10)
        with pytest.raises(ValueError, match="item_seq"):
            rec.recommend(bad, 10)
    with pytest.raises(ValueError, match="space"):
        rec.retrieve(seq, 10, space="MM")
    with pytest.raises(ValueError, match="space"):
        rec.recommend(seq, 10, space="")
    with pytest.raises(ValueError, match="space"):
        rec.evaluate_retrieval([], space="tower")
    with pytest.raises(ValueError, match="users_per_block"):
        rec.evaluate_retrieval([], users_per_block=0)
