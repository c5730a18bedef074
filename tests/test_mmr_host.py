"""Host side of the diversity feature: the float64 reference and the conditional judge
(tests/_mmr_ref.py) against exact, simulated and planted lists, the argument checks of fbn_mmr_select /
fbn_list_ild (they precede any device call: null pointers, no GPU) and the ValueErrors of the four
Recommender methods, raised before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _mmr_ref as ref
from tests._knn_ref import tol_scores

FBN_ERR_ARG = 1


def _lib():
    from ctr_recommendation_amd import _lib
    return _lib.lib()


# 36 random cases: D in {16, 128, 256}, C from 65 to 1024, K from 10 to 256
def _cases():
    rng = np.random.default_rng(2027)
    out = []
    for D in (16, 128, 256):
        for i in range(12):
            C = int(rng.integers(65, 1025)) if i < 10 else (65, 1024)[i - 10]
            K = int(rng.integers(10, 257)) if i < 10 else (256, 10)[i - 10]
            out.append((D, C, K, (0.3, 0.7, 0.5)[i % 3]))
    return out


CASES = _cases()


def _judge(case, seed, lists):
    D, C, K, lam = case
    Xn, pos, rel, live = ref.random_case(seed, D, C)
    slot, mmr, pen = lists(Xn, pos, rel, live, lam, K)
    tol = ref.tol_mmr(D, lam, float(rel.max()))
    return (Xn, pos, rel, live, lam, K), (slot, mmr, pen), (tol, tol_scores(D))


# ---------------------------------------------------------------------------------------- the judge
def test_tolerances_are_the_derived_ones():
    assert ref.tol_mmr(128, 0.7, 1.0) == pytest.approx(0.3 * 2 * 128 * 2.0 ** -24 + 4 * 2.0 ** -24)
    assert ref.tol_mmr(16, 1.0, 8.0) == pytest.approx(4 * 2.0 ** -24 * 8.0)
    assert ref.lam_pair(0.25) == (0.25, 0.75)
    lam, oml = ref.lam_pair(0.3)
    assert lam == float(np.float32(0.3)) and oml == float(np.float32(1) - np.float32(0.3))


def test_checker_accepts_the_reference_list():
    for i, case in enumerate(CASES[::3]):
        args, (slot, mmr, pen), tols = _judge(case, 100 + i, ref.mmr_ref)
        n = min(case[2], int(args[3].sum()))
        assert ref.mmr_conditional_check(*args, slot, mmr, pen, *tols) == n
        assert (slot[:n] >= 0).all() and len(set(slot[:n].tolist())) == n


def test_checker_accepts_an_f32_simulation_of_the_kernel_on_every_case():
    steps = want = diverged = 0
    for i, case in enumerate(CASES):
        args, (slot, mmr, pen), tols = _judge(case, 100 + i, ref.mmr_sim_f32)
        steps += ref.mmr_conditional_check(*args, slot, mmr, pen, *tols)
        want += min(case[2], int(args[3].sum()))
        diverged += int(not np.array_equal(slot, ref.mmr_ref(*args)[0]))
    assert steps == want and want > 3000                   # every step of every case was judged
    print(f"{steps} steps accepted; the f32 list left the float64 list in {diverged} of {len(CASES)} cases")


def test_checker_rejects_planted_wrong_answers():
    for i, case in enumerate(CASES[:6]):
        args, (slot, mmr, pen), tols = _judge(case, 100 + i, ref.mmr_ref)
        pos, live = args[1], args[3]
        # picks 1 and 2 swapped, their scores and penalties with them
        bad = [x.copy() for x in (slot, mmr, pen)]
        for b in bad:
            b[[1, 2]] = b[[2, 1]]
        with pytest.raises(AssertionError, match="step [12]"):
            ref.mmr_conditional_check(*args, *bad, *tols)
        # the slots alone swapped: the scores are then not the picks'
        bad = slot.copy()
        bad[[1, 2]] = bad[[2, 1]]
        with pytest.raises(AssertionError, match="step [12]"):
            ref.mmr_conditional_check(*args, bad, mmr, pen, *tols)
        # a slot that is not eligible
        dead = int(np.flatnonzero(~live)[0])
        bad = slot.copy()
        bad[3] = dead
        with pytest.raises(AssertionError, match="not eligible"):
            ref.mmr_conditional_check(*args, bad, mmr, pen, *tols)
        # a slot picked twice
        bad = slot.copy()
        bad[4] = bad[0]
        with pytest.raises(AssertionError, match="picked twice"):
            ref.mmr_conditional_check(*args, bad, mmr, pen, *tols)
        # a score or a penalty that is off, and a list that is too long
        off = mmr.copy()
        off[2] += 8 * tols[0]
        with pytest.raises(AssertionError, match="mmr"):
            ref.mmr_conditional_check(*args, slot, off, pen, *tols)
        off = pen.copy()
        off[2] += 8 * tols[1]
        with pytest.raises(AssertionError, match="penalty"):
            ref.mmr_conditional_check(*args, slot, mmr, off, *tols)
    Xn, pos, rel, live = ref.random_case(7, 16, 65)
    few = live & (np.arange(65) < 8)
    slot, mmr, pen = ref.mmr_ref(Xn, pos, rel, live, 0.5, 10)
    with pytest.raises(AssertionError, match="tail"):
        ref.mmr_conditional_check(Xn, pos, rel, few, 0.5, 10, slot, mmr, pen, ref.tol_mmr(16, 0.5, 1.0), tol_scores(16))


def test_reference_breaks_ties_by_slot_and_penalises_the_raw_maximum():
    X = np.eye(4)
    pos = np.array([0, 0, 1, 2, 5, -1])
    live = ref.live_ref(pos, 4)
    assert live.tolist() == [True, True, True, True, False, False]
    rel = np.array([1.0, 1.0, 0.5, 0.5, 9.0, 9.0])
    slot, mmr, pen = ref.mmr_ref(X, pos, rel, live, 0.5, 6)
    # slot 0 first (tie with its twin 1 -> smaller slot); 2 and 3 tie at 0.25; the twin pays 0.5 * 1: last
    assert slot.tolist() == [0, 2, 3, 1, -1, -1]
    assert mmr[:4].tolist() == [0.5, 0.25, 0.25, 0.0] and pen[:4].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert np.isneginf(mmr[4:]).all() and (pen[4:] == 0).all()
    Xneg = np.array([[1.0, 0.0], [-1.0, 0.0]])
    slot, mmr, pen = ref.mmr_ref(Xneg, np.array([0, 1]), np.array([1.0, 0.0]), np.array([True, True]), 0.5, 2)
    assert pen[1] == -1.0 and mmr[1] == 0.5                  # a negative cosine is a bonus: not clamped at 0
    ids = np.array([7, 0, 9, 9])
    assert ref.live_ref(np.array([0, 1, 2, 3]), 4, ids, [9, 0, 0], True).tolist() == [True, False, False, False]
    assert ref.ild_ref(np.eye(3), [0, 1, -1, 2, 3]) == (1.0, 3)
    assert ref.ild_ref(np.eye(3), [1, -1]) == (0.0, 0) and ref.ild_ref(np.eye(3), [1, 1])[0] == 0.0


# ---------------------------------------------------------------------------------------- entry points
def _mmr(h, *, ldr=200, ldp=200, U=4, C=200, M=1000, D=16, L=20, lam=0.7, K=10):
    return h.fbn_mmr_select(None, ldr, None, ldp, U, C, None, M, D, None, None, L, 1, ctypes.c_float(lam), K,
                            None, None, None, None, None, None, None, None)


def _ild(h, *, ldp=10, U=4, K=10, M=1000, D=16):
    return h.fbn_list_ild(None, ldp, U, K, None, M, D, None, None, None)


def test_diversity_entry_points_check_their_arguments_on_the_host():
    h = _lib()
    for K in (0, 257):
        assert _mmr(h, K=K) == FBN_ERR_ARG
        assert b"fbn_mmr_select" in h.fbn_last_error() and b"1..256" in h.fbn_last_error()
        assert _ild(h, K=K, ldp=300) == FBN_ERR_ARG
        assert b"fbn_list_ild" in h.fbn_last_error() and b"1..256" in h.fbn_last_error()
    assert _mmr(h, C=1025, ldr=2000, ldp=2000) == FBN_ERR_ARG
    assert b"1024" in h.fbn_last_error()
    for lam in (-0.1, 1.5, float("nan"), float("inf")):
        assert _mmr(h, lam=lam) == FBN_ERR_ARG
        assert b"lam" in h.fbn_last_error()
    assert _mmr(h, D=48) == FBN_ERR_ARG
    assert b"fbn_mmr_select" in h.fbn_last_error() and b"16,32,64,128,256" in h.fbn_last_error()
    assert _ild(h, D=48) == FBN_ERR_ARG
    assert b"fbn_list_ild" in h.fbn_last_error() and b"16,32,64,128,256" in h.fbn_last_error()
    assert _mmr(h, ldr=199) == FBN_ERR_ARG
    assert b"ldr >= C" in h.fbn_last_error()
    assert _mmr(h, ldp=199) == FBN_ERR_ARG
    assert _ild(h, ldp=9) == FBN_ERR_ARG
    assert b"ldp >= K" in h.fbn_last_error()
    assert _mmr(h, L=33) == FBN_ERR_ARG
    assert b"0..32" in h.fbn_last_error()
    assert _mmr(h, U=65536) == FBN_ERR_ARG and _ild(h, U=65536) == FBN_ERR_ARG
    # nothing to do: no launch, no error
    assert _mmr(h, U=0) == 0 and _ild(h, U=0) == 0
    assert _mmr(h, C=0) == 0
    from ctr_recommendation_amd import _lib as binding
    assert binding.FBN_MMR_MAX_C == 1024


# ---------------------------------------------------------------------------------------- the methods
def test_diversity_methods_raise_value_errors_before_any_launch():
    """The checks come first in each method, so they are reached on an object that has no device, no
    weights and no catalogue at all."""
    from ctr_recommendation_amd.recommend import Recommender
    rec = object.__new__(Recommender)
    seq = torch.ones((3, 20), dtype=torch.int64)
    cand = torch.arange(1, 31).reshape(3, 10)
    for lam in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lam"):
            rec.diversify(seq, cand, 5, lam=lam)
        with pytest.raises(ValueError, match="lam"):
            rec.recommend(seq, 5, lam=lam)
        with pytest.raises(ValueError, match="lam"):
            rec.evaluate_diversity([], lams=(1.0, lam))
    for k in (0, 257):
        with pytest.raises(ValueError, match="1..256"):
            rec.diversify(seq, cand, k)
        with pytest.raises(ValueError, match="1..256"):
            rec.recommend(seq, k, lam=0.5)
        with pytest.raises(ValueError, match="1..256"):
            rec.evaluate_diversity([], k=k)
        with pytest.raises(ValueError, match="1..256"):
            rec.evaluate_diversity([], n_candidates=k)
    for method, args in ((rec.diversify, (seq, cand, 5)), (rec.recommend, (seq, 5)), (rec.evaluate_diversity, ([],)),
                         (rec.list_diversity, (cand,))):
        with pytest.raises(ValueError, match="space"):
            method(*args, space="cosine")
    with pytest.raises(ValueError, match="1024"):
        rec.diversify(seq, torch.zeros((3, 1025), dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="by"):
        rec.diversify(seq, cand, 5, by="slot")
    with pytest.raises(ValueError, match="candidates"):
        rec.diversify(seq, cand[:2], 5)
    with pytest.raises(ValueError, match="candidates"):
        rec.diversify(None, cand, 5)                        # the cold user has one row
    for bad in ("score", torch.zeros((3, 9)), torch.zeros((3, 10), dtype=torch.float64), None):
        with pytest.raises(ValueError, match="relevance"):
            rec.diversify(seq, cand, 5, relevance=bad)
    for bad in (cand[0], cand.float(), cand[:0], torch.zeros((3, 257), dtype=torch.int64), [[1, 2]]):
        with pytest.raises(ValueError, match="index"):
            rec.list_diversity(bad)
    with pytest.raises(ValueError, match="users_per_block"):
        rec.evaluate_diversity([], users_per_block=0)
    with pytest.raises(ValueError, match="lams"):
        rec.evaluate_diversity([], lams=())
