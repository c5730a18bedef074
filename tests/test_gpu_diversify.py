"""Diversity kernels (csrc/diversify.hip, Recommender.diversify / list_diversity / recommend(lam=) /
evaluate_diversity) on an MI355X: pytest -m gpu.

A device list is judged by tests/_mmr_ref.py's conditional check -- the device's own picks replayed in
float64, every step -- not against the float64 greedy list, which f32 greedy selection leaves at a
near-tie; only the dyadic case, where every product and sum is exact in f32, is compared
slot for slot.  Shapes: C around the 64-lane wave, the 256-thread workgroup and the 1024-slot limit, K up
to 256, D in {16, 128, 256}; U in {1, 33}.  Tolerances are derived in _mmr_ref.py / _knn_ref.py.
"""
import functools

import numpy as np
import pytest
import torch

from ctr_recommendation_amd import _lib
from ctr_recommendation_amd._lib import call, ptr
from ctr_recommendation_amd.recommend import Recommender
from tests import _mmr_ref as ref
from tests._knn_ref import tol_scores
from test_gpu_recommend import L_HIST, M_CAT, _catalogue, _cfg, _histories, _state

pytestmark = pytest.mark.gpu

OUT_INT = ("slot", "index", "item")
OUT_F32 = ("rel", "mmr", "pen")


# ---------------------------------------------------------------------------------------- raw entry points
def _mmr(dev, rel, pos, xn, item_id, lam, K, seq=None, exclude=False, ldr=None):
    """fbn_mmr_select on the device -> (outputs [U, K] as numpy, status word).  The output buffers are
    filled with sentinels first, so a store that is missing shows."""
    U, C = pos.shape
    M, D = xn.shape
    rel_d = torch.as_tensor(rel, dtype=torch.float32).to(dev)
    if ldr is not None:                                   # a wider row than C
        wide = torch.full((U, ldr), float("nan"), dtype=torch.float32, device=dev)
        wide[:, :C] = rel_d
        rel_d = wide
    rel_d = rel_d.contiguous()
    pos_d = torch.as_tensor(pos, dtype=torch.int64).to(dev).contiguous()
    ids_d = torch.as_tensor(item_id, dtype=torch.int64).to(dev).contiguous()
    seq_d = None if seq is None else torch.as_tensor(seq, dtype=torch.int64).to(dev).contiguous()
    L = 0 if seq is None else int(seq_d.shape[1])
    out = {n: torch.full((U, K), -77, dtype=torch.int64, device=dev) for n in OUT_INT}
    out.update({n: torch.full((U, K), float("nan"), dtype=torch.float32, device=dev) for n in OUT_F32})
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    call("fbn_mmr_select", ptr(rel_d), int(rel_d.shape[1]), ptr(pos_d), C, U, C, ptr(xn), M, D, ptr(ids_d), ptr(seq_d), L,
         int(exclude), float(lam), K, *[ptr(out[n]) for n in OUT_INT + OUT_F32], ptr(status), _lib.stream_handle(dev))
    got = {n: v.cpu().numpy() for n, v in out.items()}
    return got, int(status.item())


def _ild(dev, lists, xn, ldp=None):
    U, K = lists.shape
    M, D = xn.shape
    lp = torch.as_tensor(lists, dtype=torch.int64).to(dev)
    if ldp is not None:
        wide = torch.full((U, ldp), 3, dtype=torch.int64, device=dev)
        wide[:, :K] = lp
        lp = wide
    lp = lp.contiguous()
    ild = torch.full((U,), float("nan"), dtype=torch.float64, device=dev)
    n_pairs = torch.full((U,), -7, dtype=torch.int32, device=dev)
    call("fbn_list_ild", ptr(lp), int(lp.shape[1]), U, K, ptr(xn), M, D, ptr(ild), ptr(n_pairs), _lib.stream_handle(dev))
    return ild, n_pairs


def _unit_rows(dev, M, D, seed):
    """[M, D] f32 unit rows normalised on the device (fbn_knn_normalize), row 2 the zero vector."""
    rng = np.random.default_rng(seed)
    X = torch.from_numpy(rng.standard_normal((M, D)).astype(np.float32))
    X[2] = 0.0
    xn = torch.empty((M, D), dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    call("fbn_knn_normalize", ptr(X.to(dev)), D, None, M, ptr(xn), M, D, ptr(err), _lib.stream_handle(dev))
    torch.cuda.synchronize(dev)
    return xn


def _check_user(x64, pos, rel, live, lam, K, got, u, D, item_id=None):
    tol = ref.tol_mmr(D, lam, float(np.abs(rel[live]).max()) if live.any() else 1.0)
    n = ref.mmr_conditional_check(x64, pos, rel, live, lam, K, got["slot"][u], got["mmr"][u], got["pen"][u], tol,
                                  tol_scores(D), dev_index=got["index"][u], dev_rel=got["rel"][u])
    if item_id is not None:
        assert (got["item"][u][:n] == np.asarray(item_id)[got["index"][u][:n]]).all()
        assert (got["item"][u][n:] == -1).all()
    return n


# ---------------------------------------------------------------------------------------- 1. the exact case
@functools.lru_cache(maxsize=None)
def _dyadic():
    """64 rows of norm exactly 1 with dyadic entries: one +-1, four +-0.5 or sixteen +-0.25."""
    rng = np.random.default_rng(16)
    X = np.zeros((64, 16), dtype=np.float32)
    for r in range(64):
        nz, v = ((1, 1.0), (4, 0.5), (16, 0.25))[r % 3]
        cols = rng.permutation(16)[:nz]
        X[r, cols] = v * rng.choice([-1.0, 1.0], size=nz)
    assert (np.square(X.astype(np.float64)).sum(axis=1) == 1.0).all()
    pos = rng.integers(0, 64, size=(2, 200))
    rel = (rng.integers(0, 65, size=(2, 200)) / 64.0).astype(np.float32)
    return X, pos, rel


@pytest.mark.parametrize("lam", [0.0, 0.25, 0.5, 0.75, 1.0])
def test_dyadic_case_equals_the_float64_greedy_list(hip_device, lam):
    dev = hip_device
    X, pos, rel = _dyadic()
    xn = torch.from_numpy(X).to(dev)
    ids = np.arange(1, 65)
    got, status = _mmr(dev, rel, pos, xn, ids, lam, 200)
    assert status == 0
    ties = 0
    for u in range(2):
        live = ref.live_ref(pos[u], 64)
        slot, mmr, pen = ref.mmr_ref(X, pos[u], rel[u], live, lam, 200)
        assert got["slot"][u].tolist() == slot.tolist()
        assert (got["mmr"][u].astype(np.float64) == mmr).all() and (got["pen"][u].astype(np.float64) == pen).all()
        assert (got["index"][u] == pos[u][slot]).all() and (got["item"][u] == ids[pos[u][slot]]).all()
        assert (got["rel"][u] == rel[u][slot]).all()
        ties += int((mmr[1:] == mmr[:-1]).sum())
    assert ties > 20                                      # the smaller-slot rule decided many steps


# ---------------------------------------------------------------------------------------- 2. random vectors
SHAPES = [(1, 1), (2, 5), (63, 10), (65, 65), (200, 10), (257, 256), (1024, 32)]


def _random_lists(D, C, U, seed):
    """-> (M, pos [U, C], rel [U, C], item_id [M], seq [U, 5]): positions with repeats, empty slots,
    positions >= M, a padding item (position 1), the zero row (position 2), history ids that occur in the
    lists, and user 0's list mostly empty."""
    rng = np.random.default_rng(seed)
    M = max(8, C // 2 + 3)
    pos = rng.integers(0, M, size=(U, C))
    pos[rng.random((U, C)) < 0.08] = -1
    pos[rng.random((U, C)) < 0.04] = M + 5
    if C > 2:
        pos[:, 1], pos[:, 2] = 1, 2
        pos[0, rng.random(C) < 0.8] = -1
    rel = rng.random((U, C)).astype(np.float32)
    item_id = np.arange(M, dtype=np.int64) + 10
    item_id[1] = 0
    seq = np.zeros((U, 5), dtype=np.int64)
    for u in range(U):
        seq[u, 1:4] = item_id[np.clip(pos[u, rng.integers(0, C, size=3)], 0, M - 1)]
    return M, pos, rel, item_id, seq


@pytest.mark.parametrize("U", [1, 33])
@pytest.mark.parametrize("C,K", SHAPES)
@pytest.mark.parametrize("D", [16, 128, 256])
def test_random_lists_pass_the_conditional_check(hip_device, D, C, K, U):
    dev = hip_device
    M, pos, rel, item_id, seq = _random_lists(D, C, U, 1000 * D + C + U)
    xn = _unit_rows(dev, M, D, D + C)
    x64 = xn.double().cpu().numpy()
    steps = 0
    for lam, exclude in ((0.3, True), (0.3, False), (0.7, True), (0.7, False)):
        got, status = _mmr(dev, rel, pos, xn, item_id, lam, K, seq=seq, exclude=exclude, ldr=C + 3)
        assert status == 0
        for u in range(U):
            live = ref.live_ref(pos[u], M, item_id, seq[u], exclude)
            steps += _check_user(x64, pos[u], rel[u], live, lam, K, got, u, D, item_id)
            if exclude:
                picked = got["item"][u][got["slot"][u] >= 0]
                assert 0 not in picked and not np.isin(picked, seq[u][seq[u] != 0]).any()
    assert steps > 0 or C <= 2


# ---------------------------------------------------------------------------------------- 3. bit equalities
def _recommender(d, dev, **kw):
    return Recommender(_state(d), _cfg(d), _catalogue(), device=dev, **kw)


@functools.lru_cache(maxsize=None)
def _users(n=40):
    """n histories of catalogue ids with some padding; rows 0..2 are _histories()' (row 0 all padding)."""
    ids = _catalogue()["item_id"]
    g = torch.Generator().manual_seed(27)
    more = ids[torch.randint(0, M_CAT, (n - 3, L_HIST), generator=g)]
    more[torch.rand((n - 3, L_HIST), generator=g) < 0.3] = 0
    return torch.cat([_histories(), more])


def test_lam_one_on_logits_is_topk_lists(hip_device):
    dev = hip_device
    rec = _recommender(16, dev)
    seq = _users(8)
    g = torch.Generator().manual_seed(3)
    cands = torch.randint(0, M_CAT, (8, 300), generator=g)
    cands[torch.rand((8, 300), generator=g) < 0.1] = -1
    for k in (1, 10, 256):
        for exclude in (True, False):
            top = rec.topk_lists(seq, cands, k, by="index", exclude_history=exclude)
            div = rec.diversify(seq, cands, k, lam=1.0, relevance="logit", by="index", exclude_history=exclude)
            for a, b in (("slot", "slot"), ("index", "index"), ("item_id", "item_id"), ("logit", "relevance")):
                assert torch.equal(top[a], div[b]), (k, exclude, a)
    assert int(rec.status.item()) == 0
    rec.check_ids()


def test_a_user_does_not_depend_on_the_others_and_penalties_are_knn_scores(hip_device):
    dev, D, C, K, U = hip_device, 128, 257, 64, 33
    M, pos, rel, item_id, seq = _random_lists(D, C, U, 5)
    xn = _unit_rows(dev, M, D, 9)
    together, _ = _mmr(dev, rel, pos, xn, item_id, 0.6, K, seq=seq, exclude=True)
    for u in range(U):
        alone, _ = _mmr(dev, rel[u:u + 1], pos[u:u + 1], xn, item_id, 0.6, K, seq=seq[u:u + 1], exclude=True)
        for n in OUT_INT + OUT_F32:
            assert np.array_equal(alone[n][0], together[n][u]), (u, n)
    # out_pen[t] is the largest fbn_knn_scores entry between pick t and the picks before it, bit for bit
    for u in (1, 17):
        picks = together["index"][u]
        n = int((picks >= 0).sum())
        assert n > 8
        q_pos = torch.from_numpy(picks[:n]).to(dev)
        S = torch.full((n * M,), float("nan"), dtype=torch.float32, device=dev)
        call("fbn_knn_scores", None, D, ptr(q_pos), ptr(xn), M, n, 0, M, D, ptr(S), _lib.stream_handle(dev))
        G = S.view(n, M)[:, q_pos]                                   # [s, t] = <pick s, pick t>
        assert torch.equal(G, G.t())
        want = torch.stack([G[:t, t].max() for t in range(1, n)]).cpu().numpy()
        assert np.array_equal(together["pen"][u][1:n], want) and together["pen"][u][0] == 0


# ---------------------------------------------------------------------------------------- 4. NaN
def test_a_nan_relevance_is_picked_last_and_flags_only_a_live_slot(hip_device):
    dev, D, C, K = hip_device, 16, 65, 65
    M, pos, rel, item_id, seq = _random_lists(D, C, 2, 44)
    pos, rel = pos[1:], rel[1:]                                      # (user 0's list is mostly empty)
    xn = _unit_rows(dev, M, D, 4)
    live = ref.live_ref(pos[0], M)
    dead, alive = int(np.flatnonzero(~live)[0]), int(np.flatnonzero(live)[5])
    rel_dead = rel.copy()
    rel_dead[0, dead] = np.nan                                       # a NaN in an empty slot sets nothing
    got, status = _mmr(dev, rel_dead, pos, xn, item_id, 0.5, K)
    assert status == 0 and dead not in got["slot"][0]
    rel_live = rel.copy()
    rel_live[0, alive] = np.nan
    got, status = _mmr(dev, rel_live, pos, xn, item_id, 0.5, K)
    n = int(live.sum())
    assert status & 1
    assert got["slot"][0][n - 1] == alive and np.isnan(got["rel"][0][n - 1]) and np.isnan(got["mmr"][0][n - 1])
    assert (got["slot"][0][n:] == -1).all() and sorted(got["slot"][0][:n].tolist()) == np.flatnonzero(live).tolist()
    # the steps before it are those of the list without that slot
    rel_without, live_without = np.nan_to_num(rel_live[0]), live.copy()
    live_without[alive] = False
    tol = ref.tol_mmr(D, 0.5, 1.0)
    ref.mmr_conditional_check(xn.double().cpu().numpy(), pos[0], rel_without, live_without, 0.5, n - 1,
                              got["slot"][0][:n - 1], got["mmr"][0][:n - 1], got["pen"][0][:n - 1], tol, tol_scores(D))


# ---------------------------------------------------------------------------------------- 5. ILD
@pytest.mark.parametrize("D", [16, 128, 256])
def test_list_ild_against_float64(hip_device, D):
    dev, M = hip_device, 300
    xn = _unit_rows(dev, M, D, 70 + D)
    x64 = xn.double().cpu().numpy()
    rng = np.random.default_rng(D)
    for K in (1, 2, 10, 256):
        lists = rng.integers(0, M, size=(7, K))
        lists[rng.random((7, K)) < 0.15] = -1
        lists[1, :] = 11                                             # one item repeated
        lists[2, :] = -1                                             # an empty list
        lists[3, K // 2] = M + 1                                     # outside the catalogue: not an entry
        if K > 2:
            lists[4, 1:] = -1                                        # a single live entry
            lists[4, 0] = 5
            lists[5, 0] = 2                                          # the zero row
        ild, n_pairs = _ild(dev, lists, xn, ldp=K + 2)
        again, n_again = _ild(dev, lists, xn, ldp=K + 2)
        assert torch.equal(ild, again) and torch.equal(n_pairs, n_again)         # equal bits
        ild, n_pairs = ild.cpu().numpy(), n_pairs.cpu().numpy()
        for u in range(7):
            want, pairs = ref.ild_ref(x64, lists[u])
            assert n_pairs[u] == pairs, (K, u)
            assert abs(ild[u] - want) <= tol_scores(D), (K, u, ild[u], want)
        assert abs(ild[1]) <= tol_scores(D) and n_pairs[1] == K * (K - 1) // 2
        assert ild[2] == 0 and n_pairs[2] == 0


# ---------------------------------------------------------------------------------------- 6. the methods
def _space_rows(rec, space):
    """float64 copy of the device's own normalised rows of a space: the kernel's operands."""
    with torch.cuda.device(rec.device):
        return rec._space(space, _lib.stream_handle(rec.device)).double().cpu().numpy()


def _judge_method(rec, out, seq, cands, rel, lam, k, space, exclude=True):
    """Recommender.diversify's dict through the conditional check, user by user -> the lists as numpy."""
    xe = _space_rows(rec, space)
    D = xe.shape[1]
    ids = rec.cat["item_id"].cpu().numpy()
    got = {"slot": out["slot"], "index": out["index"], "item": out["item_id"], "rel": out["relevance"],
           "mmr": out["mmr"], "pen": out["penalty"]}
    got = {n: v.cpu().numpy() for n, v in got.items()}
    pos, rel = cands.cpu().numpy(), rel.cpu().numpy()
    for u in range(pos.shape[0]):
        live = ref.live_ref(pos[u], rec.M, ids, None if seq is None else seq[u].numpy(), exclude)
        _check_user(xe, pos[u], rel[u], live, lam, k, got, u, D, ids)
    return got


@pytest.mark.parametrize("space,d", [("content", 16), ("id", 16), ("mm", 128)])
def test_diversify_in_every_space(hip_device, space, d):
    dev = hip_device
    rec = _recommender(d, dev)
    seq = _users(8)
    g = torch.Generator().manual_seed(d)
    cands_pos = torch.randint(0, M_CAT, (8, 200), generator=g)
    cands_pos[torch.rand((8, 200), generator=g) < 0.1] = -1
    for relevance in ("prob", "logit"):
        rel = rec.score_lists(seq, cands_pos, by="index", logits=relevance == "logit")
        rel = torch.where(cands_pos.to(dev) >= 0, rel, torch.zeros_like(rel))
        out = rec.diversify(seq, cands_pos, 10, lam=0.7, space=space, relevance=relevance, by="index")
        _judge_method(rec, out, seq, cands_pos, rel, 0.7, 10, space)
        given = rec.diversify(seq, cands_pos, 10, lam=0.7, space=space, relevance=rel, by="index")
        assert all(torch.equal(out[n], given[n]) for n in out)
    # by item id, and the cold user
    ids = rec.cat["item_id"].cpu()
    by_id = rec.diversify(seq, torch.where(cands_pos >= 0, ids[cands_pos.clamp(min=0)], torch.full_like(cands_pos, 4999)),
                          10, lam=0.7, space=space, relevance="logit")
    assert all(torch.equal(out[n], by_id[n]) for n in out)
    cold = rec.diversify(None, cands_pos[:1], 10, lam=0.5, space=space, by="index")
    rel = rec.score_lists(None, cands_pos[:1], by="index")
    _judge_method(rec, cold, None, cands_pos[:1], rel, 0.5, 10, space)
    assert int(rec.status.item()) == 0
    rec.check_ids()


def test_recommend_without_lam_is_unchanged_and_with_lam_is_retrieve_then_diversify(hip_device):
    dev = hip_device
    rec = _recommender(16, dev)
    seq = _users(8)
    for space in ("content", "id"):
        cands = rec.retrieve(seq, 200, space=space)["index"]
        plain = rec.recommend(seq, 10, space=space)
        want = rec.topk_lists(seq, cands, 10, by="index")
        assert set(plain) == set(want) == {"slot", "index", "item_id", "logit", "prob"}
        assert all(torch.equal(plain[n], want[n]) for n in want)
        none = rec.recommend(seq, 10, space=space, lam=None)
        assert all(torch.equal(plain[n], none[n]) for n in want)
        div = rec.recommend(seq, 10, space=space, lam=0.7)
        want = rec.diversify(seq, cands, 10, lam=0.7, space=space, by="index")
        assert set(div) == {"slot", "index", "item_id", "relevance", "mmr", "penalty"}
        assert all(torch.equal(div[n], want[n]) for n in want)
        assert (div["index"][0] == -1).all()                          # no usable history: an empty row
    rec.check_ids()


def test_evaluate_diversity_is_hits_and_ild_by_hand(hip_device):
    dev, space, k, n_cand = hip_device, "content", 10, 200
    rec = _recommender(16, dev)
    seqs = _users(40)
    ids = rec.cat["item_id"].cpu().numpy()
    # held-out items: somewhere in (or just behind) the user's undiversified top 12, so that hits occur
    cands = rec.retrieve(seqs, n_cand, space=space)["index"]
    top = rec.topk_lists(seqs, cands, 12, by="index")["item_id"].cpu()
    tgt = torch.stack([top[u, (5 * u) % 12] for u in range(40)])
    tgt[0], tgt[7] = 4998, 4999                                       # no list / not in the catalogue
    labels = torch.ones(80)
    labels[1::2] = 0                                                  # the negatives in between are not users
    batch = {"item_seq": seqs.repeat_interleave(2, dim=0), "item_id": tgt.repeat_interleave(2)}
    pairs = [({n: v[:30] for n, v in batch.items()}, labels[:30]), ({n: v[30:] for n, v in batch.items()}, labels[30:])]
    lams = (1.0, 0.7, 0.5)
    got = rec.evaluate_diversity(pairs, k, lams, n_candidates=n_cand, space=space, users_per_block=16)

    # by hand, over the blocks evaluate_diversity forms: 15 users of the first batch, 16 + 9 of the second
    xe = _space_rows(rec, space)
    D = xe.shape[1]
    blocks = [(0, 15), (15, 31), (31, 40)]
    cands = torch.cat([rec.retrieve(seqs[a:b], n_cand, space=space)["index"] for a, b in blocks])
    rel = torch.cat([rec.score_lists(seqs[a:b], cands[a:b], by="index") for a, b in blocks])
    ref_ild, same = {}, 0
    for lam in lams:
        out = rec.diversify(seqs, cands, k, lam=lam, space=space, relevance=rel, by="index")
        lists = _judge_method(rec, out, seqs, cands, rel, lam, k, space)
        hits, ilds, exact_ilds = 0, [], []
        for u in range(40):
            hits += int(tgt[u]) in lists["item"][u][lists["index"][u] >= 0].tolist()
            ild, pairs_u = ref.ild_ref(xe, lists["index"][u])
            if pairs_u:
                ilds.append(ild)
            live = ref.live_ref(cands[u].cpu().numpy(), rec.M, ids, seqs[u].numpy(), True)
            slot = ref.mmr_ref(xe, cands[u].cpu().numpy(), rel[u].cpu().numpy(), live, lam, k)[0]
            same += int(np.array_equal(slot, lists["slot"][u]))
            exact = ref.ild_ref(xe, np.where(slot >= 0, cands[u].cpu().numpy()[np.clip(slot, 0, None)], -1))
            if exact[1]:
                exact_ilds.append(exact[0])
        ref_ild[lam] = float(np.mean(exact_ilds))
        assert got[lam]["n"] == 40 and got[lam]["n_ild"] == len(ilds) == 39
        assert got[lam]["hr"] == {k: hits / 40}
        assert abs(got[lam]["ild"] - np.mean(ilds)) <= tol_scores(D)
    print(f"{same} of {40 * len(lams)} device lists are the float64 greedy lists; reference ILD {ref_ild}")
    assert 0 < got[1.0]["hr"][k] < 1

    # lam = 1 is the undiversified list: the hit rate of retrieve + topk_lists over the same users
    top10 = [rec.topk_lists(seqs[a:b], cands[a:b], k, by="index") for a, b in blocks]
    item, index = (torch.cat([t[n] for t in top10]).cpu() for n in ("item_id", "index"))
    hit = ((item == tgt[:, None]) & (index >= 0)).any(dim=1)
    one = rec.evaluate_diversity(pairs, k, (1.0,), n_candidates=n_cand, space=space, users_per_block=16)
    assert one[1.0]["hr"][k] == hit.sum().item() / 40 == got[1.0]["hr"][k]
    # diversity does not fall as lam does -- asserted because the float64 reference shows it on this catalogue
    assert ref_ild[0.5] >= ref_ild[1.0]
    assert got[0.5]["ild"] >= got[1.0]["ild"] - tol_scores(D)
    rec.check_ids()
