"""Rank evaluation (fbn_rec_rank, fbn_rank_hist, Recommender.rank / positions / evaluate, RankMetrics) on
an MI355X: pytest -m gpu.

The reference of every rank is numpy on the documented 64-bit keys {ordered image of the f32 logit,
0xFFFFFFFF - position}: integers, so every comparison is exact.  Kernel shapes: U = 5 users per call,
M = 2500 (segments of 1024, 1024 and 452 candidates), ld = M + 3, L = 20.  Recommender shapes are those of
tests/test_gpu_recommend.py (M = 1037, its three histories), each history repeated over nine targets.
"""
import functools

import numpy as np
import pytest
import torch

from ctr_recommendation_amd import _lib
from ctr_recommendation_amd._lib import call, ptr
from ctr_recommendation_amd.rank_metrics import RankMetrics, rank_metrics_from_record
from test_gpu_recommend import L_HIST, M_CAT, U_HIST, V_SMALL, _catalogue, _excluded, _histories, _rec

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------- the key reference
def _keys(logits):
    """uint64 keys of an f32 array [..., M] (include/fibinet.h: fbn_rec_topk)."""
    b = np.ascontiguousarray(logits, dtype=np.float32).view(np.uint32)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    o = np.where(nan, np.uint32(1), np.where((b & np.uint32(0x80000000)) != 0, ~b, b | np.uint32(0x80000000)))
    pos = np.uint64(0xFFFFFFFF) - np.arange(b.shape[-1], dtype=np.uint64)
    return (o.astype(np.uint64) << np.uint64(32)) | pos


def _ref_rank(logits, ids, seq, tpos, exclude):
    """(rank, n_eligible) int32 [U] by counting keys; seq None: no history."""
    logits, ids = np.asarray(logits, dtype=np.float32), np.asarray(ids)
    U, M = logits.shape
    keys, at = _keys(logits), np.arange(M)
    rank, nel = np.zeros(U, dtype=np.int32), np.zeros(U, dtype=np.int32)
    for u in range(U):
        t = int(tpos[u])
        elig = np.ones(M, dtype=bool)
        if exclude:
            hist = [int(s) for s in (seq[u] if seq is not None else []) if s != 0]
            elig = (ids != 0) & (~np.isin(ids, hist) | (at == t))
        nel[u] = elig.sum()
        if 0 <= t < M and ids[t] != 0:
            rank[u] = 1 + int((elig & (at != t) & (keys[u] > keys[u, t])).sum())
    return rank, nel


def test_key_reference_orders_as_documented():
    x = np.array([[np.nan, -np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, 1.0]], dtype=np.float32)
    k = _keys(x)[0]
    assert list(np.argsort(k)) == [0, 1, 2, 3, 4, 7, 5, 6]      # equal logits: the smaller position is above


# ---------------------------------------------------------------------------------------- 1. the kernel
K_U, K_M, K_LD, K_L = 5, 2500, 2503, 20
K_VALUES = np.array([np.inf, -np.inf, -0.0, 0.0, 1.5, -2.25, 1e-3], dtype=np.float32)
PAD_POS, DUP_SRC, DUP_POS = 17, 45, 2000


@functools.lru_cache(maxsize=None)
def _kernel_inputs():
    rng = np.random.default_rng(31)
    ids = (1 + rng.permutation(90000)[:K_M]).astype(np.int64)
    ids[PAD_POS] = 0                                     # one padding item
    ids[DUP_POS] = ids[DUP_SRC]                          # one repeated id (in user 1's history)
    hists = np.zeros((3, K_L), dtype=np.int64)          # all padding / full / repeats with interior zeros
    hists[1] = ids[40:60]
    a, b, c = ids[3], ids[1024], ids[2499]
    hists[2] = [0, a, a, 0, b, 0, 0, a, c, c, 0, b, 99999, 0, a, 0, 0, c, 0, b]       # 99999: not in the catalogue
    in_hist = (DUP_POS, DUP_SRC, 1024)                   # a target inside the user's own history (user 0 has none)
    seq, tpos = [], []
    for h in range(3):
        for t in (0, 1023, 1024, 2499, in_hist[h], PAD_POS, -1, K_M):
            seq.append(hists[h])
            tpos.append(t)
    seq, tpos = np.stack(seq), np.array(tpos, dtype=np.int64)
    logits = np.full((len(tpos), K_LD), np.inf, dtype=np.float32)       # the 3 columns past M are never candidates
    logits[:, :K_M] = K_VALUES[rng.integers(0, len(K_VALUES), size=(len(tpos), K_M))]
    return ids, seq, tpos, logits


def _run_kernel(dev, logits, ids, seq, tpos, exclude):
    """fbn_rec_rank on the rows, K_U users per call; -> rank, n_eligible (cpu), status."""
    st = _lib.stream_handle(dev)
    ids_d = torch.from_numpy(ids).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ranks, nels = [], []
    for r0 in range(0, len(tpos), K_U):
        lg = torch.from_numpy(logits[r0:r0 + K_U]).to(dev).contiguous()
        sq = torch.from_numpy(seq[r0:r0 + K_U]).to(dev).contiguous()
        tp = torch.from_numpy(tpos[r0:r0 + K_U]).to(dev).contiguous()
        U = lg.shape[0]
        rank = torch.full((U,), 77, dtype=torch.int32, device=dev)          # the call initialises its outputs
        nel = torch.full((U,), 77, dtype=torch.int32, device=dev)
        call("fbn_rec_rank", ptr(lg), K_LD, U, K_M, ptr(ids_d), ptr(sq), K_L, int(exclude), ptr(tp), ptr(rank),
             ptr(nel), ptr(status), st)
        ranks.append(rank)
        nels.append(nel)
    return torch.cat(ranks).cpu(), torch.cat(nels).cpu(), int(status.item())


@pytest.mark.parametrize("exclude", [1, 0])
def test_rank_kernel_equals_the_key_count(hip_device, exclude):
    ids, seq, tpos, logits = _kernel_inputs()
    want_rank, want_nel = _ref_rank(logits[:, :K_M], ids, seq, tpos, exclude)
    rank, nel, status = _run_kernel(hip_device, logits, ids, seq, tpos, exclude)
    assert torch.equal(rank, torch.from_numpy(want_rank)), (rank.tolist(), want_rank.tolist())
    assert torch.equal(nel, torch.from_numpy(want_nel)), (nel.tolist(), want_nel.tolist())
    assert status == 0
    # the inputs do what they are there for
    not_ranked = np.isin(tpos, (PAD_POS, -1, K_M))
    assert (want_rank[not_ranked] == 0).all() and (want_rank[~not_ranked] >= 1).all()
    assert len(set(want_rank[~not_ranked].tolist())) > 5                  # ties everywhere, yet no flat answer
    if exclude:
        assert want_nel[0] == K_M - 1 and want_nel[8] == K_M - 1 - 21     # padding; + 20 history ids, one twice
        assert want_nel[8 + 4] == want_nel[8] + 1                          # a history target stays eligible
    else:
        assert (want_nel == K_M).all()


@pytest.mark.parametrize("exclude", [1, 0])
def test_rank_kernel_nan_ranks_below_minus_inf(hip_device, exclude):
    ids, seq, tpos, logits = _kernel_inputs()
    far = logits.copy()
    far[2, 300] = np.nan                                 # row 2's target is 1024: a NaN elsewhere
    rank, nel, status = _run_kernel(hip_device, far, ids, seq, tpos, exclude)
    want_rank, want_nel = _ref_rank(far[:, :K_M], ids, seq, tpos, exclude)
    assert torch.equal(rank, torch.from_numpy(want_rank)) and torch.equal(nel, torch.from_numpy(want_nel))
    assert status == 0                                   # only a NaN at a target is reported
    both = far.copy()
    both[1, 1023] = np.nan                               # row 1's own target
    rank, nel, status = _run_kernel(hip_device, both, ids, seq, tpos, exclude)
    want_rank, want_nel = _ref_rank(both[:, :K_M], ids, seq, tpos, exclude)
    assert torch.equal(rank, torch.from_numpy(want_rank)) and torch.equal(nel, torch.from_numpy(want_nel))
    assert status == 1
    assert want_rank[1] == want_nel[1]                   # the NaN target is last among the eligible


# ---------------------------------------------------------------------------------------- 2. against topk
CHUNKED = U_HIST * 400
# 17: the catalogue's padding item.  Position 1036 is an item of the third history (its id `c`), so with
# exclusion on only 17 of the 24 rows over the first seven positions have a target topk may return; position
# 1035, in no history, brings the checked rows to 20 of 27.
TARGET_POS = (0, 399, 400, 1023, 1024, 1036, 17, 1035)
N_ROWS = U_HIST * (len(TARGET_POS) + 1)
SINGLE = N_ROWS * M_CAT
MODES = [(16, "fp32"), (128, "fp32"), (128, "bf16")]


@functools.lru_cache(maxsize=None)
def _rows():
    """27 evaluation users: each history over the eight positions and one item of that history (the
    all-padding history's only item is the padding id).  -> seq [27, 20], target ids [27]."""
    ids, hist = _catalogue()["item_id"], _histories()
    own = (0, int(hist[1, 0]), int(hist[2, 1]))
    seq, tgt = [], []
    for u in range(U_HIST):
        for t in [int(ids[p]) for p in TARGET_POS] + [own[u]]:
            seq.append(hist[u])
            tgt.append(t)
    return torch.stack(seq), torch.tensor(tgt, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _ranked(dev, d, mode, chunk_rows):
    """Recommender + the ranks of the 27 rows under both flags, computed once per configuration."""
    rec = _rec(d, dev, chunk_rows, mode=mode)
    seq, tgt = _rows()
    seq, tgt = seq.to(dev), tgt.to(dev)
    out = {ex: {k: v.clone() for k, v in rec.rank(seq, tgt, exclude_history=ex).items()} for ex in (True, False)}
    return rec, out


@pytest.mark.parametrize("chunk_rows", [CHUNKED, SINGLE])
@pytest.mark.parametrize("d,mode", MODES)
def test_rank_is_the_place_topk_gives(hip_device, d, mode, chunk_rows):
    dev = hip_device
    rec, ranked = _ranked(dev, d, mode, chunk_rows)
    seq, tgt = _rows()
    cat_ids = _catalogue()["item_id"]
    tpos = rec.positions(tgt).cpu()
    assert tpos.dtype == torch.int64 and (tpos >= 0).all()
    assert tpos.tolist() == [cat_ids.tolist().index(int(t)) for t in tgt]
    in_hist = torch.tensor([bool(_excluded(cat_ids, seq[r])[tpos[r]]) and int(tgt[r]) != 0 for r in range(N_ROWS)])
    padding = tgt == 0
    assert int(padding.sum()) == 4 and int(in_hist.sum()) == 3
    scores = rec.score(seq.to(dev), logits=True).cpu().numpy()          # the same sweep shape: the same bits
    for exclude in (True, False):
        rank, nel = ranked[exclude]["rank"].cpu(), ranked[exclude]["n_eligible"].cpu()
        assert rank.dtype == torch.int32 and nel.dtype == torch.int32 and rank.shape == (N_ROWS,)
        want_rank, want_nel = _ref_rank(scores, cat_ids.numpy(), seq.numpy(), tpos.numpy(), exclude)
        assert torch.equal(rank, torch.from_numpy(want_rank)), (exclude, rank.tolist(), want_rank.tolist())
        assert torch.equal(nel, torch.from_numpy(want_nel)), (exclude, nel.tolist(), want_nel.tolist())
        assert (rank[padding] == 0).all()                                 # the padding target is not ranked
        assert (rank[in_hist] >= 1).all()                                 # a history target is, under both flags
        # rows whose target topk may return: not the padding item, and not a history item when those are excluded
        rows = [r for r in range(N_ROWS) if not padding[r] and not (exclude and in_hist[r])]
        assert len(rows) == (20 if exclude else 23)
        for k in (1, 10, 256):
            index = rec.topk(seq.to(dev), k, exclude_history=exclude)["index"].cpu()
            for r in rows:
                listed = index[r].tolist()
                assert (int(rank[r]) <= k) == (int(tpos[r]) in listed), (exclude, k, r, int(rank[r]))
                if int(tpos[r]) in listed:
                    assert listed.index(int(tpos[r])) == int(rank[r]) - 1, (exclude, k, r)
    assert len(set(ranked[True]["rank"].tolist())) > 8                    # a ranking, not one flat answer
    assert int(rec.status.item()) == 0
    rec.check_ids()


def test_rank_by_index_and_cold_user(hip_device):
    dev = hip_device
    rec, ranked = _ranked(dev, 16, "fp32", CHUNKED)
    seq, tgt = _rows()
    by_index = rec.rank(seq.to(dev), rec.positions(tgt), by="index")
    assert torch.equal(by_index["rank"], ranked[True]["rank"])
    assert torch.equal(by_index["n_eligible"], ranked[True]["n_eligible"])
    cold = rec.rank(None, torch.tensor([int(tgt[1])]))
    scores = rec.score(None, logits=True).cpu().numpy()
    tpos = rec.positions(tgt[1:2]).cpu().numpy()
    want_rank, _ = _ref_rank(scores, _catalogue()["item_id"].numpy(), None, tpos, True)
    assert cold["rank"].tolist() == want_rank.tolist() and cold["n_eligible"].tolist() == [M_CAT - 1]
    with pytest.raises(ValueError):
        rec.rank(seq.to(dev), tgt[:5])
    with pytest.raises(ValueError):
        rec.rank(seq.to(dev), tgt, by="name")


# ---------------------------------------------------------------------------------------- 3. tie rule
@pytest.mark.parametrize("d", [16, 128])
def test_tied_items_take_consecutive_ranks_in_position_order(hip_device, d):
    dev = hip_device
    hist = _histories().to(dev)
    base = _rec(d, dev, U_HIST * M_CAT).score(hist, logits=True)
    best = int(base[1].argmax().item())                 # user 1's best row, copied into rows 5, 400 and 1030
    cat = {k: v.clone() for k, v in _catalogue().items()}
    for k in cat:
        for r in (5, 400, 1030):
            cat[k][r] = cat[k][best]
    ties = sorted({best, 5, 400, 1030})
    seq = hist.repeat_interleave(len(ties), dim=0)      # every user over the four tied positions
    tpos = torch.tensor(ties * U_HIST, device=dev)
    seen = []
    for chunk_rows in (CHUNKED, seq.shape[0] * M_CAT, U_HIST * 97):
        rank = _rec(d, dev, chunk_rows, cat=cat).rank(seq, tpos, exclude_history=False, by="index")["rank"].cpu()
        rank = rank.view(U_HIST, len(ties))
        assert rank[1].tolist() == list(range(1, len(ties) + 1)), (chunk_rows, rank.tolist())
        for u in range(U_HIST):
            assert rank[u].tolist() == list(range(int(rank[u, 0]), int(rank[u, 0]) + len(ties))), (chunk_rows, u)
        seen.append(rank)
    assert torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2])


# ---------------------------------------------------------------------------------------- 4. the record, evaluate
def _record(ranks):
    ranks = np.asarray(ranks, dtype=np.int64)
    rec = np.zeros(260, dtype=np.uint64)
    rec[:258] = np.bincount(np.where(ranks < 1, 0, np.minimum(ranks, 257)), minlength=258)
    rec[258] = ranks[ranks >= 1].sum()
    rec[259] = (ranks >= 1).sum()
    return rec


def test_rank_metrics_record_is_the_bincount(hip_device):
    dev = hip_device
    _, ranked = _ranked(dev, 16, "fp32", CHUNKED)
    rank = ranked[True]["rank"]
    hand = torch.tensor([0, 1, 256, 257, 100000], dtype=torch.int32, device=dev)
    m = RankMetrics(dev)
    m.update(rank[:7])
    m.update(rank[7:])
    m.update(hand)
    want = _record(rank.cpu().tolist() + hand.cpu().tolist())
    got = m.record()
    assert got.dtype == np.uint64 and got.shape == (260,)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert m.compute((1, 10, 256)) == rank_metrics_from_record(want, (1, 10, 256))
    assert m.compute((1, 10, 256))["n"] == int((rank > 0).sum()) + 4 and m.compute()["n_skipped"] == 5
    with pytest.raises(ValueError):
        m.compute((0,))
    with pytest.raises(ValueError):
        m.compute((257,))
    m.update(torch.tensor([-5], dtype=torch.int32, device=dev))           # a negative rank is "not ranked"
    assert int(m.record()[0]) == 6 and int(m.record()[259]) == int(want[259])
    m.reset()
    assert not m.record().any()
    # more ranks than one workgroup takes at a time, every bin hit
    many = torch.from_numpy(np.random.default_rng(5).integers(-2, 400, size=70001).astype(np.int32)).to(dev)
    m.update(many)
    assert np.array_equal(m.record(), _record(many.cpu().numpy()))


def test_evaluate_equals_rank_update_compute(hip_device):
    dev = hip_device
    rec, ranked = _ranked(dev, 16, "fp32", CHUNKED)
    seq, tgt = _rows()
    ks = (1, 10, 256)

    def expected(n):
        m = RankMetrics(dev)
        m.update(rec.rank(seq[:n].to(dev), tgt[:n].to(dev))["rank"])
        return m.compute(ks)

    # two batches with mixed labels whose positive rows are the 27 users, in order
    g = torch.Generator().manual_seed(9)
    cat_ids = _catalogue()["item_id"]
    pairs, r0 = [], 0
    for n_pos, n_rows in ((14, 23), (13, 31)):
        labels = torch.zeros(n_rows)
        labels[torch.randperm(n_rows, generator=g)[:n_pos]] = 1.0
        b_seq = cat_ids[torch.randint(0, M_CAT, (n_rows, L_HIST), generator=g)]
        b_item = cat_ids[torch.randint(0, M_CAT, (n_rows,), generator=g)]
        at = labels.nonzero().reshape(-1)
        b_seq[at], b_item[at] = seq[r0:r0 + n_pos], tgt[r0:r0 + n_pos]
        r0 += n_pos
        pairs.append(({"item_seq": b_seq.to(dev), "item_id": b_item.to(dev)}, labels.to(dev)))
    want = expected(N_ROWS)
    assert want["n"] == 23 and want["n_skipped"] == 4        # 3 padding targets + the all-padding user's own
    assert rec.evaluate(pairs, ks, users_per_block=5) == want
    assert rec.evaluate(pairs, ks) == want
    assert rec.evaluate(iter(pairs), ks, max_users=7) == expected(7)
    off = rec.evaluate(pairs, ks, exclude_history=False)
    assert off["n"] == 23 and off["mean_rank"] >= want["mean_rank"]
    assert sorted(rec.evaluate(pairs)["hr"]) == [5, 10, 20]


# ---------------------------------------------------------------------------------------- 5. ids
def test_positions_and_out_of_table_ids(hip_device):
    dev = hip_device
    cat = {k: v.clone() for k, v in _catalogue().items()}
    cat["item_id"][900] = cat["item_id"][30]                             # a repeated id: the smaller position wins
    rec = _rec(16, dev, CHUNKED, cat=cat)
    ids = cat["item_id"]
    assert 4999 not in ids.tolist()
    q = torch.tensor([4999, V_SMALL + 10, -3, int(ids[30]), int(ids[900]), int(ids[899]), 0, V_SMALL])
    want = [-1, -1, -1, 30, 30, 899, 17, -1]
    got = rec.positions(q.to(dev))
    assert got.dtype == torch.int64 and got.tolist() == want
    assert rec.positions(q.view(2, 4)).tolist() == [want[:4], want[4:]]
    seq = _histories().to(dev)
    out = rec.rank(seq, torch.tensor([V_SMALL + 10, -3, 4999]))
    torch.cuda.synchronize()
    assert out["rank"].tolist() == [0, 0, 0]
    assert out["n_eligible"].tolist() == [int((~_excluded(ids, s)).sum()) for s in _histories()]
    rec.check_ids()                                                      # a bad target id is no table access
    bad = seq.clone()
    bad[1, 4] = V_SMALL
    rec.rank(bad, ids[:3])
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        rec.check_ids()
