"""Per-user candidate lists (fbn_rec_fields_list, fbn_rec_topk_list, fbn_rec_rank_list and Recommender's
score_lists / topk_lists / rank_lists / evaluate_sampled) on an MI355X: pytest -m gpu.

The reference of every selection and rank is numpy on the documented 64-bit keys {ordered image of the
f32 logit, 0xFFFFFFFF - slot}: integers, so every comparison is exact.  Kernel shapes: the catalogue of
tests/test_gpu_recommend.py (M = 1037, its three histories), U = 5 lists of C = 1100 slots (segments of
1024 and 76), ldp = 1103, chunks of 400 / 400 / 300 slots with the carry; the fields kernel on U = 3
lists of C = 150 slots, ldp = 152, in two calls (100 + 50 slots).  Recommender shapes: C = 300 slots per
user in chunks of 128 / 128 / 44 and in one chunk.
"""
import functools

import numpy as np
import pytest
import torch

from ctr_recommendation_amd import _lib, ops
from ctr_recommendation_amd._lib import call, ptr
from ctr_recommendation_amd.rank_metrics import RankMetrics
from test_gpu_rank_eval import K_VALUES, _keys, _rows
from test_gpu_recommend import (FP32_BOUND, L_HIST, M_CAT, U_HIST, V_SMALL, _catalogue, _histories, _oracle_logits,
                                _project_forward, _rec, _state, _to)
from test_gpu_recommend import CHUNKED as CAT_CHUNKED, SINGLE as CAT_SINGLE

pytestmark = pytest.mark.gpu

PAD_POS = 17                     # the catalogue's padding item (_catalogue)
HIST_POS = (45, 45, 500, 45, 500)   # per list of the kernel tests: a position whose id is in that user's history
                                    # (histories 1 and 2; list 0's history is all padding, so 45 is an ordinary item)


def _same(a, b):
    """torch.equal with NaN == NaN (the infinities stay distinct from every number)."""
    if a.is_floating_point():
        a, b = torch.nan_to_num(a, nan=123.0), torch.nan_to_num(b, nan=123.0)
    return a.dtype == b.dtype and torch.equal(a, b)


# ---------------------------------------------------------------------------------------- 1. fields
F_C, F_LDP = 150, 152


@functools.lru_cache(maxsize=None)
def _field_lists():
    rng = np.random.default_rng(41)
    pos = np.full((U_HIST, F_LDP), -7, dtype=np.int64)            # the two columns past C are never read
    pos[0, :F_C] = rng.permutation(M_CAT)[:F_C]                     # a permutation prefix
    pos[1, :F_C] = rng.integers(0, M_CAT, size=F_C)
    pos[1, [0, 60, 99, 100, 149]] = [0, M_CAT - 1, PAD_POS, 0, 333]  # both ends, the padding item, position 0 twice
    pos[1, 101] = 333                                               # ... and 333 twice, across the two calls
    pos[2, :F_C] = rng.integers(0, M_CAT, size=F_C)
    pos[2, [5, 60, 99, 100]] = -1                                   # interior empty slots, on both sides of the cut
    pos[2, 120:F_C] = -1                                            # an empty tail
    pos[2, 7] = -12345                                              # any negative value is an empty slot
    return pos


@pytest.mark.parametrize("d", [16, 128])
def test_list_fields_are_the_bits_of_the_catalogue_fields(hip_device, d):
    dev = hip_device
    cat, seq = _to(_catalogue(), dev), _histories().to(dev)
    p = {k: v.to(dev).contiguous() for k, v in _state(d).items()}
    M, U, R = M_CAT, U_HIST, int(p["senet.excitation.0.weight"].shape[0])
    st = _lib.stream_handle(dev)
    hmm = torch.empty((M, d), device=dev)
    ops.gemm(cat["item_emb_d128"], p["mm_proj.0.weight"], hmm, M, d, 128, 128, 128, d, False, True,
             bias=p["mm_proj.0.bias"], stream=st)
    n_cate = p["cate_emb.weight"].shape[0]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    cache, hist = torch.empty((M, d), device=dev), torch.empty((U, d), device=dev)
    call("fbn_rec_item_cache", ptr(cat["item_id"]), ptr(cat["likes_level"]), ptr(cat["views_level"]), ptr(hmm),
         ptr(p["mm_proj.1.weight"]), ptr(p["mm_proj.1.bias"]), ops.LN_EPS, n_cate, V_SMALL, ptr(cache), ptr(err), M, d, st)
    call("fbn_rec_hist_pool", ptr(seq), ptr(p["item_emb.weight"]), V_SMALL, ptr(hist), ptr(err), U, L_HIST, d, st)
    head = [ptr(cat["item_id"]), ptr(cat["likes_level"]), ptr(cat["views_level"]), ptr(cache), ptr(hist),
            ptr(p["cate_emb.weight"]), n_cate, ptr(p["item_emb.weight"]), V_SMALL, ptr(p["senet.excitation.0.weight"]),
            ptr(p["senet.excitation.0.bias"]), ptr(p["senet.excitation.2.weight"]), ptr(p["senet.excitation.2.bias"]), R]
    ldc = 15 * d

    def outputs(rows, c_bf16):
        return (torch.full((rows, 5, d), 7.0, device=dev), torch.full((rows, 5, d), 7.0, dtype=torch.bfloat16, device=dev),
                torch.full((rows, ldc), 7.0, dtype=torch.bfloat16 if c_bf16 else torch.float32, device=dev),
                torch.full((rows, 6), 7.0, device=dev))

    def catalogue_fields(c_bf16):
        Vc, Vc16, c, a = outputs(U * M, c_bf16)
        call("fbn_rec_fields", *head, ptr(Vc), ptr(Vc16), ptr(c), ldc, c_bf16, ptr(a), ptr(err), U, 0, M, d, st)
        return Vc, Vc16, c[:, :5 * d], a

    def list_fields(pos_d, ldp, c0, Cc, c_bf16, flag):
        Vc, Vc16, c, a = outputs(U * Cc, c_bf16)
        call("fbn_rec_fields_list", *head, ptr(Vc), ptr(Vc16), ptr(c), ldc, c_bf16, ptr(a), ptr(flag), U, ptr(pos_d),
             ldp, c0, Cc, M, d, st)
        assert (c[:, 5 * d:] == 7.0).all()                          # only the V block of c is written
        return Vc, Vc16, c[:, :5 * d], a

    pos = _field_lists()
    pos_d = torch.from_numpy(pos).to(dev)
    one = torch.full((U, 1), -1, dtype=torch.int64, device=dev)    # one empty slot per user: the empty row
    for c_bf16 in (0, 1):
        want = catalogue_fields(c_bf16)
        empty = list_fields(one, 1, 0, 1, c_bf16, err)
        for t in empty:
            assert torch.isfinite(t.float()).all()
        assert (empty[0][:, :4] == 0).all() and (empty[0][1:, 4] != 0).any()      # X1..X4 = 0, X5 = a5 * hist[u]
        assert torch.equal(empty[0][:, 4], hist * empty[3][:, 5:6])
        for c0, Cc in ((0, 100), (100, 50)):
            got = list_fields(pos_d, F_LDP, c0, Cc, c_bf16, err)
            m = pos_d[:, c0:c0 + Cc]
            live = (m >= 0).reshape(-1)
            assert int((~live).sum()) > 0 and int(live.sum()) > 2 * Cc
            src = (torch.arange(U, device=dev)[:, None] * M + m.clamp(min=0)).reshape(-1)
            user = torch.arange(U, device=dev).repeat_interleave(Cc)
            for g, w, e in zip(got, want, empty):
                assert torch.equal(g[live], w[src[live]]), (c_bf16, c0, Cc)
                assert torch.equal(g[~live], e[user[~live]]), (c_bf16, c0, Cc)
    assert int(err.item()) == 0                                      # an empty slot sets no flag

    # positions M and M + 5: treated as empty, flagged, and nothing faults
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    over = pos_d[:, :8].clone().contiguous()
    over[0, 3], over[2, 6] = M, M + 5
    got = list_fields(over, 8, 0, 8, 0, flag)
    empty = list_fields(one, 1, 0, 1, 0, err)
    torch.cuda.synchronize()
    assert int(flag.item()) & 1 and int(err.item()) == 0
    for g, e in zip(got, empty):
        assert torch.equal(g[3], e[0]) and torch.equal(g[2 * 8 + 6], e[2])


# ---------------------------------------------------------------------------------------- 2. / 3. the kernels on raw logits
K_U, K_C, K_LDP, K_LD = 5, 1100, 1103, 1103
K_CHUNKS = {"one": ((0, 1100),), "carry": ((0, 400), (400, 400), (800, 300))}
HIST_SLOT, PAD_SLOT, EMPTY_SLOT, REP_POS = 7, 9, 11, 321
FEW = {3: 100, 1023: 200, 1024: 300, 1099: 400}                    # list 4's only ordinary items


@functools.lru_cache(maxsize=None)
def _kernel_lists():
    """ids [M], seq [5, 20], pos [5, ldp], logits [5, C]: full; length 700; interior empty slots (and one
    position >= M); one position in three slots; four ordinary items beside a history and a padding item."""
    rng = np.random.default_rng(43)
    ids = _catalogue()["item_id"].numpy()
    hist = _histories().numpy()
    seq = hist[[0, 1, 2, 1, 2]].copy()
    pos = np.full((K_U, K_LDP), -9, dtype=np.int64)
    pos[:, :K_C] = rng.integers(0, M_CAT, size=(K_U, K_C))           # with replacement: repeats everywhere
    pos[2, :K_C][rng.random(K_C) < 0.3] = -1
    pos[2, [0, 1023, 1024, 1099]] = [11, 12, 13, 14]
    pos[2, 13], pos[2, 14] = M_CAT + 3, M_CAT                         # not in the catalogue: empty
    row = pos[3, :K_C]
    row[row == REP_POS] = REP_POS + 1
    row[[20, 600, 1050]] = REP_POS                                    # one position, three candidates
    pos[4, :K_C] = -1
    for s, m in FEW.items():
        pos[4, s] = m
    pos[:, HIST_SLOT], pos[:, PAD_SLOT] = HIST_POS, PAD_POS
    pos[1:, EMPTY_SLOT] = -1
    pos[1, 700:K_C] = -1
    logits = K_VALUES[rng.integers(0, len(K_VALUES), size=(K_U, K_C))]
    logits[3, [20, 600, 1050]] = np.inf                               # ... tied at the top
    return ids, seq, pos, logits


def _eligible(ids, seq_row, pos_row, exclude, target=None):
    """bool [C]: the documented eligibility of every slot of one list."""
    live = (pos_row >= 0) & (pos_row < M_CAT)
    if not exclude:
        return live
    item = ids[np.where(live, pos_row, 0)]
    in_hist = np.isin(item, [int(s) for s in seq_row if s != 0])
    if target is not None:
        in_hist &= np.arange(len(pos_row)) != target
    return live & (item != 0) & ~in_hist


def _ref_topk(logits, ids, seq, pos, exclude, K):
    """The five outputs [U, K] from the slot keys (numpy)."""
    U, C = logits.shape
    keys = _keys(logits)
    out = {"slot": np.full((U, K), -1, np.int64), "index": np.full((U, K), -1, np.int64),
           "item_id": np.full((U, K), -1, np.int64), "logit": np.full((U, K), -np.inf, np.float32),
           "prob": np.zeros((U, K), np.float32)}
    one = np.float32(1.0)
    for u in range(U):
        k = np.where(_eligible(ids, seq[u], pos[u, :C], exclude), keys[u], np.uint64(0))
        order = np.argsort(k, kind="stable")[::-1][:K]
        order = order[k[order] != 0]
        n = len(order)
        assert (np.uint64(0xFFFFFFFF) - (k[order] & np.uint64(0xFFFFFFFF)) == order.astype(np.uint64)).all()
        out["slot"][u, :n], out["index"][u, :n] = order, pos[u, order]
        out["item_id"][u, :n], out["logit"][u, :n] = ids[pos[u, order]], logits[u, order]
        with np.errstate(over="ignore", invalid="ignore"):
            out["prob"][u, :n] = one / (one + np.exp(-logits[u, order], dtype=np.float32))   # the header's sigmoid
    return {n: torch.from_numpy(v) for n, v in out.items()}


def _run_topk_list(dev, logits, ids, seq, pos, exclude, K, chunks):
    st = _lib.stream_handle(dev)
    U = logits.shape[0]
    ids_d, seq_d, pos_d = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ids, seq, pos))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    carry = torch.zeros((U, K), dtype=torch.int64, device=dev)
    out = {n: torch.full((U, K), 77, dtype=torch.int64, device=dev) for n in ("slot", "index", "item_id")}
    out.update({n: torch.full((U, K), 77.0, device=dev) for n in ("logit", "prob")})
    nws = int(_lib.lib().fbn_rec_topk_workspace_size(U, max(c for _, c in chunks), K))
    ws = torch.empty(max(1, nws // 8), dtype=torch.int64, device=dev)
    for i, (c0, Cc) in enumerate(chunks):
        lg = torch.from_numpy(np.ascontiguousarray(logits[:, c0:c0 + Cc])).to(dev)
        o = out if i == len(chunks) - 1 else {}
        call("fbn_rec_topk_list", ptr(lg), U, c0, Cc, ptr(pos_d), pos.shape[1], M_CAT, ptr(ids_d), ptr(seq_d),
             seq.shape[1], int(exclude), K, ptr(carry), ptr(ws), nws, ptr(o.get("slot")), ptr(o.get("index")),
             ptr(o.get("item_id")), ptr(o.get("logit")), ptr(o.get("prob")), ptr(status), st)
    return {n: t.cpu() for n, t in out.items()}, int(status.item())


def _check_topk(got, want, what):
    for n in ("slot", "index", "item_id", "logit", "prob"):
        if not _same(got[n], want[n]):
            bad = (got[n] != want[n]).nonzero()[:4].tolist()
            raise AssertionError((what, n, bad, [(got[n][r, c].item(), want[n][r, c].item()) for r, c in bad]))


@pytest.mark.parametrize("chunks", sorted(K_CHUNKS))
@pytest.mark.parametrize("exclude", [1, 0])
def test_topk_list_kernel_equals_the_slot_key_order(hip_device, exclude, chunks):
    ids, seq, pos, logits = _kernel_lists()
    for K in (1, 10, 256):
        want = _ref_topk(logits, ids, seq, pos, exclude, K)
        got, status = _run_topk_list(hip_device, logits, ids, seq, pos, exclude, K, K_CHUNKS[chunks])
        _check_topk(got, want, (exclude, chunks, K))
        assert status == 0
    # the inputs do what they are there for (K = 256)
    slots = want["slot"].tolist()
    n_live = (want["slot"] >= 0).sum(dim=1).tolist()
    assert n_live[0] == 256 and n_live[4] == (4 if exclude else 6)                 # the short list's -1 tail
    assert (want["slot"][1] < 700).all()
    assert 13 not in slots[2] and 14 not in slots[2] and EMPTY_SLOT not in slots[2]  # positions >= M; an empty slot
    if exclude:
        assert all(PAD_SLOT not in row for row in slots) and all(HIST_SLOT not in row for row in slots[1:])
    rep = [s for s in slots[3] if s in (20, 600, 1050)]
    assert rep == [20, 600, 1050]                                                    # one position, three candidates,
    assert want["index"][3][[slots[3].index(s) for s in rep]].tolist() == [REP_POS] * 3      # tied: in slot order


def test_topk_list_kernel_nan(hip_device):
    ids, seq, pos, logits = _kernel_lists()
    for chunks in K_CHUNKS.values():
        dead = logits.copy()
        dead[1, 800], dead[2, 13], dead[4, 500] = np.nan, np.nan, np.nan          # empty slots, one a position >= M
        got, status = _run_topk_list(hip_device, dead, ids, seq, pos, 1, 10, chunks)
        _check_topk(got, _ref_topk(logits, ids, seq, pos, 1, 10), "nan in empty slots")
        assert status == 0
        live = logits.copy()
        live[4, 1023], live[4, 3], live[4, 1024], live[4, 1099] = np.nan, -np.inf, 0.0, 1.5
        got, status = _run_topk_list(hip_device, live, ids, seq, pos, 1, 10, chunks)
        _check_topk(got, _ref_topk(live, ids, seq, pos, 1, 10), "nan in a live slot")
        assert status == 1
        assert got["slot"][4, :6].tolist() == [1099, 1024, 3, 1023, -1, -1]       # ..., -inf, then the NaN, then the tail
        assert torch.isnan(got["logit"][4, 3]) and torch.isneginf(got["logit"][4, 2])


def _rank_targets():
    """slot per (target kind, list): [9, 5]."""
    empty = [-5] + [EMPTY_SLOT] * 4                                  # list 0 is full: its "empty" target is outside
    kinds = [[0] * 5, [1023] * 5, [1024] * 5, [1099] * 5, [HIST_SLOT] * 5, [PAD_SLOT] * 5, empty, [-1] * 5, [K_C] * 5]
    return np.array(kinds, dtype=np.int64)


def _ref_rank_list(logits, ids, seq, pos, tslot, exclude):
    U, C = logits.shape
    keys, at = _keys(logits), np.arange(C)
    rank, nel = np.zeros(U, np.int32), np.zeros(U, np.int32)
    for u in range(U):
        t = int(tslot[u])
        elig = _eligible(ids, seq[u], pos[u, :C], exclude, target=t)
        nel[u] = elig.sum()
        if 0 <= t < C and 0 <= pos[u, t] < M_CAT and ids[pos[u, t]] != 0:
            rank[u] = 1 + int((elig & (at != t) & (keys[u] > keys[u, t])).sum())
    return rank, nel


def _run_rank_list(dev, logits_ld, ids, seq, pos, tslot, exclude, C):
    st = _lib.stream_handle(dev)
    U = logits_ld.shape[0]
    lg, ids_d, seq_d, pos_d, ts = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                                   for a in (logits_ld, ids, seq, pos, tslot))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rank = torch.full((U,), 77, dtype=torch.int32, device=dev)       # the call initialises its outputs
    nel = torch.full((U,), 77, dtype=torch.int32, device=dev)
    call("fbn_rec_rank_list", ptr(lg), logits_ld.shape[1], U, C, ptr(pos_d), pos.shape[1], M_CAT, ptr(ids_d),
         ptr(seq_d), seq.shape[1], int(exclude), ptr(ts), ptr(rank), ptr(nel), ptr(status), st)
    return rank.cpu(), nel.cpu(), int(status.item())


@functools.lru_cache(maxsize=None)
def _rank_inputs():
    """The five lists under each of the nine target kinds: 45 rows."""
    ids, seq, pos, logits = _kernel_lists()
    tslot = _rank_targets().reshape(-1)
    n = len(tslot) // K_U
    wide = np.full((K_U, K_LD), np.inf, dtype=np.float32)            # the 3 columns past C are never candidates
    wide[:, :K_C] = logits
    return ids, np.tile(seq, (n, 1)), np.tile(pos, (n, 1)), np.tile(wide, (n, 1)), tslot


@pytest.mark.parametrize("exclude", [1, 0])
def test_rank_list_kernel_equals_the_slot_key_count(hip_device, exclude):
    ids, seq, pos, wide, tslot = _rank_inputs()
    want_rank, want_nel = _ref_rank_list(wide[:, :K_C], ids, seq, pos, tslot, exclude)
    rank, nel, status = _run_rank_list(hip_device, wide, ids, seq, pos, tslot, exclude, K_C)
    assert torch.equal(rank, torch.from_numpy(want_rank)), (rank.tolist(), want_rank.tolist())
    assert torch.equal(nel, torch.from_numpy(want_nel)), (nel.tolist(), want_nel.tolist())
    assert status == 0
    kind = want_rank.reshape(-1, K_U)                                 # [target kind, list]
    assert (kind[5:] == 0).all()                                      # padding item, empty slot, -1 and C: not ranked
    assert (kind[1:4, 1] == 0).all()                                  # list 1 ends at slot 700
    assert (kind[0, :4] >= 1).all() and kind[0, 4] == 0               # slot 0 (empty in list 4)
    assert (kind[4] >= 1).all()                                       # a history target is ranked, under both flags
    assert len(set(want_rank[want_rank > 0].tolist())) > 5            # ties everywhere, yet no flat answer
    nel = want_nel.reshape(-1, K_U)
    if exclude:
        assert nel[0, 4] == 4 and nel[4, 4] == 5                      # the target's own slot stays eligible
        assert (nel[4, 1:] == nel[7, 1:] + 1).all()
    else:
        assert nel[0].tolist()[:2] == [K_C, 699] and nel[0, 4] == 6 and (nel == nel[0]).all()


def test_rank_list_kernel_nan_only_at_a_ranked_target(hip_device):
    ids, seq, pos, wide, tslot = _rank_inputs()
    far = wide.copy()
    far[0, 300], far[1, 800], far[K_U + 4, 500] = np.nan, np.nan, np.nan      # a live non-target slot; empty slots
    rank, nel, status = _run_rank_list(hip_device, far, ids, seq, pos, tslot, 1, K_C)
    want_rank, want_nel = _ref_rank_list(far[:, :K_C], ids, seq, pos, tslot, 1)
    assert torch.equal(rank, torch.from_numpy(want_rank)) and torch.equal(nel, torch.from_numpy(want_nel))
    assert status == 0
    own = far.copy()
    own[K_U + 4, 1023] = np.nan                                       # list 4's target slot 1023
    rank, nel, status = _run_rank_list(hip_device, own, ids, seq, pos, tslot, 1, K_C)
    want_rank, want_nel = _ref_rank_list(own[:, :K_C], ids, seq, pos, tslot, 1)
    assert torch.equal(rank, torch.from_numpy(want_rank)) and torch.equal(nel, torch.from_numpy(want_nel))
    assert status == 1 and want_rank[K_U + 4] == want_nel[K_U + 4] == 4      # the NaN target is last among the eligible


# ---------------------------------------------------------------------------------------- 4. the whole catalogue as a list
MODES = [(16, "fp32"), (128, "fp32"), (128, "bf16")]


@pytest.mark.parametrize("chunk_rows", [CAT_CHUNKED, CAT_SINGLE])
@pytest.mark.parametrize("d,mode", MODES)
def test_a_list_of_the_whole_catalogue_is_the_catalogue_path(hip_device, d, mode, chunk_rows):
    dev = hip_device
    rec = _rec(d, dev, chunk_rows, mode=mode)
    seq = _histories().to(dev)
    whole = torch.arange(M_CAT, device=dev).repeat(U_HIST, 1)
    ids = _catalogue()["item_id"]
    assert torch.equal(rec.score_lists(seq, whole, by="index", logits=True), rec.score(seq, logits=True))
    assert torch.equal(rec.score_lists(seq, whole, by="index"), rec.score(seq))
    tgt = torch.tensor([int(ids[399]), int(ids[45]), 0])             # ordinary; in user 1's history; the padding item
    tpos = rec.positions(tgt)
    assert tpos.tolist() == [399, 45, PAD_POS]
    for exclude in (True, False):
        for k in (1, 10, 256):
            a, b = rec.topk_lists(seq, whole, k, exclude_history=exclude, by="index"), rec.topk(seq, k, exclude)
            for n in ("index", "item_id", "logit", "prob"):
                assert torch.equal(a[n], b[n]), (exclude, k, n)
            assert torch.equal(a["slot"], a["index"])
        a = rec.rank_lists(seq, whole, tpos, exclude_history=exclude, by="index")
        b = rec.rank(seq, tgt, exclude_history=exclude)
        assert torch.equal(a["rank"], b["rank"]) and torch.equal(a["n_eligible"], b["n_eligible"])
        assert a["rank"].dtype == torch.int32 and a["rank"][2].item() == 0 and (a["rank"][:2] >= 1).all()
    assert int(rec.status.item()) == 0
    rec.check_ids()


# ---------------------------------------------------------------------------------------- 5. real shortlists
S_C = 300
S_CHUNKED = U_HIST * 128         # chunks of 128, 128 and 44 slots
S_SINGLE = U_HIST * S_C

# bf16 / bf16_fwd: max |dlogit| of the project's eval forward (ops.forward) against itself on the 900
# expanded rows of the lists, run as one batch and as two halves, measured on an MI355X
# (_list_forward_spread below; profiles/recommend_lists_parity.json), and the bound 4 x that spread with
# the fp32 bound as the floor.
#   (mode, d): (measured spread, bound)
BF16_SPREAD_BOUND = {
    ("bf16", 16): (0.0, 1e-4),
    ("bf16", 128): (0.0, 1e-4),
    ("bf16_fwd", 16): (0.0, 1e-4),
    ("bf16_fwd", 128): (0.0, 1e-4),
}


@functools.lru_cache(maxsize=None)
def _short_lists():
    """pos [3, 300] (int64): interior empty slots; 220 slots then empty; 30 % empty.  Every list holds
    the padding item and a position whose id is in the user's history (users 1 and 2)."""
    rng = np.random.default_rng(47)
    pos = rng.integers(0, M_CAT, size=(U_HIST, S_C)).astype(np.int64)
    pos[0, [3, 127, 128, 299]] = -1
    pos[1, 220:] = -1
    pos[2][rng.random(S_C) < 0.3] = -1
    pos[:, 10], pos[:, 200] = PAD_POS, (45, 45, 500)
    pos[:, 0], pos[:, 130] = (7, 8, 9), (1036, 0, 1035)
    return torch.from_numpy(pos)


def _expanded_lists(dev):
    """The ordinary batch of the U x C pairs of _short_lists(), row u * C + j (an empty slot: position 0)."""
    cat, pos = _catalogue(), _short_lists()
    m = pos.clamp(min=0).reshape(-1)
    b = {k: v[m] for k, v in cat.items()}
    b["item_seq"] = _histories().repeat_interleave(S_C, dim=0)
    return _to(b, dev)


def _list_forward_spread(d, mode, dev):
    """max |dlogit| of ops.forward on the expanded rows of the lists: one batch vs two halves."""
    b = _expanded_lists(dev)
    whole = _project_forward(d, mode, b, dev)
    h = whole.numel() // 2
    lo = _project_forward(d, mode, {k: v[:h].contiguous() for k, v in b.items()}, dev)
    hi = _project_forward(d, mode, {k: v[h:].contiguous() for k, v in b.items()}, dev)
    return (torch.cat([lo, hi]) - whole).abs().max().item(), whole


def _as_ids(pos):
    """The lists as item ids: an empty slot stays -1 (no catalogue id is negative)."""
    ids = _catalogue()["item_id"]
    return torch.where(pos >= 0, ids[pos.clamp(min=0)], torch.full_like(pos, -1))


@pytest.mark.parametrize("chunk_rows", [S_CHUNKED, S_SINGLE])
@pytest.mark.parametrize("d", [16, 128])
def test_list_scores_match_the_oracle_fp32(hip_device, d, chunk_rows):
    dev = hip_device
    rec = _rec(d, dev, chunk_rows)
    seq, pos = _histories().to(dev), _short_lists()
    live = pos >= 0
    want = _oracle_logits(d).view(U_HIST, M_CAT).gather(1, pos.clamp(min=0))
    logits = rec.score_lists(seq, pos.to(dev), by="index", logits=True).cpu()
    probs = rec.score_lists(seq, pos.to(dev), by="index").cpu()
    dl = (logits - want)[live].abs().max().item()
    dp = (probs - torch.sigmoid(want))[live].abs().max().item()
    print(f"fp32 d={d} chunk_rows={chunk_rows}: lists max |dlogit| {dl:.3e}, max |dprob| {dp:.3e}")
    assert logits.shape == (U_HIST, S_C) and int((~live).sum()) > 100
    assert dl < FP32_BOUND and dp < FP32_BOUND
    assert torch.isneginf(logits[~live]).all() and (probs[~live] == 0).all()       # empty slots
    by_id = rec.score_lists(seq, _as_ids(pos).to(dev), logits=True).cpu()           # by="item_id": the same lists
    assert torch.equal(by_id, logits)
    cold = rec.score_lists(None, pos[:1].to(dev), by="index", logits=True).cpu()
    want0 = _oracle_logits(d, with_seq=False).view(1, M_CAT).gather(1, pos[:1].clamp(min=0))
    assert cold.shape == (1, S_C) and (cold - want0)[live[:1]].abs().max().item() < FP32_BOUND
    rec.check_ids()


@pytest.mark.parametrize("chunk_rows", [S_CHUNKED, S_SINGLE])
@pytest.mark.parametrize("mode,d", sorted(BF16_SPREAD_BOUND))
def test_list_scores_match_the_projects_forward_bf16(hip_device, mode, d, chunk_rows):
    dev = hip_device
    spread, whole = _list_forward_spread(d, mode, dev)
    _, bound = BF16_SPREAD_BOUND[(mode, d)]
    rec = _rec(d, dev, chunk_rows, mode=mode)
    pos = _short_lists().to(dev)
    live = pos >= 0
    logits = rec.score_lists(_histories().to(dev), pos, by="index", logits=True)
    dl = (logits - whole.view(U_HIST, S_C))[live].abs().max().item()
    print(f"{mode} d={d} chunk_rows={chunk_rows}: forward one batch vs halves {spread:.3e}; "
          f"lists vs forward {dl:.3e}; bound {bound:.3e}")
    assert dl < bound
    assert torch.isneginf(logits[~live]).all()
    rec.check_ids()


@pytest.mark.parametrize("chunk_rows", [S_CHUNKED, S_SINGLE])
@pytest.mark.parametrize("d,mode", MODES)
def test_topk_and_rank_lists_are_exact_on_their_own_scores(hip_device, d, mode, chunk_rows):
    dev = hip_device
    rec = _rec(d, dev, chunk_rows, mode=mode)
    seq, pos = _histories(), _short_lists()
    ids = _catalogue()["item_id"]
    scores = rec.score_lists(seq.to(dev), pos.to(dev), by="index", logits=True).cpu()
    live = pos >= 0
    assert all(scores[u][live[u]].unique().numel() > 100 for u in range(U_HIST))       # a ranking, not one flat score
    raw = torch.where(live, scores, torch.zeros_like(scores)).numpy()                  # an empty slot's logit is not read
    tslot = torch.tensor([[0, 127, 128, 299, 200, 10, -1, S_C], [0, 219, 220, 130, 200, 10, 299, 5],
                          [0, 130, 200, 10, 1, 2, 3, 4]])                              # [3 users, 8 targets]
    for exclude in (True, False):
        for k in (1, 10, 256):
            got = {n: t.cpu() for n, t in rec.topk_lists(seq.to(dev), pos.to(dev), k, exclude_history=exclude,
                                                         by="index").items()}
            want = _ref_topk(raw, ids.numpy(), seq.numpy(), pos.numpy(), exclude, k)
            for n in ("slot", "index", "item_id", "logit"):
                assert _same(got[n], want[n]), (exclude, k, n)
            assert (got["prob"] - torch.sigmoid(got["logit"])).abs().max().item() < 1e-6
            if exclude:
                for u in range(U_HIST):
                    hist = set(int(s) for s in seq[u].tolist() if s != 0)
                    assert not (set(got["item_id"][u].tolist()) & hist) and 0 not in got["item_id"][u].tolist()
        for t in range(tslot.shape[1]):
            out = rec.rank_lists(seq.to(dev), pos.to(dev), tslot[:, t], exclude_history=exclude, by="index")
            want_rank, want_nel = _ref_rank_list(raw, ids.numpy(), seq.numpy(), pos.numpy(), tslot[:, t].numpy(), exclude)
            assert out["rank"].cpu().tolist() == want_rank.tolist(), (exclude, t)
            assert out["n_eligible"].cpu().tolist() == want_nel.tolist(), (exclude, t)
    assert (got["slot"][1] < 220).all() and (got["slot"] >= 0).sum().item() > 256      # user 1's short list ends early
    assert int(rec.status.item()) == 0
    rec.check_ids()


def test_list_ids_outside_the_catalogue_and_the_tables(hip_device):
    dev = hip_device
    rec = _rec(16, dev, S_CHUNKED)
    seq, pos = _histories().to(dev), _short_lists()
    cand = _as_ids(pos)
    assert 4999 not in _catalogue()["item_id"].tolist()
    cand[0, 5], cand[1, 6], cand[2, 8] = 4999, V_SMALL + 10, -3       # not in the catalogue; outside the table; negative
    base = rec.score_lists(seq, _as_ids(pos).to(dev), logits=True).cpu()
    got = rec.score_lists(seq, cand.to(dev), logits=True).cpu()
    changed = torch.zeros_like(pos, dtype=torch.bool)
    changed[0, 5] = changed[1, 6] = changed[2, 8] = True
    assert torch.isneginf(got[changed]).all() and torch.equal(got[~changed], base[~changed])
    top = rec.topk_lists(seq, cand.to(dev), 256)
    for u, s in ((0, 5), (1, 6), (2, 8)):
        assert s not in top["slot"][u].tolist()
    out = rec.rank_lists(seq, cand.to(dev), torch.tensor([5, 6, 8]))
    assert out["rank"].tolist() == [0, 0, 0]
    rec.check_ids()                                                   # an unknown candidate id is no table access
    over = pos.clone()
    over[1, 4] = M_CAT                                                # by="index": a position past the catalogue
    assert torch.isneginf(rec.score_lists(seq, over.to(dev), by="index", logits=True)[1, 4])
    with pytest.raises(IndexError):
        rec.check_ids()
    rec = _rec(16, dev, S_CHUNKED)
    bad = seq.clone()
    bad[1, 4] = V_SMALL                                               # a history id outside the table
    rec.topk_lists(bad, cand.to(dev), 10)
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        rec.check_ids()
    for call_ in (lambda: rec.topk_lists(seq, cand.to(dev), 0), lambda: rec.topk_lists(seq, cand.to(dev), 257),
                  lambda: rec.score_lists(seq, cand[:2].to(dev)), lambda: rec.score_lists(seq, cand.to(dev), by="name"),
                  lambda: rec.rank_lists(seq, cand.to(dev), torch.tensor([1, 2]))):
        with pytest.raises(ValueError):
            call_()


# ---------------------------------------------------------------------------------------- 6. sampled evaluation
def _pairs(dev):
    """Two batches with mixed labels whose positive rows are the 27 users of test_gpu_rank_eval._rows(), in
    order (14 + 13), as test_evaluate_equals_rank_update_compute builds them."""
    seq, tgt = _rows()
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
    return pairs


def _sampled_by_hand(rec, blocks, n_neg, ks, seed, exclude=True):
    """evaluate_sampled's protocol rebuilt from rank_lists: one draw of [users, n_neg] per block."""
    dev = rec.device
    seq, tgt = _rows()
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    m, n_cand = RankMetrics(dev), 0
    for r0, n in blocks:
        tpos = rec.positions(tgt[r0:r0 + n].to(dev))
        neg = torch.randint(0, M_CAT, (n, n_neg), generator=gen, device=dev, dtype=torch.int64)
        neg = torch.where(neg == tpos[:, None], torch.full_like(neg, -1), neg)
        out = rec.rank_lists(seq[r0:r0 + n].to(dev), torch.cat([tpos[:, None], neg], dim=1),
                             torch.zeros(n, dtype=torch.int64), exclude_history=exclude, by="index")
        m.update(out["rank"])
        n_cand += int(out["n_eligible"][out["rank"] > 0].sum().item())
    res = m.compute(ks)
    res["mean_candidates"] = n_cand / res["n"] if res["n"] else 0.0
    return res


def test_evaluate_sampled_equals_rank_lists_update_compute(hip_device):
    dev = hip_device
    rec = _rec(16, dev, CAT_CHUNKED)
    pairs = _pairs(dev)
    ks = (1, 10)
    want = _sampled_by_hand(rec, ((0, 14), (14, 13)), 50, ks, 3)
    got = rec.evaluate_sampled(pairs, n_neg=50, ks=ks, seed=3)
    assert got == want
    assert got["n"] == 23 and got["n_skipped"] == 4                   # evaluate's: 3 padding targets + the all-padding user's own
    full = rec.evaluate(pairs, ks)
    assert (got["n"], got["n_skipped"]) == (full["n"], full["n_skipped"])
    assert 1.0 < got["mean_candidates"] <= 51.0
    assert rec.evaluate_sampled(iter(pairs), n_neg=50, ks=ks, seed=3) == got          # the same seed: the same dict
    other = rec.evaluate_sampled(pairs, n_neg=50, ks=ks, seed=4)
    assert other["n"] == 23 and sorted(other) == sorted(got)
    # the blocking and max_users are honoured: the draws follow the blocks
    blocks5 = ((0, 5), (5, 5), (10, 4), (14, 5), (19, 5), (24, 3))
    assert rec.evaluate_sampled(pairs, n_neg=50, ks=ks, seed=3, users_per_block=5) == \
        _sampled_by_hand(rec, blocks5, 50, ks, 3)
    seven = rec.evaluate_sampled(pairs, n_neg=50, ks=ks, seed=3, max_users=7)
    assert seven == _sampled_by_hand(rec, ((0, 7),), 50, ks, 3) and seven["n"] + seven["n_skipped"] == 7
    off = rec.evaluate_sampled(pairs, n_neg=50, ks=ks, seed=3, exclude_history=False)
    assert off == _sampled_by_hand(rec, ((0, 14), (14, 13)), 50, ks, 3, exclude=False)
    assert off["mean_candidates"] >= got["mean_candidates"]
    # no negatives: every ranked user is first in a list of one
    alone = rec.evaluate_sampled(pairs, n_neg=0, ks=ks)
    assert alone["n"] == 23 and alone["hr"][1] == 1.0 and alone["mean_rank"] == 1.0 and alone["mean_candidates"] == 1.0
    assert sorted(rec.evaluate_sampled(pairs, seed=1)["hr"]) == [5, 10, 20]            # the defaults: 99 negatives
    with pytest.raises(ValueError):
        rec.evaluate_sampled(pairs, n_neg=-1)
    assert int(rec.status.item()) == 0
    rec.check_ids()
