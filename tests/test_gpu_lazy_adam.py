"""The lazy table Adam entry points, one at a time, against the library's own eager kernels (pytest -m gpu).

The eager twin.  A table [NROWS][D] with m, v and the 16-byte row-state record per row is stepped
eagerly for s = 0 .. T: fbn_adam_table(mode = 1) gives every row the zero-gradient step, except the rows
that carry a deferred gradient at step s, which take fbn_adam_touched in the owner layout (Lp1 = 1:
gvec [NE][D] = ring slot s % ring_n, slot_row[e] = row, map[row] = e) with that step's clip coefficient
coef_hist[s].  Those two kernels are the definition of "eager"; tests/test_gpu_adam.py pins them (and the flush
of a deferred gradient) to float64 torch Adam, launch by launch, so bit-identity with them carries that anchor.

The lazy copy.  Row r has a replay start k0[r] drawn from [max(0, T - lag_max), T]; it takes the twin's
(p, m, v) of that row as they stood before step k0[r] (copied across as the twin's loop passes
s == k0[r]), last[r] = k0[r], and about a third of the lagging rows carry pend[r] = e, their gradient in
ring[k0 % ring_n][e] and a non-unit coef_hist[k0].

After an entry point has run, (p, m, v) of every row it must have brought up to date are BITWISE equal to
the twin's at the target step, with last == target and pend == -1; every other row is bitwise unchanged,
last and pend included.  The lazy copy holds live rows everywhere (nothing is pre-filled with zeros), so
a missed or a stray store shows.
"""
import functools

import numpy as np
import pytest
import torch

from ctr_recommendation_amd import _lib, schedule
from ctr_recommendation_amd._lib import call, ptr

pytestmark = pytest.mark.gpu

NROWS = 1500          # no multiple of 64, of the rows per wave (8 / 16), or of F
NE = 64               # deferred-gradient slots per ring step
FBN_SLOT_FLAG = 0x40000000
FBN_RING_BF16 = 0x40000000
FBN_GRAD_BF16 = 0x40000
FBN_ERR_ARG, FBN_ERR_UNSUPPORTED = 1, 3
BETA2, EPS, WD = 0.999, 1e-8, 1e-2
F_WIN = 7             # the rolling window's F

D_ALL = [16, 32, 64, 128, 256]
D_WIDE = [128, 256]
# (D, decoupled, kind): kind "small" = T 40, lag <= 33, ring of 34 steps; "large" = T 300 = total_steps,
# lag <= 299, no deferred gradients (past the 256-step LDS window, the table's last row read);
# "bf16" = small with a bf16 ring
SMALL = [(D, dw, "small") for D in D_ALL for dw in (0, 1)]
LARGE = [(16, 0, "large"), (128, 0, "large")]
BF16 = [(128, 0, "bf16")]


def _id(c):
    return f"D{c[0]}-dw{c[1]}-{c[2]}"


def _cases(ds, large=True):
    out = [c for c in SMALL if c[0] in ds] + ([c for c in LARGE if c[0] in ds] if large else []) + BF16
    return pytest.mark.parametrize("cfg", out, ids=_id)


class Case:
    """The twin's snapshots and the lazy copy of one (D, decoupled, kind); built once, never modified."""

    def __init__(self, dev, D, decoupled, kind):
        self.dev, self.D, self.decoupled, self.kind = dev, D, decoupled, kind
        large = kind == "large"
        self.T = T = 300 if large else 40
        self.total = 300 if large else 48
        self.lag_max = 299 if large else 33
        self.ring_n = 34
        self.pend_on = not large
        self.bf16 = kind == "bf16"
        # the prefetch's target: T + 1 (rows replayed through step T inclusive); the large case stops at
        # T, the last row of its schedule table
        self.pf_target = T if large else T + 1
        last_step = T if large else T + 1                         # eager steps run: s = 0 .. last_step - 1
        rng = np.random.RandomState(1000 + D + 7 * decoupled + (31 if large else 0))
        self.wd = 0.0 if decoupled else WD                        # as the trainer: L2 inside the gradient, or dmul
        tab, _ = schedule.adam_table(self.total, decoupled_wd=WD if decoupled else 0.0)
        assert tab.shape == (self.total + 1, 8)
        self.sched = torch.from_numpy(tab).to(dev)
        k0 = rng.randint(max(0, T - self.lag_max), T + 1, size=NROWS)
        k0[rng.choice(NROWS, 40, replace=False)] = T              # some rows surely up to date
        self.k0 = k0
        pend = np.full(NROWS, -1, dtype=np.int64)
        coef = np.ones(last_step + 1, dtype=np.float32)
        if self.pend_on:
            coef[:] = rng.uniform(0.3, 0.95, size=coef.shape)
            for s in range(max(0, T - self.lag_max), T):
                rows = np.nonzero(k0 == s)[0]
                take = rows[rng.rand(rows.size) < 1.0 / 3.0][:NE]
                pend[take] = rng.permutation(NE)[:take.size]
        self.pend = pend
        g = torch.Generator(device="cpu").manual_seed(int(rng.randint(1 << 30)))
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
        tp = (0.1 * rnd(NROWS, D)).to(dev)
        tm = (0.01 * rnd(NROWS, D)).to(dev)
        tv = (1e-4 * rnd(NROWS, D).abs()).to(dev)
        self.coef_hist = torch.from_numpy(coef).to(dev)
        self.ring = None
        if self.pend_on:
            n = self.ring_n * NE * D
            vals = 0.1 * rnd(n)
            if self.bf16:     # 16 elements of padding: a bf16 row is read with the width of an f32 one
                self.ring_store = torch.zeros(n + 16, dtype=torch.bfloat16, device=dev)
                self.ring_store[:n] = vals.to(dev)
                self.ring = self.ring_store[:n]
            else:
                self.ring = vals.to(dev)
        # ---- the eager twin, and the lazy copy picked up on the way
        lp, lm, lv = torch.empty_like(tp), torch.empty_like(tm), torch.empty_like(tv)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        emap = torch.full((NROWS,), -1, dtype=torch.int32, device=dev)
        st = _lib.stream_handle(dev)
        k0_d = torch.from_numpy(k0).to(dev)
        esz = 2 if self.bf16 else 4
        lp1 = 1 | (FBN_GRAD_BF16 if self.bf16 else 0)
        self.snap = {}
        keep = set(range(T - F_WIN + 1, last_step + 1))
        for s in range(last_step + 1):
            idx = torch.nonzero(k0_d == s).flatten()
            if idx.numel():
                lp[idx], lm[idx], lv[idx] = tp[idx], tm[idx], tv[idx]
            if s in keep:
                self.snap[s] = (tp.clone(), tm.clone(), tv.clone())
            if s == last_step:
                break
            step.fill_(s)
            rows = np.nonzero((k0 == s) & (pend >= 0))[0]
            if rows.size:
                srow = torch.full((NE,), -1, dtype=torch.int32)
                srow[torch.from_numpy(pend[rows])] = torch.from_numpy(rows).int()
                srow = srow.to(dev)
                emap[torch.from_numpy(rows).to(dev)] = torch.from_numpy(pend[rows]).int().to(dev)
            call("fbn_adam_table", ptr(tp), ptr(tm), ptr(tv), NROWS, D, ptr(emap), None, None, None, 1, None,
                 ptr(self.sched), ptr(step), self.wd, BETA2, EPS, 1, st)
            if rows.size:
                gvec = self.ring.data_ptr() + (s % self.ring_n) * NE * D * esz
                call("fbn_adam_touched", ptr(tp), ptr(tm), ptr(tv), D, ptr(emap), gvec, None, ptr(srow), lp1, NE,
                     self.coef_hist.data_ptr() + 4 * s, ptr(self.sched), ptr(step), self.wd, BETA2, EPS, None, st)
                torch.cuda.synchronize(dev)
                assert bool((emap == -1).all())
        rs = torch.empty((NROWS, 4), dtype=torch.int32)
        rs[:, 0], rs[:, 1] = 123, 1                                # a stale pre-claim tag (step 1)
        rs[:, 2] = torch.from_numpy(k0).int()
        rs[:, 3] = torch.from_numpy(pend).int()
        self.base = (lp, lm, lv, rs.to(dev))
        torch.cuda.synchronize(dev)

    def state(self):
        """A fresh lazy copy: (p, m, v, row_state)."""
        return tuple(t.clone() for t in self.base)

    def tail(self, st, step):
        """The replay argument tail: last, table, step, wd, beta2, eps, pend, ring, coef_hist, stride, ring_n,
        decoupled."""
        rs = st[3]
        self._step = torch.full((1,), step, dtype=torch.int32, device=self.dev)
        pend = (rs.data_ptr() + 12, ptr(self.ring), ptr(self.coef_hist), NE * self.D,
                self.ring_n | (FBN_RING_BF16 if self.bf16 else 0)) if self.pend_on else (None, None, None, 0, 0)
        return (rs.data_ptr() + 8, ptr(self.sched), ptr(self._step), self.wd, BETA2, EPS, *pend, self.decoupled)

    def check(self, st, target_of_row):
        """target_of_row [NROWS] (CPU int64): the step a row must have been brought to, or -1 = untouched.
        Rows already at or past their target stay as they are."""
        p, m, v, rs = st
        torch.cuda.synchronize(self.dev)
        tgt = np.where(target_of_row > self.k0, target_of_row, -1)
        exp = [t.clone() for t in self.base]
        for t in np.unique(tgt[tgt >= 0]):
            idx = torch.from_numpy(np.nonzero(tgt == t)[0]).to(self.dev)
            for e, s in zip(exp[:3], self.snap[int(t)]):
                e[idx] = s[idx]
            exp[3][idx, 2] = int(t)
            exp[3][idx, 3] = -1
        for name, got, want in (("p", p, exp[0]), ("m", m, exp[1]), ("v", v, exp[2])):
            bad = (got.view(torch.int32) != want.view(torch.int32)).any(1).cpu().numpy()
            if bad.any():
                r = int(np.nonzero(bad)[0][0])
                raise AssertionError(f"{name}: {int(bad.sum())} rows differ bitwise; first row {r} (k0 {self.k0[r]}, "
                                     f"pend {self.pend[r]}, target {tgt[r]}): {got[r, :4].tolist()} vs "
                                     f"{want[r, :4].tolist()}")
        for name, col in (("last", 2), ("pend", 3)):
            bad = (rs[:, col] != exp[3][:, col]).cpu().numpy()
            if bad.any():
                r = int(np.nonzero(bad)[0][0])
                raise AssertionError(f"{name}: {int(bad.sum())} rows differ; first row {r} (k0 {self.k0[r]}, pend "
                                     f"{self.pend[r]}, target {tgt[r]}): {int(rs[r, col])} vs {int(exp[3][r, col])}")
        return exp


@functools.lru_cache(maxsize=None)
def _case(dev, D, decoupled, kind):
    return Case(dev, D, decoupled, kind)


def _targets(rows, target):
    t = np.full(NROWS, -1, dtype=np.int64)
    t[np.asarray(rows, dtype=np.int64)] = target
    return t


def _i32(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)


def _batch(seed, dev, B=33, L=20):
    """item [B], seq [B][L] (int64) from a pool of 300 ids, with id 0 padding; the entries' ids in order."""
    rng = np.random.RandomState(seed)
    pool = rng.choice(np.arange(1, NROWS), 300, replace=False)
    ent = pool[rng.randint(0, 300, size=(B, L + 1))]
    ent[rng.rand(B, L + 1) < 0.08] = 0
    ent[0, 3] = 0
    item = torch.from_numpy(ent[:, 0].copy()).to(dev)
    seq = torch.from_numpy(ent[:, 1:].copy()).to(dev)
    return item, seq, ent.reshape(-1), pool


def _lids(seed, n=700):
    """Local rows with negatives, duplicates and row 0."""
    rng = np.random.RandomState(seed)
    lids = rng.randint(0, NROWS, size=n)
    lids[rng.rand(n) < 0.1] = -1
    lids[5], lids[77] = 0, 0
    return lids


# ------------------------------------------------------------------------------------------ fbn_adam_flush
@_cases(D_ALL)
def test_flush(hip_device, cfg):
    c = _case(hip_device, *cfg)
    st = c.state()
    call("fbn_adam_flush", ptr(st[0]), ptr(st[1]), ptr(st[2]), NROWS, c.D, *c.tail(st, c.T),
         _lib.stream_handle(hip_device))
    c.check(st, _targets(np.arange(NROWS), c.T))


# ------------------------------------------------------------------- fbn_adam_catchup, the rolling window
def _window(c, st, t, cmap, dev):
    call("fbn_adam_catchup", ptr(st[0]), ptr(st[1]), ptr(st[2]), NROWS, c.D, None, 0, ptr(cmap), F_WIN, 2,
         *c.tail(st, t), _lib.stream_handle(dev))


@_cases(D_ALL)
def test_catchup_window(hip_device, cfg):
    c = _case(hip_device, *cfg)
    chunk = (NROWS + F_WIN - 1) // F_WIN
    win = lambda t: np.arange((t % F_WIN) * chunk, min(NROWS, (t % F_WIN + 1) * chunk))
    # the window of step T; every third row of it is claimed by the batch and left alone
    rows = win(c.T)
    cmap = np.full(NROWS, -1)
    cmap[rows[::3]] = 5
    st = c.state()
    _window(c, st, c.T, _i32(cmap, hip_device), hip_device)
    c.check(st, _targets(rows[cmap[rows] == -1], c.T))
    # every window in turn on one table: steps T - F + 1 .. T visit each of the rows once
    st = c.state()
    none = _i32(np.full(NROWS, -1), hip_device)
    tgt = np.full(NROWS, -1, dtype=np.int64)
    for t in range(c.T - F_WIN + 1, c.T + 1):
        _window(c, st, t, none, hip_device)
        tgt[win(t)] = t
    assert (tgt >= 0).all()
    c.check(st, tgt)


# --------------------------------------------------------------------- fbn_adam_catchup, the claimed rows
@_cases(D_ALL)
def test_catchup_claimed(hip_device, cfg):
    c = _case(hip_device, *cfg)
    rng = np.random.RandomState(5)
    rows = rng.choice(NROWS, 700, replace=False)                  # each row named at most once
    rows[:40] = np.nonzero(c.k0 == c.T)[0][:40]                   # ... some of them already at T
    rows = np.unique(rows)
    rng.shuffle(rows)
    srow = np.full(700, -1)
    srow[:rows.size] = rows
    srow[rng.rand(700) < 0.12] = -1
    named = srow[srow >= 0].copy()
    flag = (srow >= 0) & (rng.rand(700) < 0.2)
    srow[flag] |= FBN_SLOT_FLAG
    F = c.lag_max
    st = c.state()
    call("fbn_adam_catchup", ptr(st[0]), ptr(st[1]), ptr(st[2]), NROWS, c.D, ptr(_i32(srow, hip_device)), 700,
         None, F, 1, *c.tail(st, c.T), _lib.stream_handle(hip_device))
    c.check(st, _targets(named, c.T))


# ------------------------------------------------------------------------------- fbn_adam_claim_catchup
@pytest.mark.parametrize("pre", [0, 1], ids=["cas", "preclaimed"])
@_cases(D_ALL)
def test_claim_catchup(hip_device, cfg, pre):
    c = _case(hip_device, *cfg)
    dev = hip_device
    B, L = 33, 20
    n = B * (L + 1)
    item, seq, ent, _ = _batch(11, dev, B, L)
    st = c.state()
    cmap = _i32(np.full(NROWS, -1), dev)
    if pre:     # the previous step's prefetch of this very batch: tags for step T, the rows brought to T
        call("fbn_adam_prefetch", ptr(item), ptr(seq), B, L, NROWS, ptr(cmap), st[3].data_ptr(), ptr(st[0]),
             ptr(st[1]), ptr(st[2]), c.D, *c.tail(st, c.T - 1), _lib.stream_handle(dev))
    srow = _i32(np.full(n, -1), dev)
    dup = _i32(np.full(n, 7), dev)
    hasdup = _i32(np.zeros(n), dev)
    call("fbn_adam_claim_catchup", ptr(item), ptr(seq), B, L, NROWS, ptr(cmap), ptr(srow), ptr(dup), ptr(hasdup),
         st[3].data_ptr() if pre else None, ptr(st[0]), ptr(st[1]), ptr(st[2]), NROWS, c.D, c.lag_max,
         *c.tail(st, c.T), _lib.stream_handle(dev))
    c.check(st, _targets(ent[ent > 0], c.T))
    cmap, srow, dup, hasdup = (t.cpu().numpy() for t in (cmap, srow, dup, hasdup))
    exp_map = np.full(NROWS, -1)
    for r in np.unique(ent[ent > 0]):
        es = np.nonzero(ent == r)[0]
        cl = cmap[r]
        assert cl in es, f"row {r}: claimer {cl} is no entry naming it"
        if pre:
            assert cl == es.min(), f"row {r}: a pre-claimed row goes to its smallest entry, got {cl}"
        assert srow[cl] == r and dup[cl] == -1
        others = es[es != cl]
        assert (dup[others] == cl).all() and (srow[others] == -1).all()
        assert hasdup[cl] == (1 if others.size else 0)
        exp_map[r] = cl
    assert (cmap == exp_map).all()
    pad = np.nonzero(ent <= 0)[0]
    assert (dup[pad] == -1).all() and (srow[pad] == -1).all() and (hasdup[pad] == 0).all()


# ------------------------------------------------------------------------- fbn_adam_owner_claim_catchup
@pytest.mark.parametrize("skip0", [0, 1])
@_cases([16, 128, 256])
def test_owner_claim_catchup(hip_device, cfg, skip0):
    c = _case(hip_device, *cfg)
    dev = hip_device
    lids = _lids(21)
    n = lids.size
    st = c.state()
    cmap = _i32(np.full(NROWS, -1), dev)
    srow = _i32(np.full(n, -1), dev)
    call("fbn_adam_owner_claim_catchup", ptr(_i32(lids, dev)), n, skip0, ptr(cmap), ptr(srow), None, ptr(st[0]),
         ptr(st[1]), ptr(st[2]), NROWS, c.D, c.lag_max, *c.tail(st, c.T), _lib.stream_handle(dev))
    valid = (lids >= 0) & ~((lids == 0) & bool(skip0))
    c.check(st, _targets(lids[valid], c.T))
    cmap, srow = cmap.cpu().numpy(), srow.cpu().numpy()
    for r in np.unique(lids[valid]):
        cl = cmap[r]
        assert lids[cl] == r and srow[cl] == r
    assert (srow >= 0).sum() == np.unique(lids[valid]).size
    assert (cmap >= 0).sum() == np.unique(lids[valid]).size


# ------------------------------------------------------------------------------------- the prefetch family
def _claimed_map(pool, dev):
    """map with a third of the pool's ids claimed by "this batch"."""
    cmap = np.full(NROWS, -1)
    cmap[pool[::3]] = 2
    return cmap


def _check_tags(st, ent, target):
    """the two-pass forms post (target << 32) | (0xFFFFFFFF - smallest entry index) for every id the
    entries ent name (<= 0: none)"""
    tags = st[3].cpu().numpy().view(np.uint32)
    ids = ent[ent > 0]
    for r in np.unique(ids):
        first = int(np.nonzero(ent == r)[0].min())
        assert int(tags[r, 1]) == target and int(tags[r, 0]) == 0xFFFFFFFF - first, f"row {r}: pre-claim tag"
    rest = np.setdiff1d(np.arange(NROWS), ids)
    assert (tags[rest, 0] == 123).all() and (tags[rest, 1] == 1).all()


def _prefetch(c, dev, pre, binned=False):
    B, L = 33, 20
    item, seq, ent, pool = _batch(31, dev, B, L)
    cmap = _claimed_map(pool, dev)
    st = c.state()
    head = (ptr(item), ptr(seq), B, L, NROWS, ptr(_i32(cmap, dev)), st[3].data_ptr() if pre else None,
            ptr(st[0]), ptr(st[1]), ptr(st[2]), c.D, *c.tail(st, c.pf_target - 1))
    if binned:
        nb = _lib.lib().fbn_adam_prefetch_binned_ws_size(B * (L + 1))
        ws = torch.full(((nb + 3) // 4,), 0x55555555, dtype=torch.int32, device=dev)
        call("fbn_adam_prefetch_binned", *head, ptr(ws), ws.numel() * 4, _lib.stream_handle(dev))
    else:
        call("fbn_adam_prefetch", *head, _lib.stream_handle(dev))
    ids = ent[ent > 0]
    c.check(st, _targets(ids[cmap[ids] == -1], c.pf_target))
    if pre:
        _check_tags(st, ent, c.pf_target)
    else:
        assert torch.equal(st[3][:, :2], c.base[3][:, :2])


@_cases(D_ALL)
def test_prefetch_two_pass(hip_device, cfg):
    _prefetch(_case(hip_device, *cfg), hip_device, pre=True)


@_cases(D_WIDE)
def test_prefetch_one_pass(hip_device, cfg):
    _prefetch(_case(hip_device, *cfg), hip_device, pre=False)


@_cases(D_WIDE)
def test_prefetch_binned(hip_device, cfg):
    _prefetch(_case(hip_device, *cfg), hip_device, pre=True, binned=True)


@pytest.mark.parametrize("pre", [0, 1], ids=["one_pass", "two_pass"])
@_cases(D_WIDE, large=False)
def test_prefetch_rows(hip_device, cfg, pre):
    c = _case(hip_device, *cfg)
    dev = hip_device
    lids = _lids(41)
    skip0 = 1
    valid = (lids > 0)
    cmap = np.full(NROWS, -1)
    cmap[np.unique(lids[valid])[::3]] = 4
    st = c.state()
    call("fbn_adam_prefetch_rows", ptr(_i32(lids, dev)), lids.size, skip0, NROWS, ptr(_i32(cmap, dev)),
         st[3].data_ptr() if pre else None, ptr(st[0]), ptr(st[1]), ptr(st[2]), c.D,
         *c.tail(st, c.pf_target - 1), _lib.stream_handle(dev))
    ids = lids[valid]
    c.check(st, _targets(ids[cmap[ids] == -1], c.pf_target))
    if pre:
        _check_tags(st, lids, c.pf_target)


# -------------------------------------------------------------------------------------- argument errors
def test_argument_errors(hip_device):
    """The argument-error returns, code by code; none of them launches device work."""
    dev = hip_device
    c = _case(dev, 128, 0, "small")
    L = _lib.lib()
    s = _lib.stream_handle(dev)
    st = c.state()
    p, m, v = ptr(st[0]), ptr(st[1]), ptr(st[2])
    tail = c.tail(st, c.T)
    no_ring = tail[:7] + (None,) + tail[8:]                       # pend without a ring
    small_ring = tail[:10] + (F_WIN,) + tail[11:]                 # ring_n <= F
    item, seq, _, _ = _batch(11, dev)
    cmap = _i32(np.full(NROWS, -1), dev)
    srow = _i32(np.full(700, -1), dev)
    lids = _i32(_lids(21), dev)
    pre = st[3].data_ptr()
    catchup = lambda D, F, parts, t: L.fbn_adam_catchup(p, m, v, NROWS, D, ptr(srow), 700, ptr(cmap), F, parts, *t, s)
    claim = lambda D, F, t: L.fbn_adam_claim_catchup(ptr(item), ptr(seq), 33, 20, NROWS, ptr(cmap), ptr(srow), None,
                                                     None, None, p, m, v, NROWS, D, F, *t, s)
    owner = lambda D, F, t: L.fbn_adam_owner_claim_catchup(ptr(lids), 700, 0, ptr(cmap), ptr(srow), None, p, m, v,
                                                           NROWS, D, F, *t, s)
    pf = lambda D, pr, t: L.fbn_adam_prefetch(ptr(item), ptr(seq), 33, 20, NROWS, ptr(cmap), pr, p, m, v, D, *t, s)
    rows = lambda D, pr, t: L.fbn_adam_prefetch_rows(ptr(lids), 700, 0, NROWS, ptr(cmap), pr, p, m, v, D, *t, s)
    nb = L.fbn_adam_prefetch_binned_ws_size(693)
    ws = torch.zeros((nb + 3) // 4, dtype=torch.int32, device=dev)
    binned = lambda D, pr, t, w, wb: L.fbn_adam_prefetch_binned(ptr(item), ptr(seq), 33, 20, NROWS, ptr(cmap), pr, p,
                                                                m, v, D, *t, w, wb, s)
    got = {
        "catchup F=0": catchup(128, 0, 2, tail), "catchup F=513": catchup(128, 513, 1, tail),
        "claim F=513": claim(128, 513, tail), "owner F=0": owner(128, 0, tail),
        "catchup no ring": catchup(128, F_WIN, 2, no_ring), "claim no ring": claim(128, F_WIN, no_ring),
        "owner no ring": owner(128, F_WIN, no_ring), "prefetch no ring": pf(128, pre, no_ring),
        "rows no ring": rows(128, pre, no_ring), "binned no ring": binned(128, pre, no_ring, ptr(ws), nb),
        "catchup ring_n<=F": catchup(128, F_WIN, 1, small_ring), "claim ring_n<=F": claim(128, F_WIN, small_ring),
        "owner ring_n<=F": owner(128, F_WIN, small_ring),
        "catchup parts=3": catchup(128, F_WIN, 3, tail),
        "prefetch D=48": pf(48, pre, tail), "rows D=64": rows(64, pre, tail), "binned D=64": binned(64, pre, tail, ptr(ws), nb),
        "prefetch one-pass D=16": pf(16, None, tail),
        "binned ws too small": binned(128, pre, tail, ptr(ws), nb - 16), "binned no ws": binned(128, pre, tail, None, nb),
        "binned no preclaim": binned(128, None, tail, ptr(ws), nb),
    }
    unsupported = {
        "catchup D=48": catchup(48, F_WIN, 1, tail), "window D=48": catchup(48, F_WIN, 2, tail),
        "claim D=48": claim(48, F_WIN, tail), "owner D=48": owner(48, F_WIN, tail),
        "flush D=48": L.fbn_adam_flush(p, m, v, NROWS, 48, *tail, s),
    }
    assert got == {k: FBN_ERR_ARG for k in got}
    assert unsupported == {k: FBN_ERR_UNSUPPORTED for k in unsupported}
    c.check(st, np.full(NROWS, -1, dtype=np.int64))               # nothing ran
