"""The optimizer reference of tests/_adam_ref.py checked without a GPU: against torch itself (float64 Adam /
AdamW + clip_grad_norm_ + OneCycleLR), its bounds against an honest float32 evaluation, the library's float32
schedule table against it, and the hand-built claims against index_add_.  test_gpu_adam.py then holds the
kernels to the same reference and bounds.

The last test turns the bounds on float32 steps that are wrong on purpose -- the schedule row of the next step,
wd p joined before the clip multiply, eps lost, b2 where 1 - b2 belongs, the n % 4 tail skipped -- and asserts
that each one breaks them: a bound that a wrong kernel meets checks nothing.
"""
import math

import numpy as np
import pytest
import torch

from ctr_recommendation_amd import schedule
from tests import _adam_ref as ar

TOTAL = 20            # the schedule: phase 1 ends at step index 0.3 * 20 - 1 = 5
U = ar.U


# ------------------------------------------------------------------------------- trajectory against torch
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_trajectory_matches_torch(decoupled):
    """12 steps of the 20-step schedule (across the phase boundary at step 5) on two tensors, the gradients a
    fixed sequence whose scale makes some steps clip and some not: p, m, v to 1e-12 relative, element by
    element.  Pins: wd joins after the clip, step t runs the scheduler's values of index t - 1, the bias
    corrections use t."""
    wd, max_norm, steps = ar.WD, 1.0, 12
    gen = torch.Generator().manual_seed(5)
    shapes = [(37,), (8, 16)]
    init = [0.1 * torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    scale = [0.02, 0.5, 0.05, 0.3, 0.01, 0.2, 0.04, 0.6, 0.03, 0.08, 0.4, 0.02]
    grads = [[sc * torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes] for sc in scale]
    # ---- torch
    params = [torch.nn.Parameter(t.clone()) for t in init]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(params, lr=1e-3, betas=(0.9, ar.BETA2), eps=ar.EPS, weight_decay=wd)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-2, total_steps=TOTAL, pct_start=0.3, div_factor=25.0,
                                              final_div_factor=1000.0)
    # ---- the reference
    ks = ar.step_consts(TOTAL, 1e-3, ar.BETA2, wd, decoupled)
    p = [t.clone() for t in init]
    m = [torch.zeros_like(t) for t in init]
    v = [torch.zeros_like(t) for t in init]
    clipped = []
    for s in range(steps):
        for q, g in zip(params, grads[s]):
            q.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        sch.step()
        norm, coef = ar.clip_ref([float((g * g).sum()) for g in grads[s]], max_norm)
        clipped.append(coef < 1.0)
        for i in range(len(p)):
            p[i], m[i], v[i], _ = ar.adam_step_ref(p[i], m[i], v[i], grads[s][i], coef, ks[s], wd, ar.BETA2, ar.EPS,
                                                   decoupled)
        for i, q in enumerate(params):
            st = opt.state[q]
            for name, got, want in (("p", p[i], q.detach()), ("m", m[i], st["exp_avg"]), ("v", v[i], st["exp_avg_sq"])):
                rel = float(((got - want).abs() / want.abs()).max())
                assert rel <= 1e-12, f"step {s + 1} tensor {i} {name}: {rel:.3e} relative"
    assert any(clipped) and not all(clipped), clipped
    assert ks[5].lr > ks[4].lr and ks[5].lr > ks[6].lr              # the phase boundary lies inside the 12 steps


def test_clip_ref_overflow_matches_float32_torch():
    """A sum of squares past float32's range: torch's float32 norm is inf and the coefficient 0."""
    g = torch.full((4,), 1e30, dtype=torch.float32)
    q = torch.nn.Parameter(torch.zeros(4))
    q.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_([q], 1.0)
    assert math.isinf(float(total)) and bool((q.grad == 0).all())
    assert ar.clip_ref([float((g.double() ** 2).sum())], 1.0) == (math.inf, 0.0)
    assert ar.clip_ref([0.0], 1.0) == (0.0, 1.0)


# ---------------------------------------------------------------------------- float32 evaluation vs bounds
CASES32 = [(t, dw, coef) for t in (1, 8, 12) for dw in (False, True) for coef in (1.0, 0.37)]


def _ratios(fn, t, decoupled, coef, n=4099, seed=1):
    """Worst error / bound of a float32 step ``fn`` (adam_elem_f32's signature) for m, v, p."""
    ks = ar.step_consts(TOTAL, 1e-3, ar.BETA2, ar.WD, decoupled)
    k = ks[t - 1]
    coef = ar.f32(coef)
    p, m, v, g = ar.make_state(n, seed, ar.WD, coef, decoupled)
    ref = ar.adam_step_ref(p, m, v, g, coef, k, ar.WD, ar.BETA2, ar.EPS, decoupled)
    e_m, e_v, e_p = ar.step_bounds(p, m, v, g, coef, k, ar.WD, ar.BETA2, ar.EPS, decoupled)
    got = fn(p, m, v, g, coef, ks, t, decoupled)
    out = {}
    for name, x, r, e in (("m", got[1], ref[1], e_m), ("v", got[2], ref[2], e_v), ("p", got[0], ref[0], e_p)):
        out[name], nan = ar.ratio(x, r, e)
        assert not nan
    return out


def _honest(p, m, v, g, coef, ks, t, decoupled):
    return ar.adam_elem_f32(p, m, v, g, coef, ar.table_row_f32(ks[t - 1], ar.WD, decoupled), ar.WD, ar.BETA2, ar.EPS,
                            decoupled)


@pytest.mark.parametrize("t,decoupled,coef", CASES32)
def test_float32_evaluation_sits_inside_the_bounds(t, decoupled, coef):
    """adam_elem's operation order in float32 torch on every generated input, the planted edges included."""
    r = _ratios(_honest, t, decoupled, coef)
    print(f"[adam-ratio] f32-host t={t} dw={int(decoupled)} coef={coef} m={r['m']:.4f} v={r['v']:.4f} p={r['p']:.4f}")
    assert max(r.values()) <= 1.0, r


def test_generated_edges_are_what_they_claim():
    for decoupled in (False, True):
        k = ar.step_consts(TOTAL, 1e-3, ar.BETA2, ar.WD, decoupled)[7]
        p, m, v, g = ar.make_state(64, 1, ar.WD, 1.0, decoupled)
        _, m1, v1, g1 = ar.adam_step_ref(p, m, v, g, 1.0, k, ar.WD, ar.BETA2, ar.EPS, decoupled)
        assert m[0] == 0 and v[0] == 0 and g[0] != 0 and m[1] == 0 and v[1] == 0 and g[1] == 0 and g[2] == 0
        if not decoupled:
            assert abs(float(g1[3] - m[3].double())) < 2.0 ** -16 * abs(float(m[3]))         # m and g' nearly cancel
            assert float(g1[1]) != 0.0                                                     # g' = wd p alone
        assert 0 < float(v[4]) < ar.FLT_MIN and 0 < float(v1[4]) < ar.FLT_MIN
        assert abs(float(p[5])) > 3.9 and abs(float(p[6])) > 3.9 and float(v[7]) == 0.0


# ------------------------------------------------------------------------------------- the schedule table
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_schedule_table_is_step_consts_rounded_once(decoupled):
    """Every float32 column of schedule.adam_table within u relative of the double value read off torch: the
    rounding the GPU tests charge to the bound while they take their expectations from step_consts."""
    tab, lrs = schedule.adam_table(TOTAL, 1e-3, ar.BETA2, decoupled_wd=ar.WD if decoupled else 0.0)
    ks = ar.step_consts(TOTAL, 1e-3, ar.BETA2, ar.WD, decoupled)
    assert tab.dtype == np.float32 and tab.shape == (TOTAL + 1, 8)
    for k in ks:
        want = [1.0 - k.b1, -(k.lr / k.bc1), math.sqrt(k.bc2), 1.0 / math.sqrt(k.bc2),
                1.0 - k.lr * ar.WD if decoupled else 1.0]
        for col, w in enumerate(want):
            got = float(tab[k.t - 1, col])
            assert abs(got - w) <= U * abs(w), f"step {k.t} column {col}: {got!r} vs {w!r}"
        assert abs(lrs[k.t - 1] - k.lr) <= 1e-15
    assert (tab[:, 5:] == 0).all() and (tab[TOTAL] == tab[TOTAL - 1]).all()
    if not decoupled:
        assert (tab[:, 4] == 1.0).all()


# ---------------------------------------------------------------------------------------- claim builder
@pytest.mark.parametrize("layout,full,bf16", [("vec", False, False), ("vec", True, False), ("rows", False, False),
                                              ("rows", True, False), ("rows", False, True)])
@pytest.mark.parametrize("D", [16, 128])
def test_claim_builder(layout, full, bf16, D):
    B, L, V = 8, 20, 400
    ids = ar.entry_ids(B, L, V, seed=3)
    flat = ids.reshape(-1)
    n = flat.size
    c = ar.make_claims(flat, V, D, seed=D + 1, B=B if layout == "vec" else None, L=L if layout == "vec" else None,
                       full=full, bf16=bf16)
    # ---- float64 index_add_ of every entry's vector
    vecs = c.gvec.view(-1, D).double()[torch.from_numpy(c.vec_of)]
    live = torch.from_numpy((flat > 0) & (flat < V))
    want = torch.zeros((V, D), dtype=torch.float64)
    want.index_add_(0, torch.from_numpy(flat)[live], vecs[live])
    absum = torch.zeros((V, D), dtype=torch.float64)
    absum.index_add_(0, torch.from_numpy(flat)[live], vecs[live].abs())
    rows = torch.from_numpy(c.rows)
    assert torch.equal(c.grad_all, want[rows])
    # grad differs from it by extra's one rounding to float32 at most
    assert bool(((c.grad - want[rows]).abs() <= U * absum[rows]).all())
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[rows] = False
    assert bool((want[untouched] == 0).all()) and bool((c.map[untouched] == -1).all())
    # ---- each touched row claimed exactly once, by an entry that names it; row 0 never
    sr = c.slot_row.numpy()
    claimed = sr[sr != -1] & ~ar.FBN_SLOT_FLAG
    assert np.array_equal(np.sort(claimed), c.rows) and 0 not in claimed and int(c.map[0]) == -1
    assert (flat == 0).any() and c.flagged.any() and not c.flagged.all()
    for i, r in enumerate(c.rows):
        cl = int(c.map[r])
        assert cl == c.claimer[i] and flat[cl] == r
        dups = int((flat == r).sum()) - 1
        assert bool(sr[cl] & ar.FBN_SLOT_FLAG) == (dups > 0) == bool(c.flagged[i])
        assert (sr[cl] & ~ar.FBN_SLOT_FLAG) == r
        if not dups:
            assert bool((c.extra[cl] == 0).all()) and bool((c.grad_err[i] == 0).all())
    assert bool((c.extra[torch.from_numpy(sr == -1)] == 0).all())
    if layout == "vec":                                   # entry e = b (L + 1) + t reads vector 2 b + (t > 0)
        e = 5 * (L + 1)
        assert c.vec_of[e] == 10 and c.vec_of[e + 1] == 11 and c.vec_of[e + L] == 11 and c.lp1 & 0xffff == L + 1
    else:
        assert c.lp1 & 0xffff == 1 and bool(c.lp1 & ar.FBN_GRAD_BF16) == bf16
    if bf16:
        assert torch.equal(c.gvec_store[:n * D].float().view(n, D), c.gvec) and c.gvec_store.numel() == n * D + 16
    assert bool(c.lp1 & ar.FBN_GRAD_FULL) == full
    assert c.rs.shape == (V, 4) and bool((c.rs[:, 3] == -1).all())


# ------------------------------------------------------------------------------- the bounds have teeth
def _mutant(name):
    def fn(p, m, v, g, coef, ks, t, decoupled):
        f = lambda x: torch.tensor(float(x), dtype=torch.float32)
        row = ar.table_row_f32(ks[t if name == "next_row" else t - 1], ar.WD, decoupled)
        wd, beta2, eps = ar.WD, ar.BETA2, ar.EPS
        if name == "no_eps":
            eps = 0.0
        if name in ("next_row", "no_eps"):
            return ar.adam_elem_f32(p, m, v, g, coef, row, wd, beta2, eps, decoupled)
        if name == "skip_tail":
            q = list(ar.adam_elem_f32(p, m, v, g, coef, row, wd, beta2, eps, decoupled))
            n4 = p.numel() // 4 * 4
            for x, old in zip(q, (p, m, v)):
                x[n4:] = old[n4:]
            return q
        w1, nss, bc2s = f(row[0]), f(row[1]), f(row[2])
        b2 = f(beta2)
        omb2 = f(1.0 - float(b2))
        p, m, v, g = (x.float() for x in (p, m, v, g))
        if name == "wd_before_clip":
            g = (g + f(wd) * p) * f(coef)
        else:
            g = g * f(coef) + f(wd) * p
        m = m + w1 * (g - m)
        v = v * omb2 + (b2 * g) * g if name == "b2_swapped" else v * b2 + (omb2 * g) * g
        return p + (nss * m) / (v.sqrt() / bc2s + f(eps)), m, v
    return fn


@pytest.mark.parametrize("name", ["next_row", "wd_before_clip", "no_eps", "b2_swapped", "skip_tail"])
def test_bounds_reject_wrong_steps(name):
    """Step 8 of 20 (both neighbours' constants differ), Adam with wd = 1e-2, coef = 0.37, n = 4099 (a tail of 3)."""
    r = _ratios(_mutant(name), 8, False, 0.37)
    print(f"[adam-ratio] mutant {name} m={r['m']:.3g} v={r['v']:.3g} p={r['p']:.3g}")
    assert max(r.values()) > 1.0, r
