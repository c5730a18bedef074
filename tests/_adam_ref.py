"""The float64 reference, the derived error bounds, the hand-built claims and the inputs shared by the
optimizer tests (test_adam_ref_host.py, test_gpu_adam.py).

Plain torch / numpy on the CPU; no project kernel is involved, and ctr_recommendation_amd.schedule is the
source of no expected value: ``step_consts`` reads lr and beta1 off a real torch OneCycleLR driving a real
torch Adam / AdamW (the arguments of tests/test_oracle.py::test_schedule_matches_torch_onecycle_and_adam),
``adam_step_ref`` is one step of torch's single-tensor Adam written out in float64 and ``clip_ref`` is
clip_grad_norm_'s coefficient.  test_adam_ref_host.py holds those three against torch itself.

Semantics (optimizer step t = 1, 2, ...; the device step counter and the schedule table row are t - 1):
  g' = g coef + wd p          (Adam: the L2 term joins AFTER the clip)     AdamW: p <- p (1 - lr wd), g' = g coef
  m' = m + (1 - b1) (g' - m)                        b1, lr: the scheduler's values of index t - 1
  v' = b2 v + (1 - b2) g'^2
  p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)        bc1 = 1 - b1^t, bc2 = 1 - b2^t

Error bounds (``step_bounds``).  First-order running error analysis of the arithmetic adam_tab1 (csrc/optim.hip)
documents, u = 2^-24, as tests/_fields_ref.py does it: every float32 operation contributes u |result|, a
float32 constant u |constant|, and an operand's error is carried through by the absolute value of the partial
derivative.  The kernel's step and its roundings, in order:
  gc  = g * coef                      1 (the product)                       [+ the caller's g_err, times coef]
  g'  = fma(wd, p, gc)                1 (the fma) + 1 on wd p (float(wd))   [2 on wd p unfused: + its product]
  p1  = p * dmul (AdamW only)         2: float(dmul) and the product; Adam: dmul = 1, exact
  d   = g' - m                        1
  m'  = fma(w1, d, m)                 1 (the fma) + 1 on w1 d (float(w1))   [2 on w1 d unfused]
  t   = omb2 * g'                     1 + omb2's own error (below)
  v'  = fma(t, g', v * b2)            1 (the fma) + 2 on b2 v (float(b2), the product)   [+ 1 on t g' unfused]
  s   = v_sqrt_f32(v')                1 ulp = 2 u; subnormal v': absolute sqrt(FLT_MIN) (the instruction does
                                      not take subnormals; 1e-19 against eps = 1e-8)
  den = fma(s, rbc2s, eps)            1 (the fma) + 1 on s rbc2s (float(rbc2s)) + 1 on eps (float(eps))
  q   = v_rcp_f32(den)                1 ulp = 2 u
  nm  = nss * m'                      2: float(nss) and the product
  p'  = fma(nm, q, p1)                1 (the fma): u |p'|
omb2 = float(1 - double(float(b2))): the C ABI takes beta2 as a float, so the kernel's 1 - b2 carries b2's
rounding, u b2 ABSOLUTE, and its own, u (1 - b2): relative u b2 / (1 - b2) + u (about 1000 u at b2 = 0.999).
"[... unfused]" is the extra product rounding of the same update without fused multiply-adds (adam_elem's
operation order, the float32 host evaluation test_adam_ref_host.py holds to the same bounds); the bounds
count the larger of the two, so both forms sit under them.  Results in the subnormal range round to
2^-149 absolute instead: TINY is added where an operand can be that small.
The p bound keeps its three parts apart -- |nss| e(m') / den (m' can cancel to nothing, so its error is no
relative one), the relative term on the update, u |p'| -- because |p| can be 4 beside an update of 1e-9.

Clip (``clip_bounds``): the squares are float32 products (u each; 3 u where a flagged row's float32 sum
gvec + extra is squared) summed in float64 (n 2^-53, counted), the total is cast to float (u), so the norm's
radicand carries 2 u and the norm u, + sqrtf (u: correctly rounded); norm + 1e-6f: float(1e-6) and the add;
the divide: u.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
FLT_MIN = 2.0 ** -126
FLT_MAX = float(np.finfo(np.float32).max)
FBN_SLOT_FLAG = 0x40000000
FBN_GRAD_FULL = 0x10000
FBN_GRAD_BF16 = 0x40000
FBN_SUMSQ_SLOTS = 64
BETA2, EPS, WD = 0.999, 1e-8, 1e-2


def f32(x):
    """The double value of x rounded to float32 (what a float argument of the C ABI carries)."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------- schedule
def step_consts(total_steps, base_lr=1e-3, beta2=BETA2, wd=0.0, decoupled=False):
    """Per optimizer step t = 1 .. total_steps (list index t - 1): lr and beta1 as a real OneCycleLR sets them
    on a real torch Adam / AdamW before that step, the bias corrections in double precision, and t."""
    p = torch.nn.Parameter(torch.zeros(3))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=base_lr, betas=(0.9, beta2), weight_decay=wd)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=10 * base_lr, total_steps=total_steps, pct_start=0.3,
                                              div_factor=25.0, final_div_factor=1000.0)
    out = []
    for t in range(1, total_steps + 1):
        grp = opt.param_groups[0]
        lr, b1 = float(grp["lr"]), float(grp["betas"][0])
        out.append(SimpleNamespace(t=t, lr=lr, b1=b1, bc1=1.0 - b1 ** t, bc2=1.0 - beta2 ** t))
        p.grad = torch.ones(3)
        opt.step()
        sch.step()
    return out


def table_row_f32(k, wd, decoupled):
    """The five float32 schedule constants of step k.t: (w1, nss, bc2s, rbc2s, dmul), each the double value
    rounded once."""
    return np.array([1.0 - k.b1, -(k.lr / k.bc1), math.sqrt(k.bc2), 1.0 / math.sqrt(k.bc2),
                     1.0 - k.lr * wd if decoupled else 1.0], dtype=np.float32)


# ------------------------------------------------------------------------------------------ reference
def adam_step_ref(p, m, v, g, coef, k, wd, beta2, eps, decoupled):
    """One step in float64 from float32 (or float64) tensors: (p', m', v', g').  coef: a float; k: one entry of
    step_consts; wd: the L2 coefficient (Adam) or the decoupled decay (AdamW)."""
    p, m, v, g = (t.detach().double() for t in (p, m, v, g))
    if decoupled:
        p1 = p * (1.0 - k.lr * wd)
        g1 = g * coef
    else:
        p1 = p
        g1 = g * coef + wd * p
    m1 = m + (1.0 - k.b1) * (g1 - m)
    v1 = beta2 * v + (1.0 - beta2) * g1 * g1
    den = v1.sqrt() / math.sqrt(k.bc2) + eps
    return p1 - (k.lr / k.bc1) * m1 / den, m1, v1, g1


def adam_elem_f32(p, m, v, g, coef, row, wd, beta2, eps, decoupled):
    """The same step in float32 torch on the CPU, adam_elem's operation order (no fused multiply-add, IEEE
    square root and division), from the float32 schedule row (w1, nss, bc2s, rbc2s, dmul): (p', m', v')."""
    f = lambda x: torch.tensor(float(x), dtype=torch.float32)
    w1, nss, bc2s, dmul = f(row[0]), f(row[1]), f(row[2]), f(row[4])
    b2 = f(beta2)
    omb2 = f(1.0 - float(b2))
    wd_l2 = f(0.0 if decoupled else wd)
    p, m, v, g = (t.detach().float() for t in (p, m, v, g))
    g = g * f(coef)
    g = g + wd_l2 * p
    p = p * dmul
    m = m + w1 * (g - m)
    v = v * b2
    v = v + (omb2 * g) * g
    den = v.sqrt() / bc2s + f(eps)
    return p + (nss * m) / den, m, v


def step_bounds(p, m, v, g, coef, k, wd, beta2, eps, decoupled, g_err=None):
    """Bounds on |m' - ref|, |v' - ref|, |p' - ref| of a float32 evaluation (module docstring): (e_m, e_v, e_p).
    g_err: an absolute error the gradient carries before the clip multiply (a flagged row's float32 sum)."""
    p_, m_, v_, g_ = (t.detach().double() for t in (p, m, v, g))
    p1, m1, v1, g1 = adam_step_ref(p, m, v, g, coef, k, wd, beta2, eps, decoupled)
    w1, nss, r = 1.0 - k.b1, k.lr / k.bc1, 1.0 / math.sqrt(k.bc2)
    ge = torch.zeros_like(g_) if g_err is None else g_err.double()
    gc = (g_ * coef).abs()
    wdp = torch.zeros_like(p_) if decoupled else (wd * p_).abs()
    # g': the caller's error through coef; gc: 1; wd p: 2 (float(wd) + the unfused product); the sum: 1
    e_g = abs(coef) * ge + U * gc + 2 * U * wdp + U * g1.abs() + TINY
    # p1 = p dmul: 2 under AdamW (float(dmul), the product); exact under Adam
    pd = p_ * (1.0 - k.lr * wd) if decoupled else p_
    e_p1 = 2 * U * pd.abs() if decoupled else torch.zeros_like(p_)
    # m': d = g' - m: 1; w1 d: 2 (float(w1) + the unfused product); the sum: 1
    d = g1 - m_
    e_m = w1 * (e_g + U * d.abs()) + 2 * U * (w1 * d).abs() + U * m1.abs() + TINY
    # v': b2 v: 2 (float(b2), the product); (1 - b2) g'^2: omb2's error + 1 (omb2 g') + 1 (the unfused
    # product with g'); g' enters squared; the sum: 1
    omb2 = 1.0 - beta2
    r_o = U * beta2 / omb2 + U
    e_v = 2 * U * beta2 * v_.abs() + omb2 * (2 * g1.abs() * e_g + (r_o + 2 * U) * g1 * g1) + U * v1 + 2 * TINY
    # s = sqrt(v'): the operand's error by 1 / (2 sqrt(v')), 1 ulp = 2 u of the instruction; where v' (or what the
    # kernel holds for it) can be subnormal the instruction may return anything in [0, sqrt(2 FLT_MIN)]
    s = v1.sqrt()
    sub = v1 - e_v < 2 * FLT_MIN
    e_s = torch.where(sub, torch.full_like(s, 2 * math.sqrt(FLT_MIN)),
                      e_v / (2 * s.clamp_min(math.sqrt(FLT_MIN))) + 2 * U * s)
    # den = s rbc2s + eps: 1 on s rbc2s (float(rbc2s)), 1 on eps (float(eps)), the fma: 1
    den = s * r + eps
    e_den = r * e_s + U * s * r + U * eps + U * den
    # p' = p1 - nss m' / den: nss e(m') / den explicitly; the relative term: float(nss) 1, nss m' 1, den's, the
    # reciprocal 1 ulp = 2 u (the unfused form: the division 1); the fma: u |p'|
    upd = nss * m1 / den
    e_p = e_p1 + nss * e_m / den + upd.abs() * (4 * U + e_den / den) + U * p1.abs() + TINY
    return e_m, e_v, e_p


# ----------------------------------------------------------------------------------------------- clip
def clip_ref(sumsq_parts, max_norm):
    """(norm, coef) of clip_grad_norm_ from partial sums of squares, in float64; a total past float32's range
    gives (inf, 0), as the float32 norm torch clips with."""
    s = float(np.sum(np.asarray(sumsq_parts, dtype=np.float64)))
    if s > FLT_MAX * (1 + U / 2):          # rounds to inf as a float
        return math.inf, 0.0
    norm = math.sqrt(s)
    return norm, min(1.0, max_norm / (norm + 1e-6))


def clip_bounds(sumsq_parts, max_norm, n_terms=0, sq_roundings=1):
    """(e_norm, e_coef).  Radicand: sq_roundings u (what produced the squares: 1 for a float32 product, 3 where a
    float32 sum was squared, 0 when the parts ARE the kernel's slots) + n_terms 2^-53 (the float64 additions) +
    u (the cast): half of it on the norm, + u (sqrtf).  Denominator: u 1e-6 (float(1e-6)) + u (the add); the
    divide: u."""
    norm, coef = clip_ref(sumsq_parts, max_norm)
    if math.isinf(norm):
        return 0.0, 0.0
    e_norm = norm * (((sq_roundings + 1) * U + (n_terms + FBN_SUMSQ_SLOTS) * 2.0 ** -53) / 2 + U)
    den = norm + 1e-6
    e_den = e_norm + U * 1e-6 + U * den
    x = max_norm / den
    return e_norm, x * (e_den / den + U)          # min(1, .) is 1-Lipschitz


def sumsq_bound(total, n_terms, pre_total=0.0, sq_roundings=1):
    """Bound on |(slots after - slots before).sum() - total| for a kernel that adds a sum of ``total`` into the 64
    slots holding pre_total: sq_roundings u per square (clip_bounds), n_terms float64 additions on the way, up
    to 64 atomic additions per slot, each rounding at the slot's size, and the test's own 64 subtractions and
    their sum."""
    eps64 = 2.0 ** -53
    return (sq_roundings * U + n_terms * eps64) * total + eps64 * (64 * (pre_total + total) + 65 * total)


# --------------------------------------------------------------------------------------------- claims
def make_claims(ids, V, D, seed, B=None, L=None, full=False, bf16=False, step=0, gscale=0.05):
    """The sparse-gradient layout of one step built by hand from the entries' row ids ``ids`` [n] (<= 0 or
    >= V: no row).  B, L given: per-sample vectors gvec [B][2][D], n = B (L + 1), Lp1 = L + 1, entry
    e = b Lp1 + t reads vector 2 b + (t > 0); else per-entry rows gvec [n][D], Lp1 = 1 (bf16: stored as bf16,
    16 elements of padding behind the last row).  Each named row is claimed by ONE of its entries, picked at
    random (the kernels' claim is a race: any of them may win): map[row] = that entry, slot_row[entry] = row,
    with FBN_SLOT_FLAG when other entries name the row too; extra[entry] is then the float32 sum of those
    others' vectors, or under ``full`` (FBN_GRAD_FULL) of all of them, the claimer's included.
    Returns map, slot_row, extra, gvec (gvec_store: the padded bf16 buffer), lp1 (flags included), rs [V][4]
    int32 row-state records {tag lo, tag hi, last, pend} = {123, 1, step, -1}, rows (the claimed rows, sorted),
    claimer [rows], flagged [rows], and per claimed row in that order:
      grad     float64 [rows][D]  what the kernels must consume: gvec(claimer) + extra, or extra under full
      grad_err float64 [rows][D]  the error bound of the kernels' float32 sum: u |grad| on a flagged row without
                                  full, else 0
      grad_all float64 [rows][D]  the float64 sum over every entry naming the row (what index_add_ gives)."""
    ids = np.asarray(ids, dtype=np.int64)
    n = ids.size
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    per_sample = B is not None
    if per_sample:
        assert n == B * (L + 1) and not bf16
        gvec = gscale * torch.randn((B, 2, D), generator=g)
        e = np.arange(n)
        vec_of = 2 * (e // (L + 1)) + (e % (L + 1) > 0)
        flat = gvec.view(2 * B, D)
        lp1 = L + 1
    else:
        gvec = gscale * torch.randn((n, D), generator=g)
        if bf16:
            gvec = gvec.bfloat16().float()
        vec_of = np.arange(n)
        flat = gvec
        lp1 = 1 | (FBN_GRAD_BF16 if bf16 else 0)
    c = SimpleNamespace(n=n, V=V, D=D, B=B, L=L, full=full, bf16=bf16, lp1=lp1 | (FBN_GRAD_FULL if full else 0))
    c.map = torch.full((V,), -1, dtype=torch.int32)
    c.slot_row = torch.full((n,), -1, dtype=torch.int32)
    c.extra = torch.zeros((n, D), dtype=torch.float32)
    live = (ids > 0) & (ids < V)
    rows = np.unique(ids[live])
    claimer = np.zeros(rows.size, dtype=np.int64)
    flagged = np.zeros(rows.size, dtype=bool)
    grad = torch.zeros((rows.size, D), dtype=torch.float64)
    grad_err, grad_all = torch.zeros_like(grad), torch.zeros_like(grad)
    f64 = flat.double()
    for i, r in enumerate(rows):
        es = np.nonzero(live & (ids == r))[0]
        cl = int(es[rng.randint(es.size)])
        claimer[i] = cl
        c.map[r] = cl
        others = es[es != cl]
        grad_all[i] = f64[vec_of[es]].sum(0)
        if others.size:
            flagged[i] = True
            c.slot_row[cl] = int(r) | FBN_SLOT_FLAG
            c.extra[cl] = (grad_all[i] if full else f64[vec_of[others]].sum(0)).float()
            if full:
                grad[i] = c.extra[cl].double()
            else:
                grad[i] = f64[vec_of[cl]] + c.extra[cl].double()
                grad_err[i] = U * grad[i].abs()
        else:
            c.slot_row[cl] = int(r)
            grad[i] = f64[vec_of[cl]]
    c.rows, c.claimer, c.flagged = rows, claimer, flagged
    c.grad, c.grad_err, c.grad_all = grad, grad_err, grad_all
    c.vec_of = vec_of
    c.gvec = gvec
    c.gvec_store = None
    if bf16:
        c.gvec_store = torch.zeros(n * D + 16, dtype=torch.bfloat16)
        c.gvec_store[:n * D] = gvec.flatten().bfloat16()
    rs = torch.empty((V, 4), dtype=torch.int32)
    rs[:, 0], rs[:, 1], rs[:, 2], rs[:, 3] = 123, 1, step, -1
    c.rs = rs
    return c


def entry_ids(B, L, V, seed, pool=None, pad=0.1):
    """ids [B][L + 1] (column 0: the item, then the history) drawn from a pool of ``pool`` rows of [1, V) so
    that rows repeat, with id 0 padding; entry 3 is padding and entries 0, 1 name one row."""
    rng = np.random.RandomState(seed)
    pool = pool or max(2, (B * (L + 1)) // 3)
    rows = rng.choice(np.arange(1, V), min(pool, V - 1), replace=False)
    ids = rows[rng.randint(0, rows.size, size=(B, L + 1))]
    ids[rng.rand(B, L + 1) < pad] = 0
    flat = ids.reshape(-1)
    if flat.size > 3:
        flat[3] = 0
        flat[1] = flat[0] = rows[0]
    return ids


# --------------------------------------------------------------------------------------------- inputs
N_EDGES = 8


def make_state(n, seed, wd=WD, coef=1.0, decoupled=False):
    """float32 p, m, v, g [n] in training ranges (p about 0.1, m about 0.01, v about 1e-4, g about 0.01, a fifth
    of the gradient exactly 0), with the edge elements planted at indices 0 .. N_EDGES - 1 (those below n):
      0  fresh state m = v = 0, g != 0          1  fresh state, g = 0 (g' = wd p only)
      2  g = 0 on a live state (the zero-gradient step)
      3  g' = g coef + wd p within 2^-18 of m (m' cancels)
      4  v subnormal, and so small a p, m that v' stays subnormal
      5  p = 4 - 2^-21 beside an update of 1e-9          6  p = -4 beside a tiny update
      7  v = 0 with m != 0 and g = 0 (the denominator is eps alone under AdamW)"""
    gen = torch.Generator().manual_seed(977 * seed + n)
    rn = lambda: torch.randn(n, generator=gen)
    p, m, v, g = 0.1 * rn(), 0.01 * rn(), 1e-4 * rn().abs(), 0.01 * rn()
    g[torch.rand(n, generator=gen) < 0.2] = 0.0
    l2 = 0.0 if decoupled else wd
    edges = [
        dict(p=0.07, m=0.0, v=0.0, g=0.013),
        dict(p=-0.05, m=0.0, v=0.0, g=0.0),
        dict(p=0.11, m=-0.004, v=2e-4, g=0.0),
        dict(p=0.09, m=0.0123, v=1.5e-4, g=(0.0123 * (1 + 2.0 ** -18) - l2 * f32(0.09)) / coef),
        dict(p=1e-21, m=1e-21, v=1e-40, g=0.0),
        dict(p=4.0 - 2.0 ** -21, m=1e-9, v=1e-4, g=1e-9),
        dict(p=-4.0, m=-3e-10, v=3e-5, g=2e-10),
        dict(p=0.2, m=0.003, v=0.0, g=0.0),
    ]
    assert len(edges) == N_EDGES
    for i, e in enumerate(edges[:n]):
        p[i], m[i], v[i], g[i] = e["p"], e["m"], e["v"], e["g"]
    return p, m, v, g


def ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 where the error is 0; inf where only the bound is), and
    whether any element is NaN."""
    err = (got.detach().double().cpu() - ref.detach().double()).abs()
    bound = bound.detach().double().expand_as(err)
    r = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return (float(r.max()) if r.numel() else 0.0), bool(torch.isnan(err).any())
