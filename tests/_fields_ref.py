"""Inputs, the host reference and the derived error bounds shared by the fields / pair-product tests
(test_fields_ref_host.py, test_gpu_fields.py).

``fields_ref`` is the forward of K1 / K2 (include/fibinet.h, header of csrc/fields.hip) written out in plain
torch on the CPU, float64 by default; ``fields_bwd_ref`` is torch autograd on that function from a given
``dV`` (K4); ``pairs_ref`` the ten element-wise pair products of K5.  No project kernel is involved.  Every
function takes ``dtype``: the float32 evaluation of the same code is the "honest float32 implementation"
the tests hold the bounds against.

Conventions restated from the kernels' documentation:
  * X5 is the mean of the history rows whose id is not 0 (padding), divided by max(1, count).
  * Field 0 (user) is structurally zero: z0 = 0 and only fields 1..5 are stored.
  * An out-of-range likes / views id reads cate row 0 (and that row gets no gradient from the sample);
    an out-of-range item id contributes a zero row; an out-of-range history id is padding.  Each of
    these raises the error flag.  Table row 0 never receives a gradient.
  * Exchanged-row modes: ``table`` is ``(rows, pos)``; entry pos[b][0] is the item's row, pos[b][1 + t]
    history slot t's, -1 = none (a zero row / padding).  bf16 rows are widened exactly.

The backward kernels are handed X = (X3, X5), a and cnt as float32 arrays and recompute fields 1, 2, 4, the
squeeze z and the SENET hidden layer; ``fields_bwd_ref`` therefore takes those same arrays: X3 and X5 are
leaves, a enters as the given value with the sigmoid's derivative a (1 - a) attached to it, cnt divides
dX5.

Error bounds (``fwd_bounds`` / ``bwd_bounds``).  First-order running error analysis of the arithmetic the
kernels document, u = 2^-24: every float32 operation contributes u |result|, a sum of n terms on a path
of K additions K u sum|terms|, and an input's error is carried through by the absolute values of the
partial derivatives.  Each bound is therefore a sum of products K u S with S a float64 sum of absolute
values taken from the reference.  The counts K:
  LS = log2(D) + 1   additions on a path of a D-column sum (3 in the lane's 4 columns, log2(D/4) shuffles)
  sqrtf and the reciprocal: 1 ulp (2 u) each; __expf(x): (2 + 1.173 |x|) ulp, the documented allowance of
  the fast exponential (exp2 of a rounded x log2(e))
  the SENET dot products are sequential: 7 roundings on a 6-term path with its bias, R + 1 on an R-term one
"""
import functools
import math
from types import SimpleNamespace

import torch

from oracle.fibinet_oracle import pair_list

U = 2.0 ** -24
MARGIN = 1e-4            # distance every pre-ReLU value keeps from 0 (LayerNorm output, SENET hidden)
DEAD = -50.0             # bias of the units that are dead on purpose
PAIRS = [(i - 1, j - 1) for i, j in pair_list(6) if i >= 1]        # field 0 is zero: 10 pairs of fields 1..5


# ------------------------------------------------------------------------------------------ forward
def _gather(item_id, item_seq, table, dtype):
    """X3 [B][D], history rows [B][L][D] (zero where not live), live [B][L], bad-id flag."""
    B = item_id.shape[0]
    if isinstance(table, tuple):
        rows, pos = table
        rows, pos = rows.to(dtype), pos.long()
        live = pos >= 0
        g = rows[pos.clamp_min(0)] * live[..., None].to(dtype)
        return g[:, 0], g[:, 1:], live[:, 1:], False
    V, D = table.shape
    t = table.to(dtype)
    ok = (item_id >= 0) & (item_id < V)
    x3 = t[item_id.clamp(0, V - 1)] * ok[:, None].to(dtype)
    if item_seq is None:
        return x3, torch.zeros((B, 0, D), dtype=dtype), torch.zeros((B, 0), dtype=torch.bool), not bool(ok.all())
    inr = (item_seq >= 0) & (item_seq < V)
    live = inr & (item_seq != 0)
    hist = t[item_seq.clamp(0, V - 1)] * live[..., None].to(dtype)
    return x3, hist, live, not (bool(ok.all()) and bool(inr.all()))


def _core(x1, x2, x3, h, x5, ln_g, ln_b, ln_eps, w1, b1, w2, b2, a_given=None):
    """LayerNorm + ReLU, squeeze, excitation, V = X a.  a_given: the value the backward kernel is handed; it
    replaces sigmoid(s) and keeps the derivative a (1 - a) with respect to s."""
    D = h.shape[1]
    mean = h.mean(1, keepdim=True)
    dh = h - mean
    var = (dh * dh).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + ln_eps)
    y = dh * rstd * ln_g + ln_b
    x4 = torch.relu(y)
    X = torch.stack([x1, x2, x3, x4, x5], 1)
    z = torch.cat([torch.zeros_like(h[:, :1]), X.mean(2)], 1)
    q = z @ w1.T + b1
    r = torch.relu(q)
    s = r @ w2.T + b2
    a = torch.sigmoid(s)
    if a_given is not None:
        a = a_given + (s - s.detach()) * (a_given * (1 - a_given))
    V = X * a[:, 1:, None]
    return SimpleNamespace(D=D, h=h, dh=dh, var=var, rstd=rstd, y=y, X=X, X4=x4, z=z, q=q, r=r, s=s, a=a, V=V)


def _cate_rows(cate, ids, n_cate):
    ok = (ids >= 0) & (ids < n_cate)
    return ok, cate[torch.where(ok, ids, torch.zeros_like(ids))]


def fields_ref(item_id, item_seq, likes, views, hmm, ln_g, ln_b, ln_eps, cate, table, w1, b1, w2, b2,
               dtype=torch.float64):
    """The forward.  Returns a namespace with X3, X5, cnt, X4, z, a, V [B][5][D], the error flag ``err`` and
    the intermediates the bounds need (y: pre-ReLU LayerNorm, q: SENET hidden pre-activation, s: logits)."""
    c = lambda t: t.to(dtype)
    x3, hist, live, bad = _gather(item_id, item_seq, table, dtype)
    nnz = live.sum(1).to(dtype)
    cnt = nnz.clamp_min(1.0)
    x5 = hist.sum(1) / cnt[:, None]
    ok1, x1 = _cate_rows(c(cate), likes, cate.shape[0])
    ok2, x2 = _cate_rows(c(cate), views, cate.shape[0])
    o = _core(x1, x2, x3, c(hmm), x5, c(ln_g), c(ln_b), ln_eps, c(w1), c(b1), c(w2), c(b2))
    o.X3, o.X5, o.cnt, o.nnz, o.live = x3, x5, cnt, nnz, live
    o.hist_abs = hist.abs().sum(1)
    o.err = int(bad or not bool(ok1.all()) or not bool(ok2.all()))
    return o


def fwd_bounds(o, ln_g, ln_b, ln_eps, w1, b1, w2, b2, x5_exact=False):
    """Absolute error bounds of a float32 evaluation of the forward (module docstring), from the float64
    reference ``o``: a namespace of e_X5, e_X4, e_z, e_q, e_r, e_a, e_V, and e_dh / rel_r / e_X for the
    backward.  x5_exact: X5 is an input (the backward's recompute)."""
    d = lambda t: t.double()
    ln_g, ln_b, w1, b1, w2, b2 = d(ln_g), d(ln_b), d(w1), d(b1), d(w2), d(b2)
    D, R = o.D, w1.shape[0]
    LS = math.log2(D) + 1
    # X5: nnz - 1 additions in slot order and the division
    e_x5 = torch.zeros_like(o.X5) if x5_exact else o.nnz.clamp_min(1.0)[:, None] * U * o.hist_abs / o.cnt[:, None]
    # mean: LS additions, one division.  dh = h - mean: one rounding, and the mean's error
    e_dh = U * o.dh.abs() + (LS + 1) * U * o.h.abs().mean(1, keepdim=True)
    # var: dh^2 (1), LS additions, / D (1), + eps (1); rstd: sqrtf and reciprocal, 2 u each
    e_var = 2 * (o.dh.abs() * e_dh).mean(1, keepdim=True) + (LS + 3) * U * o.var
    rel_r = e_var / (2 * (o.var + ln_eps)) + 4 * U
    # y = dh rstd g + b: two products and the sum
    t = o.dh * o.rstd * ln_g
    e_y = (o.rstd * ln_g).abs() * e_dh + t.abs() * (rel_r + 2 * U) + U * (t.abs() + ln_b.abs())
    e_x4 = torch.where(o.y > 0, e_y, torch.zeros_like(e_y))
    zero = torch.zeros_like(e_x4)
    e_X = torch.stack([zero, zero, zero, e_x4, e_x5], 1)
    # z: LS additions, one division
    e_z = torch.cat([zero[:, :1], e_X.mean(2) + (LS + 1) * U * o.X.abs().mean(2)], 1)
    # q_j = b1 + sum_f w1 z (sequential, 6 products): 7 roundings on the longest path
    e_q = e_z @ w1.abs().T + 7 * U * (b1.abs() + o.z.abs() @ w1.abs().T)
    e_r = torch.where(o.q > 0, e_q, torch.zeros_like(e_q))
    # s_f = b2 + sum_j w2 r (sequential, R products): R + 1 roundings
    e_s = e_r @ w2.abs().T + (R + 1) * U * (b2.abs() + o.r.abs() @ w2.abs().T)
    # a = 1 / (1 + __expf(-s)): da/ds = a (1 - a); the exponential's relative error enters with the same
    # factor; the addition (u) and the division (2 u)
    a = o.a.detach()
    e_a = a * (1 - a) * (e_s + (2 + 1.173 * o.s.abs()) * 2 * U) + 3 * U * a
    e_V = o.X.abs() * e_a[:, 1:, None] + a[:, 1:, None] * e_X + U * o.V.abs()
    return SimpleNamespace(e_X5=e_x5, e_X4=e_x4, e_y=e_y, e_X=e_X, e_z=e_z, e_q=e_q, e_r=e_r, e_s=e_s, e_a=e_a, e_V=e_V,
                           e_dh=e_dh, rel_r=rel_r)


# ----------------------------------------------------------------------------------------- backward
GRAD_KEYS = ("w1", "b1", "w2", "b2", "ln_g", "ln_b", "cate", "hb")      # the partial row's eight segments


def _segments(D, R, n_cate):
    return [6 * R, R, 6 * R, 6, D, D, n_cate * D, D]


def _table_rows(item_id, item_seq, table):
    """(V or None, pos or None)"""
    if isinstance(table, tuple):
        return None, table[1].long()
    return table.shape[0], None


def _scatter(item_id, item_seq, V, D, gi, gh):
    """Dense table gradient [V][D]: gi[b] to row item_id[b], gh[b] to every live history row; row 0 and
    out-of-range ids get nothing.  Also the number of additions per row."""
    gt = torch.zeros((V, D), dtype=gi.dtype)
    n = torch.zeros((V,), dtype=torch.int64)
    ok = (item_id > 0) & (item_id < V)
    gt.index_add_(0, item_id[ok], gi[ok])
    n += torch.bincount(item_id[ok], minlength=V)
    if item_seq is not None and item_seq.shape[1] > 0:
        live = (item_seq > 0) & (item_seq < V)
        b = torch.arange(item_seq.shape[0])[:, None].expand_as(item_seq)[live]
        gt.index_add_(0, item_seq[live], gh[b])
        n += torch.bincount(item_seq[live], minlength=V)
    return gt, n


def _send_rows(pos, gi, gh):
    """[n_entries][D] rows of the pos modes: entry pos[b][0] <- gi[b], pos[b][1 + t] <- gh[b]; NaN elsewhere."""
    B, L1 = pos.shape
    out = torch.full((B * L1, gi.shape[1]), float("nan"), dtype=gi.dtype)
    src = torch.cat([gi[:, None], gh[:, None].expand(B, L1 - 1, gh.shape[1])], 1)
    live = pos >= 0
    out[pos[live]] = src[live]
    return out


def fields_bwd_ref(item_id, item_seq, likes, views, hmm, ln_g, ln_b, ln_eps, cate, table, w1, b1, w2, b2,
                   X, a, cnt, dV, dtype=torch.float64):
    """Autograd of the forward from dV, with X = [X3, X5], a and cnt as the backward kernels read them.
    Returns dhmm, grads (GRAD_KEYS; hb = the column sum of dhmm), gvec [B][2][D] = (dX3, dX5 / cnt) and
    gtab + adds per row (table mode) or send (pos modes)."""
    c = lambda t: t.detach().to(dtype)
    leaf = lambda t: c(t).requires_grad_()
    hmm_, lg, lb, ct = leaf(hmm), leaf(ln_g), leaf(ln_b), leaf(cate)
    w1_, b1_, w2_, b2_ = leaf(w1), leaf(b1), leaf(w2), leaf(b2)
    x3, x5 = leaf(X[:, 0]), leaf(X[:, 1])
    n_cate = cate.shape[0]
    ok1, x1 = _cate_rows(ct, likes, n_cate)
    ok2, x2 = _cate_rows(ct, views, n_cate)
    x1 = torch.where(ok1[:, None], x1, x1.detach())         # fields_bwd_cate skips a bad id's row
    x2 = torch.where(ok2[:, None], x2, x2.detach())
    o = _core(x1, x2, x3, hmm_, x5, lg, lb, ln_eps, w1_, b1_, w2_, b2_, a_given=c(a))
    loss = (o.V * c(dV)).sum()
    g = torch.autograd.grad(loss, [w1_, b1_, w2_, b2_, lg, lb, ct, hmm_, x3, x5])
    grads = dict(zip(GRAD_KEYS[:7], g[:7]))
    dhmm, dx3, dx5 = g[7], g[8], g[9]
    grads["hb"] = dhmm.sum(0)
    gh = dx5 / c(cnt)[:, None]
    out = SimpleNamespace(dhmm=dhmm, grads=grads, gvec=torch.stack([dx3, gh], 1))
    V, pos = _table_rows(item_id, item_seq, table)
    if pos is None:
        out.gtab, out.adds = _scatter(item_id, item_seq, V, hmm.shape[1], dx3, gh)
    else:
        out.send = _send_rows(pos, dx3, gh)
    return out


def bwd_launch_shape(B, D):
    """(blocks, samples per wave, iterations of the grid-stride loop) of the fields backward."""
    spw = 64 // (D // 4)
    blocks = max(1, min(512, (-(-B // spw) + 3) // 4))
    return blocks, spw, -(-B // (blocks * 4 * spw))


def bwd_bounds(item_id, item_seq, likes, views, hmm, ln_g, ln_b, ln_eps, cate, table, w1, b1, w2, b2,
               X, a, cnt, dV):
    """The backward written out in closed form in float64, as the kernel documents it, with the error
    bound of a float32 evaluation beside every output (module docstring).  Returns (values, bounds):
    namespaces with dhmm, gvec, grads, and gtab or send.  The bounds hold two sets for the parameter
    gradients: ``grads`` for the ones that went through the partial-row reduce kernel (64 streams, folded
    in order) and ``grads_part`` for a float64 sum of the partial rows."""
    d = lambda t: t.detach().double()
    ln_g, ln_b, w1, b1, w2, b2, cate, dv, a, cnt = (d(t) for t in (ln_g, ln_b, w1, b1, w2, b2, cate, dV, a, cnt))
    B, D = hmm.shape
    R, n_cate = w1.shape[0], cate.shape[0]
    LS = math.log2(D) + 1
    ok1, x1 = _cate_rows(cate, likes, n_cate)
    ok2, x2 = _cate_rows(cate, views, n_cate)
    o = _core(x1, x2, d(X[:, 0]), d(hmm), d(X[:, 1]), ln_g, ln_b, ln_eps, w1, b1, w2, b2)
    o.X5, o.nnz, o.hist_abs, o.cnt = o.X[:, 4], None, None, None
    f = fwd_bounds(o, ln_g, ln_b, ln_eps, w1, b1, w2, b2, x5_exact=True)
    a5 = a[:, 1:]
    # da_f = sum_d dv x: one product, LS additions
    dvx = dv * o.X
    e_da = (dv.abs() * f.e_X).sum(2) + (LS + 1) * U * dvx.abs().sum(2)
    # ds = da (1 - a) a: the subtraction and two products
    ds5 = dvx.sum(2) * (1 - a5) * a5
    e_ds5 = e_da * (1 - a5) * a5 + 3 * U * ds5.abs()
    z1 = torch.zeros_like(ds5[:, :1])
    ds, e_ds = torch.cat([z1, ds5], 1), torch.cat([z1, e_ds5], 1)
    # dr_j = sum_f w2[f][j] ds_f (6 sequential terms); dq = dr where q > 0
    gate = (o.q > 0).double()
    dq = (ds @ w2) * gate
    e_dq = (e_ds @ w2.abs() + 6 * U * (ds.abs() @ w2.abs())) * gate
    # dz_f = sum_j w1[j][f] dq_j (R sequential terms added to 0)
    dz = dq @ w1
    e_dz = e_dq @ w1.abs() + (R + 1) * U * (dq.abs() @ w1.abs())
    # dx = dv a + dz / D: product, division, sum
    dva, dzD = dv * a5[:, :, None], dz[:, 1:, None] / D
    dx = dva + dzD
    e_dx = e_dz[:, 1:, None] / D + 2 * U * (dva.abs() + dzD.abs())
    gh = dx[:, 4] / cnt[:, None]
    e_gh = e_dx[:, 4] / cnt[:, None] + U * gh.abs()
    val = SimpleNamespace(gvec=torch.stack([dx[:, 2], gh], 1))
    bnd = SimpleNamespace(gvec=torch.stack([e_dx[:, 2], e_gh], 1))
    # ---- per-sample terms of the parameter gradients
    t, e = {}, {}
    t["w1"] = dq[:, :, None] * o.z[:, None, :]
    e["w1"] = e_dq[:, :, None] * o.z.abs()[:, None, :] + dq.abs()[:, :, None] * f.e_z[:, None, :] + U * t["w1"].abs()
    t["b1"], e["b1"] = dq, e_dq
    t["w2"] = ds[:, :, None] * o.r[:, None, :]
    e["w2"] = e_ds[:, :, None] * o.r.abs()[:, None, :] + ds.abs()[:, :, None] * f.e_r[:, None, :] + U * t["w2"].abs()
    t["b2"], e["b2"] = ds, e_ds
    live4 = (o.X4 > 0).double()
    gl, e_gl = dx[:, 3] * live4, e_dx[:, 3] * live4
    xh = o.dh * o.rstd
    e_xh = o.rstd * f.e_dh + xh.abs() * (f.rel_r + U)
    t["ln_g"] = gl * xh
    e["ln_g"] = e_gl * xh.abs() + gl.abs() * e_xh + U * t["ln_g"].abs()
    t["ln_b"], e["ln_b"] = gl, e_gl
    # ---- dhmm = rstd (gx - m1 - xh m2), gx = gl g, m1 = mean gx, m2 = mean gx xh
    gx = gl * ln_g
    e_gx = e_gl * ln_g.abs() + U * gx.abs()
    m1 = gx.mean(1, keepdim=True)
    e_m1 = e_gx.mean(1, keepdim=True) + (LS + 1) * U * gx.abs().mean(1, keepdim=True)
    m2 = (gx * xh).mean(1, keepdim=True)
    e_m2 = (e_gx * xh.abs() + gx.abs() * e_xh).mean(1, keepdim=True) + (LS + 2) * U * (gx * xh).abs().mean(1, keepdim=True)
    inner = gx - m1 - xh * m2
    e_in = e_gx + e_m1 + e_xh * m2.abs() + xh.abs() * e_m2 + 3 * U * (gx.abs() + m1.abs() + (xh * m2).abs())
    val.dhmm = o.rstd * inner
    bnd.dhmm = o.rstd * e_in + val.dhmm.abs() * (f.rel_r + U)
    t["hb"], e["hb"] = val.dhmm, bnd.dhmm
    # ---- sums over the batch.  A lane adds its samples in turn (iters), the wave's groups fold by
    # shuffles (log2 spw), the block adds its 4 wave slices (2); the reduce kernel then adds
    # ceil(blocks / 64) rows per stream and folds the streams that hold any (<= 64) in order.
    blocks, spw, iters = bwd_launch_shape(B, D)
    k_acc = iters + math.log2(spw) + 2
    k_red = -(-blocks // 64) + min(64, blocks)
    val.grads, bnd.grads, bnd.grads_part = {}, {}, {}
    for k in t:
        val.grads[k] = t[k].sum(0)
        bnd.grads_part[k] = e[k].sum(0) + k_acc * U * t[k].abs().sum(0)
        bnd.grads[k] = bnd.grads_part[k] + k_red * U * t[k].abs().sum(0)
    # cate rows: the wave's groups take turns on its LDS slice, likes and views both: 2 iters spw additions
    tc, ec, ac = (torch.zeros((n_cate, D), dtype=torch.float64) for _ in range(3))
    for ok, ids, fld in ((ok1, likes, 0), (ok2, views, 1)):
        tc.index_add_(0, ids[ok], dx[:, fld][ok])
        ec.index_add_(0, ids[ok], e_dx[:, fld][ok])
        ac.index_add_(0, ids[ok], dx[:, fld][ok].abs())
    val.grads["cate"] = tc
    bnd.grads_part["cate"] = ec + (2 * iters * spw + 2) * U * ac
    bnd.grads["cate"] = bnd.grads_part["cate"] + k_red * U * ac
    # ---- the table gradient: n atomic additions in any order, or the routed rows
    V, pos = _table_rows(item_id, item_seq, table)
    if pos is None:
        val.gtab, n = _scatter(item_id, item_seq, V, D, dx[:, 2], gh)
        eg, _ = _scatter(item_id, item_seq, V, D, e_dx[:, 2], e_gh)
        ag, _ = _scatter(item_id, item_seq, V, D, dx[:, 2].abs(), gh.abs())
        bnd.gtab = eg + n[:, None].double() * U * ag
        val.adds = n
    else:
        val.send = _send_rows(pos, dx[:, 2], gh)
        bnd.send = _send_rows(pos, e_dx[:, 2], e_gh)
    return val, bnd


def half_ulp_bf16(ref):
    """Half a bf16 ulp at |ref| (8 significand bits)."""
    _, ex = torch.frexp(ref.double().abs().clamp_min(2.0 ** -126))
    return torch.exp2((ex - 9).double())


# -------------------------------------------------------------------------------------------- pairs
def pairs_ref(V, Uf, mode, dtype=torch.float64):
    """[B][10][D]: mode 0 ("all") V_i U_j, mode 1 ("each") U_i V_j over the pairs i < j of fields 1..5."""
    V, Uf = V.to(dtype), Uf.to(dtype)
    return torch.stack([V[:, i] * Uf[:, j] if mode == 0 else Uf[:, i] * V[:, j] for i, j in PAIRS], 1)


def pairs_bwd_ref(dc, V, Uf, mode, dtype=torch.float64):
    """Autograd of c = [V | pairs] from dc [B][15][D]: (dV, dU, sum|terms| of dV, of dU, terms of dV, of dU)."""
    Vl, Ul = V.detach().to(dtype).requires_grad_(), Uf.detach().to(dtype).requires_grad_()
    dc = dc.to(dtype)
    c = torch.cat([Vl, pairs_ref(Vl, Ul, mode, dtype)], 1)
    dVv, dUu = torch.autograd.grad((c * dc).sum(), [Vl, Ul])
    Va, Ua, da = V.double().abs(), Uf.double().abs(), dc.double().abs()
    sV, sU = da[:, :5].clone(), torch.zeros_like(Va)
    nV, nU = torch.ones(5), torch.zeros(5)
    for k, (i, j) in enumerate(PAIRS):
        vi, ui = (i, j) if mode == 0 else (j, i)             # the field whose V / whose U enters pair k
        sV[:, vi] += da[:, 5 + k] * Ua[:, ui]
        sU[:, ui] += da[:, 5 + k] * Va[:, vi]
        nV[vi] += 1
        nU[ui] += 1
    return dVv, dUu, sV, sU, nV, nU


# ---------------------------------------------------------------------------------- input generator
def ids_family(family, g, shape, V):
    """ids in [1, V): uniform, or Zipf(1.2) ranks mapped through a fixed permutation."""
    if family == "zipf" and math.prod(shape) > 0:
        w = 1.0 / torch.arange(1, V, dtype=torch.float64) ** 1.2
        rank = torch.multinomial(w, math.prod(shape), replacement=True, generator=g)
        perm = torch.randperm(V - 1, generator=g) + 1
        return perm[rank].view(shape)
    return torch.randint(1, V, shape, generator=g)


VOCAB = {"uniform": 5000, "collide": 61, "zipf": 5000}


@functools.lru_cache(maxsize=4)
def make_case(D, B, L, R=3, n_cate=11, family="uniform", mode="table", seed=0):
    """One test case on the CPU (treat as read-only): ids, float32 inputs, dV, and for the pos modes the
    shuffled row buffer.  Samples 0 / 1 / 2 (those that exist): the item id also in its own history; all
    padding; a single live slot mid-history.  Sample 3: item id 0.  Column 1 of LayerNorm and (R > 1) SENET
    hidden unit 0 are dead on purpose (bias -50).  hmm rows that leave a pre-ReLU value within MARGIN of zero
    (float64) are drawn again, deterministically."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * D + 13 * B + 31 * L + R)
    V = VOCAB[family]
    c = SimpleNamespace(D=D, B=B, L=L, R=R, n_cate=n_cate, V=V, family=family, mode=mode, ln_eps=1e-5)
    c.item_id = ids_family(family, g, (B,), V)
    seq = ids_family(family, g, (B, L), V)
    seq[torch.rand((B, L), generator=g) < 0.5] = 0
    if L > 0:
        seq[0, L // 2] = c.item_id[0]
        if B > 1:
            seq[1] = 0
        if B > 2:
            seq[2] = 0
            seq[2, L // 2] = 11
    if B > 3:
        c.item_id[3] = 0
    c.item_seq = seq if L > 0 else None
    c.likes = torch.randint(0, n_cate, (B,), generator=g)
    c.views = torch.randint(0, n_cate, (B,), generator=g)
    rn = lambda *s: torch.randn(s, generator=g)
    c.table, c.cate = rn(V, D), rn(n_cate, D)
    c.ln_g, c.ln_b = 1.0 + 0.3 * rn(D), 0.3 * rn(D)
    c.ln_b[1] = DEAD
    c.w1, c.b1 = rn(R, 6), 0.5 * rn(R)
    c.w2, c.b2 = rn(6, R) / math.sqrt(R), 0.5 * rn(6)
    c.b1[R - 1] = c.b1[R - 1].abs() + 1.5          # one unit that is mostly live
    if R > 1:
        c.b1[0] = DEAD
    c.dV = rn(B, 5, D)
    c.hmm = rn(B, D)
    c.hmm[4::5] *= 0.05                            # rows of small variance: ln_eps is 0.4 % of var + eps there
    c.rows = c.pos = None
    c.tab = c.table
    if mode != "table":
        ids = torch.cat([c.item_id[:, None], seq], 1)
        perm = torch.randperm(B * (L + 1), generator=g).view(B, L + 1).int()
        c.pos = torch.where(ids > 0, perm, torch.full_like(perm, -1)).contiguous()
        rows = torch.zeros(B * (L + 1), D)
        live = c.pos >= 0
        rows[c.pos[live].long()] = c.table[ids[live]]
        c.rows = rows.bfloat16() if mode == "rows_bf16" else rows
        c.tab = (c.rows, c.pos)
    for _ in range(50):
        o = fields_ref(*fwd_args(c))
        near = ((o.y.abs() < MARGIN).any(1) | (o.q.abs() < MARGIN).any(1)).nonzero().flatten()
        if near.numel() == 0:
            break
        c.hmm[near] = torch.randn((near.numel(), D), generator=g) * torch.where(near % 5 == 4, 0.05, 1.0)[:, None]
    else:
        raise AssertionError("make_case: margins not met after 50 draws")
    return c


def fwd_args(c):
    return (c.item_id, c.item_seq, c.likes, c.views, c.hmm, c.ln_g, c.ln_b, c.ln_eps, c.cate, c.tab,
            c.w1, c.b1, c.w2, c.b2)


def b_sizes(D):
    """One live group; a second block with one live group; a ragged wave mid-grid."""
    spb = 1024 // D
    return [1, spb + 1, 3 * spb + 64 // (D // 4) // 2 + 1]


def shape_matrix():
    """The forward / backward cases of test_gpu_fields.py: dicts of make_case arguments (+ hch / cmp / hot)."""
    m = []
    add = lambda **k: m.append(k)
    for D in (16, 32, 64, 128, 256):                          # every instantiation at three batch shapes
        for B in b_sizes(D):
            add(D=D, B=B, L=20)
    for D, B in ((256, 2051), (16, 32771), (256, 4099), (16, 65539)):   # the grid-stride loops iterate
        add(D=D, B=B, L=2)
    for D in (16, 128):
        for L in (0, 1, 7, 23, 32):
            add(D=D, B=b_sizes(D)[2], L=L)
        add(D=D, B=b_sizes(D)[2], L=20, n_cate=3)
        for fam in ("collide", "zipf"):
            add(D=D, B=300, L=20, family=fam)
    for D in (16, 256):
        for R in (1, 2, 4, 8):
            add(D=D, B=b_sizes(D)[1], L=20, R=R)
    for D in (16, 128, 256):
        for mode in ("rows_f32", "rows_bf16"):
            add(D=D, B=b_sizes(D)[2], L=20, mode=mode)
    for hch in ("5", "10", "20"):
        add(D=128, B=41, L=23, hch=hch, seed=1)
    add(D=128, B=41, L=23, cmp=True, seed=1)
    add(D=128, B=300, L=20, family="zipf", hot=True, seed=1)
    return m


# the cases of test_fields_bwd_img_and_slot and of test_bad_id_raises_the_flag (before the bad id goes in)
IMG_SLOT_CASES = [dict(D=D, B=b_sizes(D)[2], L=20, seed=2) for D in (128, 32)]
BAD_ID_CASE = dict(D=16, B=65, L=23, seed=3)

CASE_KEYS = ("D", "B", "L", "R", "n_cate", "family", "mode", "seed")


def case_of(k):
    return make_case(**{x: k[x] for x in CASE_KEYS if x in k})


def case_id(k):
    return "-".join(f"{x}{k[x]}" if not isinstance(k[x], bool) else x for x in k)
