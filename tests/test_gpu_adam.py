"""The clip-norm and Adam kernels (csrc/optim.hip) against float64 torch Adam, one launch at a time (pytest -m gpu).

Every check is step-locked: the kernel's inputs (p, m, v, the gradient, the claims, the norm slots) are built on
the CPU, one launch runs, and the outputs are compared with tests/_adam_ref.py -- adam_step_ref of those very
inputs at the constants step_consts read off torch's OneCycleLR and Adam (never the library's own schedule
table, which the kernel is handed and whose float32 rounding the bound counts), under step_bounds / clip_bounds,
the first-order error bounds derived there.  Error cannot accumulate, so there is no trajectory tolerance, and
no element is left out of any comparison.  Everything that is not arithmetic -- map, slot_row, pend, last, the
ring, the counters, the norm slots, canaries behind every buffer, rows a kernel must not touch -- is compared
bitwise.  Every value check prints "[adam-ratio] <name> kernel=<worst error / bound> f32ref=<the same for the
float32 CPU evaluation of the step in adam_elem's operation order>"; the worst of each name goes to
adam_kernels.json in the parity tests' output directory ($FBN_PARITY_OUT, or their common default: _out_dir of
tests/test_gpu_c4.py).  tests/test_adam_ref_host.py holds the reference
to torch, the float32 evaluation to the bounds, and shows that the bounds reject a step that reads the next
schedule row, joins wd p before the clip multiply, loses eps, swaps b2 and 1 - b2 or skips the n % 4 tail.

Worst ratios over the whole file on an MI355X (kernel / float32 reference), as m, v, p:
  fbn_adam_dense (coef ptr, NULL, slots)   0.79 / 0.87, 0.71 / 0.71, 0.98 / 0.98
  fbn_adam_table modes 0, 1, 2             0.82 / 0.87, 0.72 / 0.72, 0.99 / 0.99
  fbn_adam_touched                         0.82 / 0.82, 0.67 / 0.67, 0.97 / 0.97
  fbn_adam_commit, rows stepped now        0.75 / 0.75, 0.65 / 0.65, 0.89 / 0.89
  fbn_adam_step_tail, rows stepped now     0.74 / 0.74, 0.60 / 0.60, 0.87 / 0.87
  fbn_adam_step_tail, the dense part       0.86 / 0.88, 0.72 / 0.72, 0.99 / 0.99
  fbn_adam_flush after either              0.81 / 0.83, 0.71 / 0.71, 0.96 / 0.96
  six locked steps, dense                  0.74 / 0.79, 0.64 / 0.64, 0.94 / 0.94
  six locked steps, table                  0.75 / 0.86, 0.66 / 0.66, 0.98 / 0.98
  norm 0.15, coefficient 0.23, fbn_sumsq 0.30, fbn_unpack_sumsq 0.20, fbn_sumsq_sparse 0.02,
  fbn_sumsq_sparse_norms 0.01 (fx 0.002)
m and v sit near 0.7 to 0.8 because a handful of roundings hit their worst case somewhere among 10^5 elements; p sits
at 0.99 because its bound is dominated by u |p'|, half an ulp of the result, which an element just under a power of
two (the planted |p| = 4 - 2^-21, and others by chance) meets exactly.  The kernel is never above the float32 host
evaluation by more than a few percent: the fused multiply-adds save roundings that v_sqrt_f32 / v_rcp_f32 spend.

What covers what:
  fbn_sumsq                          n 1 .. 512*256*4 + 7, the n_rows form, slots added to      test_sumsq
  fbn_clip_coef, fbn_adam_dense's in-kernel clip   norm 0, under, over, 1e3 over, past float32   test_clip_coef
  fbn_sumsq_sparse, fbn_sumsq_sparse_norms (+ fx, dense)   D 16 / 128, both layouts, FULL        test_sumsq_sparse*
  fbn_pack_extras, fbn_unpack_extras, fbn_unpack_sumsq                                           test_pack_unpack
  fbn_sum_slices                     ns 1 / 3 / 8, f32 / f64                                     test_sum_slices
  fbn_adam_dense                     n 1 .. 3*1024*4 + 5, Adam / AdamW, coef ptr / NULL / slots   test_adam_dense*
  fbn_adam_table (0, 1, 2), fbn_adam_touched   D 16 .. 256, nrows 1 / 37 / 1500, every layout    test_adam_table
  fbn_adam_commit, fbn_adam_step_tail, fbn_step_end, fbn_adam_flush   D 16 / 128                 test_step_tail*
  six steps on the device counter    sumsq + clip_coef + dense + table mode 0 + step_end         test_six_locked_steps
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from ctr_recommendation_amd import _lib, schedule
from ctr_recommendation_amd._lib import call, ptr
from tests import _adam_ref as ar
from tests.test_gpu_c4 import _out_dir          # $FBN_PARITY_OUT or the parity tests' default directory

pytestmark = pytest.mark.gpu
TOTAL = 20
STEP = 7                                  # the device counter of the single-step tests: optimizer step 8 of 20
BETA2, EPS, WD = ar.BETA2, ar.EPS, ar.WD
FBN_OK, FBN_ERR_ARG = 0, 1
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_file():
    yield
    with open(os.path.join(_out_dir(), "adam_kernels.json"), "w") as f:
        json.dump({k: {"kernel": v[0], "f32ref": v[1]} for k, v in sorted(RATIOS.items())}, f, indent=1)


# ---------------------------------------------------------------------------------------------- helpers
_KS, _TAB = {}, {}


def consts(decoupled):
    if decoupled not in _KS:
        _KS[decoupled] = ar.step_consts(TOTAL, 1e-3, BETA2, WD, decoupled)
    return _KS[decoupled]


def table(dev, decoupled):
    """The library's own float32 schedule table on the device (what the trainer uploads)."""
    if decoupled not in _TAB:
        tab, _ = schedule.adam_table(TOTAL, 1e-3, BETA2, decoupled_wd=WD if decoupled else 0.0)
        _TAB[decoupled] = torch.from_numpy(tab).to(dev)
    return _TAB[decoupled]


def wd_arg(decoupled):
    return 0.0 if decoupled else WD       # as the trainer: L2 inside the gradient, or dmul in the table


def _record(name, worst, w32):
    old = RATIOS.get(name, (0.0, 0.0))
    RATIOS[name] = (max(old[0], worst), max(old[1], w32))
    print(f"[adam-ratio] {name} kernel={worst:.4f} f32ref={w32:.4f}")


def _check(name, got, ref, bound, ref32):
    worst, nan = ar.ratio(got, ref, bound)
    assert not nan, f"{name}: NaN in the output"
    w32, _ = ar.ratio(ref32, ref, bound)
    _record(name, worst, w32)
    if worst > 1.0:
        err = (got.detach().double().cpu() - ref).abs() / bound.expand_as(ref)
        i = int(torch.nan_to_num(err, 0.0).flatten().argmax())
        raise AssertionError(f"{name}: error / bound = {worst:.3f} at flat index {i}: got {got.flatten()[i].item()!r}, "
                             f"reference {ref.flatten()[i].item()!r}, bound {bound.expand_as(ref).flatten()[i].item():.3e}")
    assert not w32 > 1.0, f"{name}: the float32 reference exceeds the bound ({w32:.3f}): the bound is too tight"


def _check_step(name, before, g64, g_err, coef, step, decoupled, after):
    """after = (p, m, v) of a kernel that applied optimizer step ``step + 1`` to before = (p, m, v) (CPU float32)
    with the gradient g64 (float64, error bound g_err before the clip multiply) and the float coef."""
    k = consts(decoupled)[step]
    p, m, v = before
    ref = ar.adam_step_ref(p, m, v, g64, coef, k, WD, BETA2, EPS, decoupled)
    e_m, e_v, e_p = ar.step_bounds(p, m, v, g64, coef, k, WD, BETA2, EPS, decoupled, g_err)
    r32 = ar.adam_elem_f32(p, m, v, g64.float(), coef, ar.table_row_f32(k, WD, decoupled), WD, BETA2, EPS, decoupled)
    for nm, got, r, e, r3 in (("m", after[1], ref[1], e_m, r32[1]), ("v", after[2], ref[2], e_v, r32[2]),
                              ("p", after[0], ref[0], e_p, r32[0])):
        _check(f"{name}.{nm}", got.cpu(), r, e, r3)


def _bits(t):
    return t.detach().cpu().contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(name, got, want):
    assert torch.equal(_bits(got), _bits(want)), f"{name}: not bitwise unchanged / equal"


def _i32(x, dev):
    return torch.tensor([x], dtype=torch.int32, device=dev)


def _f32(x, dev):
    return torch.tensor([x], dtype=torch.float32, device=dev)


def _slots_for(total, seed=0):
    """64 float64 slot values with the given sum (up to float64 rounding), none of them zero."""
    w = np.random.RandomState(seed).uniform(0.5, 1.5, ar.FBN_SUMSQ_SLOTS)
    return total * w / w.sum()


# ---------------------------------------------------------------------------------- norm and coefficient
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 512 * 256 * 4 + 7])
def test_sumsq(hip_device, n):
    dev, st = hip_device, _lib.stream_handle(hip_device)
    x = 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(n))
    pre = torch.from_numpy(_slots_for(17.0, 1))
    out, xd = pre.to(dev), x.to(dev)
    call("fbn_sumsq", ptr(xd), n, None, 0, ptr(out), st)
    got = out.cpu()
    want = float((x.double() ** 2).sum())
    bound = ar.sumsq_bound(want, n, 17.0)
    err = abs(float((got - pre).sum()) - want)
    _record("sumsq", err / bound, 0.0)
    assert err <= bound, (err, bound)
    assert bool((got >= pre).all()), "a slot was overwritten, not added to"
    if n <= 1023:                                     # one block holds every element: the other slots get + 0.0
        _same("slots 1..63", got[1:], pre[1:])
    # ---- the n_rows / row_len form: the limit n_rows * row_len < n; what lies past it is 1e30
    row_len = 5 if n > 5 else 1
    rows = (n - 1) // row_len
    lim = rows * row_len
    y = x.clone()
    y[lim:] = 1e30
    out, yd, rows_d = pre.to(dev), y.to(dev), _i32(rows, dev)      # (every operand held until the launch is in)
    call("fbn_sumsq", ptr(yd), n, ptr(rows_d), row_len, ptr(out), st)
    want = float((x[:lim].double() ** 2).sum())
    err = abs(float((out.cpu() - pre).sum()) - want)
    bound = ar.sumsq_bound(want, lim, 17.0)
    assert err <= bound, ("n_rows form", err, bound)


CLIP_CASES = {"zero": 0.0, "under": (1.0 - 1e-5) ** 2, "over": (1.0 + 1e-5) ** 2, "far_over": 1e6, "inf": 1e39}


@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clip_coef(hip_device, case):
    """fbn_clip_coef and the in-kernel form of fbn_adam_dense on the same slots: both against clip_ref, bitwise
    equal to each other, and the dense step taken with that coefficient."""
    dev, st = hip_device, _lib.stream_handle(hip_device)
    max_norm = 1.0
    parts = _slots_for(CLIP_CASES[case], 2)
    slots = torch.from_numpy(parts).to(dev)
    coef, norm = _f32(float("nan"), dev), _f32(float("nan"), dev)
    call("fbn_clip_coef", ptr(slots), max_norm, ptr(coef), ptr(norm), st)
    n = 37
    p, m, v, g = ar.make_state(n, 3)
    d = [t.to(dev) for t in (p, m, v, g)]
    coef2, norm2, step = _f32(float("nan"), dev), _f32(float("nan"), dev), _i32(STEP, dev)
    call("fbn_adam_dense", ptr(d[0]), ptr(d[3]), ptr(d[1]), ptr(d[2]), n, None, ptr(table(dev, False)),
         ptr(step), WD, BETA2, EPS, ptr(slots), max_norm, ptr(coef2), ptr(norm2), st)
    torch.cuda.synchronize()
    _same("coef (in-kernel vs fbn_clip_coef)", coef2, coef)
    _same("norm (in-kernel vs fbn_clip_coef)", norm2, norm)
    _same("slots", slots, torch.from_numpy(parts))
    rn, rc = ar.clip_ref(parts, max_norm)
    en, ec = ar.clip_bounds(parts, max_norm, sq_roundings=0)
    c, nm = float(coef), float(norm)
    if case == "inf":
        assert math.isinf(nm) and c == 0.0
    elif case == "zero":
        assert nm == 0.0 and c == 1.0
    else:
        _record("clip.norm", abs(nm - rn) / en, 0.0)
        _record("clip.coef", abs(c - rc) / ec if c != rc else 0.0, 0.0)
        assert abs(nm - rn) <= en and abs(c - rc) <= ec, (nm, rn, en, c, rc, ec)
        assert (c == 1.0) == (case == "under") and c <= 1.0
    _check_step("dense.slots", (p, m, v), g.double(), None, c, STEP, False, d[:3])


def _claims(layout, D, full, bf16, B=8, L=20, V=400, seed=0, step=STEP, pool=None):
    ids = ar.entry_ids(B, L, V, seed=seed + 3, pool=pool).reshape(-1) if V > 1 else np.zeros(B * (L + 1), dtype=np.int64)
    vec = layout == "vec"
    return ar.make_claims(ids, V, D, seed=seed + D + 1, B=B if vec else None, L=L if vec else None, full=full, bf16=bf16,
                          step=step)


class _DevClaims:
    def __init__(self, c, dev):
        self.map, self.slot_row, self.extra = c.map.to(dev), c.slot_row.to(dev), c.extra.to(dev)
        self.gvec = (c.gvec_store if c.bf16 else c.gvec).to(dev)
        self.rs = c.rs.to(dev)

    def src(self, c):
        """gvec, extra, slot_row, Lp1"""
        return ptr(self.gvec), ptr(self.extra), ptr(self.slot_row), c.lp1


@pytest.mark.parametrize("layout,full,bf16", [("vec", False, False), ("vec", True, False), ("rows", False, False),
                                              ("rows", True, True)])
@pytest.mark.parametrize("D", [16, 128])
def test_sumsq_sparse(hip_device, D, layout, full, bf16):
    """The float64 sum over the claimed rows.  Per element: the float32 sum gvec + extra of a flagged row (2 u on
    its square), the float32 square (u); the float64 additions."""
    dev, st = hip_device, _lib.stream_handle(hip_device)
    c = _claims(layout, D, full, bf16, B=33)
    d = _DevClaims(c, dev)
    pre = torch.from_numpy(_slots_for(3.0, 4))
    out = pre.to(dev)
    call("fbn_sumsq_sparse", *d.src(c), c.n, D, ptr(out), st)
    want = float((c.grad ** 2).sum())
    bound = ar.sumsq_bound(want, c.n * D, 3.0, sq_roundings=3)
    err = abs(float((out.cpu() - pre).sum()) - want)
    _record("sumsq_sparse", err / bound, 0.0)
    assert err <= bound, (err, bound, want)
    _same("extra", d.extra, c.extra)
    _same("slot_row", d.slot_row, c.slot_row)


@pytest.mark.parametrize("dense_n", [0, 1028])
@pytest.mark.parametrize("fx", [False, True])
@pytest.mark.parametrize("D", [16, 128])
def test_sumsq_sparse_norms(hip_device, D, fx, dense_n):
    """gnorm [B][2] from float64; unflagged claimers add their vector's norm, flagged ones gvec + extra -- or,
    with the fixed-point accumulator, the row round(x 2^40) 2^-40 that the kernel writes to extra, zeroing acc."""
    dev, st = hip_device, _lib.stream_handle(hip_device)
    c = _claims("vec", D, fx, False, B=33)
    d = _DevClaims(c, dev)
    gnorm = (c.gvec.double() ** 2).sum(2)
    grad = c.grad.clone()
    acc_d = None
    if fx:
        acc = torch.full((c.n, D), 77, dtype=torch.int64)
        exp_extra = torch.full((c.n, D), float("nan"))
        for i in np.nonzero(c.flagged)[0]:
            a = torch.round(c.grad_all[i] * 2.0 ** 40).to(torch.int64)
            acc[c.claimer[i]] = a
            exp_extra[c.claimer[i]] = (a.double() * 2.0 ** -40).float()
            grad[i] = exp_extra[c.claimer[i]].double()
        d.extra = torch.full((c.n, D), float("nan"), device=dev)   # the kernel writes the flagged claimers' rows
        acc_d = acc.to(dev)
    dense = 0.2 * torch.randn(dense_n, generator=torch.Generator().manual_seed(9)) if dense_n else None
    dense_d = dense.to(dev) if dense_n else None
    pre = torch.from_numpy(_slots_for(3.0, 4))
    out, gnorm_d = pre.to(dev), gnorm.to(dev)
    call("fbn_sumsq_sparse_norms", ptr(gnorm_d), *d.src(c), c.n, D, ptr(out), ptr(acc_d), ptr(dense_d), dense_n, st)
    torch.cuda.synchronize()
    unfl = torch.from_numpy(~c.flagged)
    want = float(gnorm.view(-1)[torch.from_numpy(c.vec_of[c.claimer])][unfl].sum()) + float((grad[~unfl] ** 2).sum())
    want_d = float((dense.double() ** 2).sum()) if dense_n else 0.0
    bound = ar.sumsq_bound(want + want_d, c.n * D + dense_n, 3.0, sq_roundings=3)
    err = abs(float((out.cpu() - pre).sum()) - want - want_d)
    _record("sumsq_sparse_norms" + (".fx" if fx else ""), err / bound, 0.0)
    assert err <= bound, (err, bound, want, want_d)
    if fx:
        fl = torch.from_numpy(c.claimer[c.flagged])
        _same("extra of the flagged claimers", d.extra[fl], exp_extra[fl])
        assert bool(torch.isnan(d.extra.cpu()[torch.from_numpy(c.slot_row.numpy() == -1)]).all())
        want_acc = acc.clone()
        want_acc[fl] = 0
        _same("acc", acc_d, want_acc)
    else:
        _same("extra", d.extra, c.extra)


def test_sumsq_sparse_norms_argument_errors(hip_device):
    dev, st, L = hip_device, _lib.stream_handle(hip_device), _lib.lib()
    c = _claims("vec", 16, False, False)
    d = _DevClaims(c, dev)
    gnorm = (c.gvec.double() ** 2).sum(2).to(dev)
    pre = torch.from_numpy(_slots_for(3.0, 4))
    out = pre.to(dev)
    dense = torch.ones(16, device=dev)
    f = lambda lp1, dn, nd: L.fbn_sumsq_sparse_norms(ptr(gnorm), ptr(d.gvec), ptr(d.extra), ptr(d.slot_row), lp1, c.n, 16,
                                                     ptr(out), None, dn, nd, st)
    got = {"n_dense % 4": f(c.lp1, ptr(dense), 5), "dense NULL, n_dense 4": f(c.lp1, None, 4),
           "dense misaligned": f(c.lp1, ptr(dense) + 4, 8), "n_dense < 0": f(c.lp1, ptr(dense), -4), "Lp1 = 1": f(1, None, 0)}
    assert got == {k: FBN_ERR_ARG for k in got}
    assert L.fbn_sumsq_sparse_norms(ptr(gnorm), ptr(d.gvec), ptr(d.extra), ptr(d.slot_row), c.lp1, 0, 16, ptr(out), None,
                                    None, 0, st) == FBN_OK
    torch.cuda.synchronize()
    _same("slots", out, pre)


@pytest.mark.parametrize("n", [0, 5, 4099])
def test_pack_unpack(hip_device, n):
    dev, st = hip_device, _lib.stream_handle(hip_device)
    loss = _f32(0.6931471, dev)
    parts = _slots_for(0.37, 5)
    slots = torch.from_numpy(parts).to(dev)
    out = torch.full((2,), float("nan"), device=dev)
    call("fbn_pack_extras", ptr(loss), ptr(slots), ptr(out), st)
    _same("the loss through the pack", out[0], loss[0])
    assert float(out[1]) == float(np.float32(math.fsum(parts))), "the table part: the slots' sum rounded once"
    assert bool((slots == 0).all()), "the pack zeroes the table slots"
    # ---- unpack_extras: the loss, and slot 0 += double(in[1])
    pre = torch.from_numpy(_slots_for(2.0, 6))
    wire = torch.tensor([0.25, 0.123], dtype=torch.float32)
    sums, lo, wire_d = pre.to(dev), _f32(float("nan"), dev), wire.to(dev)
    call("fbn_unpack_extras", ptr(wire_d), ptr(lo), ptr(sums), st)
    want = pre.clone()
    want[0] = pre[0] + wire[1].double()
    _same("loss", lo[0], wire[0])
    _same("slots after unpack_extras", sums, want)
    # ---- unpack_sumsq: the same and the dense squares in one launch
    x = 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(n + 1))
    sums, lo, xd = pre.to(dev), _f32(float("nan"), dev), x.to(dev)
    call("fbn_unpack_sumsq", ptr(wire_d), ptr(lo), ptr(xd) if n else None, n, ptr(sums), st)
    got = sums.cpu()
    _same("loss", lo[0], wire[0])
    want_s = float((x.double() ** 2).sum()) + float(wire[1].double())
    bound = ar.sumsq_bound(want_s, n + 1, 2.0)
    err = abs(float((got - pre).sum()) - want_s)
    _record("unpack_sumsq", err / bound, 0.0)
    assert err <= bound and bool((got >= pre).all()), (err, bound)
    if n == 0:
        _same("slots after unpack_sumsq, n = 0", got, want)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("ns", [1, 3, 8])
def test_sum_slices(hip_device, ns, dtype):
    dev, st, L = hip_device, _lib.stream_handle(hip_device), _lib.lib()
    n = 1003
    td = torch.float32 if dtype == 0 else torch.float64
    x = torch.randn((ns, n), generator=torch.Generator().manual_seed(ns), dtype=td)
    out, xd = torch.full((n + 4,), float("nan"), dtype=td, device=dev), x.to(dev)
    call("fbn_sum_slices", ptr(xd), ns, n, dtype, ptr(out), st)
    want = x[0].clone()
    for k in range(1, ns):
        want = want + x[k]
    _same("left-to-right sum", out[:n], want)
    assert bool(torch.isnan(out[n:]).all())
    f = L.fbn_sum_slices
    got = {"ns = 0": f(ptr(xd), 0, n, dtype, ptr(out), st), "dtype 2": f(ptr(xd), ns, n, 2, ptr(out), st),
           "in NULL": f(None, ns, n, dtype, ptr(out), st), "out NULL": f(ptr(xd), ns, n, dtype, None, st)}
    assert got == {k: FBN_ERR_ARG for k in got}
    assert L.fbn_sum_slices(None, 0, 0, 5, None, st) == FBN_OK
    torch.cuda.synchronize()
    _same("out after the refused calls", out[:n], want)


# ------------------------------------------------------------------------------------------- dense Adam
CANARY = 8
DENSE_N = [1, 2, 3, 4, 5, 7, 1027, 4099, 3 * 1024 * 4 + 5]


def _padded(t, dev, fill=123.25):
    out = torch.full((t.numel() + CANARY,), fill, dtype=t.dtype)
    out[:t.numel()] = t
    return out.to(dev)


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("n", DENSE_N)
def test_adam_dense(hip_device, n, decoupled):
    """coef as a pointer, NULL (= 1) and from the slots; *step = 7 of the 20-step table; canaries behind n."""
    dev, st = hip_device, _lib.stream_handle(hip_device)
    tab, step = table(dev, decoupled), _i32(STEP, dev)
    for mode in ("ptr", "null", "slots"):
        coef = ar.f32(0.37) if mode == "ptr" else 1.0
        p, m, v, g = ar.make_state(n, 11, WD, coef if mode != "slots" else 0.5, decoupled)
        d = [_padded(t, dev) for t in (p, m, v, g)]
        parts = _slots_for(4.0, 7)                                  # norm 2: coef about 0.5
        slots = torch.from_numpy(parts).to(dev) if mode == "slots" else None
        cout, cin = _f32(float("nan"), dev), _f32(coef, dev)
        call("fbn_adam_dense", ptr(d[0]), ptr(d[3]), ptr(d[1]), ptr(d[2]), n, ptr(cin) if mode == "ptr" else None,
             ptr(tab), ptr(step), wd_arg(decoupled), BETA2, EPS, ptr(slots), 1.0, ptr(cout) if mode == "slots" else None,
             None, st)
        torch.cuda.synchronize()
        if mode == "slots":
            coef = float(cout)
            rc, ec = ar.clip_ref(parts, 1.0)[1], ar.clip_bounds(parts, 1.0, sq_roundings=0)[1]
            assert abs(coef - rc) <= ec and coef < 1.0
        _check_step(f"dense.{mode}", (p, m, v), g.double(), None, coef, STEP, decoupled, [t[:n] for t in d[:3]])
        for name, t in zip("pmv", d[:3]):
            assert bool((t[n:] == 123.25).all()), f"{name}: written past n"
        _same("g", d[3][:n], g)
        assert int(step) == STEP


def test_adam_dense_refusals(hip_device):
    """A misaligned pointer: FBN_ERR_ARG; n = 0: FBN_OK; neither writes anything."""
    dev, st, L = hip_device, _lib.stream_handle(hip_device), _lib.lib()
    n = 64
    p, m, v, g = ar.make_state(n, 12)
    d = [_padded(t, dev) for t in (p, m, v, g)]
    tab, step, coef = table(dev, False), _i32(STEP, dev), _f32(0.5, dev)
    f = lambda pp, gg, mm, vv, nn: L.fbn_adam_dense(pp, gg, mm, vv, nn, ptr(coef), ptr(tab), ptr(step), WD, BETA2, EPS, None,
                                                    1.0, None, None, st)
    a = [ptr(t) for t in d]
    got = {"p": f(a[0] + 4, a[3], a[1], a[2], n - 4), "g": f(a[0], a[3] + 8, a[1], a[2], n - 4),
           "m": f(a[0], a[3], a[1] + 4, a[2], n - 4), "v": f(a[0], a[3], a[1], a[2] + 12, n - 4)}
    assert got == {k: FBN_ERR_ARG for k in got}
    assert f(a[0], a[3], a[1], a[2], 0) == FBN_OK
    torch.cuda.synchronize()
    for t, t0 in zip(d, (p, m, v, g)):
        _same("after the refused calls", t[:n], t0)


# ------------------------------------------------------------------------------------- eager table Adam
def _table_state(c, nrows, D, seed, decoupled, dev):
    """(p, m, v) [nrows + 4][D] on the CPU; the planted edge elements sit in the first claimed row (row 0 when
    the batch names none)."""
    V = nrows + 4
    p, m, v, _ = ar.make_state(V * D, seed, WD, 1.0, decoupled)
    out = [t.view(V, D).clone() for t in (p, m, v)]
    if c.rows.size:
        r = int(c.rows[0])
        for t in out:
            t[[0, r]] = t[[r, 0]]
    return out


def _row_grads(c, nrows, D):
    """float64 gradient and its error bound per table row ([nrows + 4][D]; zero off the claimed rows)."""
    g = torch.zeros((nrows + 4, D), dtype=torch.float64)
    e = torch.zeros_like(g)
    rows = torch.from_numpy(c.rows)
    g[rows], e[rows] = c.grad, c.grad_err
    return g, e


def _layouts(D):
    return [("vec", False, False), ("vec", True, False), ("rows", False, D == 128), ("rows", True, D == 128)]


@pytest.mark.parametrize("nrows", [1, 37, 1500])
@pytest.mark.parametrize("D", [16, 32, 64, 128, 256])
def test_adam_table(hip_device, D, nrows):
    """fbn_adam_table modes 0 / 1 / 2 and fbn_adam_touched (with and without ``last``) on hand-built claims:
    unflagged, flagged and FBN_GRAD_FULL rows in both gradient layouts (bf16 per-entry rows at D = 128)."""
    dev, st = hip_device, _lib.stream_handle(hip_device)
    V = nrows + 4
    for li, (layout, full, bf16) in enumerate(_layouts(D)):
        decoupled = bool(li & 1)
        tab, step, wd = table(dev, decoupled), _i32(STEP, dev), wd_arg(decoupled)
        coef = ar.f32(0.37)
        c = _claims(layout, D, full, bf16, V=nrows, seed=li)
        c.map = torch.cat([c.map, torch.full((4,), -1, dtype=torch.int32)])
        c.rs = torch.cat([c.rs, c.rs[:1].expand(4, 4)])
        before = _table_state(c, nrows, D, 20 + li, decoupled, dev)
        g64, gerr = _row_grads(c, nrows, D)
        touched = torch.zeros(V, dtype=torch.bool)
        touched[torch.from_numpy(c.rows)] = True
        live = torch.arange(V) < nrows
        tag = f"D{D}.{layout}{'.full' if full else ''}{'.bf16' if bf16 else ''}"
        for kern in ("mode0", "mode1", "mode2", "touched", "touched.nolast"):
            d = _DevClaims(c, dev)
            s = [t.to(dev) for t in before]
            cin = _f32(coef, dev)
            if kern.startswith("mode"):
                call("fbn_adam_table", ptr(s[0]), ptr(s[1]), ptr(s[2]), nrows, D, ptr(d.map), *d.src(c), ptr(cin),
                     ptr(tab), ptr(step), wd, BETA2, EPS, int(kern[4]), st)
            else:
                call("fbn_adam_touched", ptr(s[0]), ptr(s[1]), ptr(s[2]), D, ptr(d.map), *d.src(c), c.n, ptr(cin),
                     ptr(tab), ptr(step), wd, BETA2, EPS, d.rs.data_ptr() + 8 if kern == "touched" else None, st)
            torch.cuda.synchronize()
            s = [t.cpu() for t in s]
            stepped = live & {"mode0": torch.ones_like(live), "mode1": ~touched, "mode2": ~touched}.get(kern, touched)
            if bool(stepped.any()):
                _check_step(f"table.{kern.split('.')[0]}", [t[stepped] for t in before], g64[stepped], gerr[stepped], coef, STEP,
                            decoupled, [t[stepped] for t in s])
            for name, got, was in zip("pmv", s, before):
                _same(f"{tag} {kern}: {name} of the rows it must not touch", got[~stepped], was[~stepped])
            if kern in ("mode1", "mode2"):
                _same(f"{tag} {kern}: map", d.map, c.map)
                _same(f"{tag} {kern}: extra", d.extra, c.extra)
            else:
                assert bool((d.map == -1).all()), f"{tag} {kern}: map not reset on the touched rows"
                assert bool((d.extra == 0).all()), f"{tag} {kern}: a flagged claimer's extra not zeroed"
            _same(f"{tag} {kern}: slot_row", d.slot_row, c.slot_row)
            want_rs = c.rs.clone()
            if kern == "touched":
                want_rs[torch.from_numpy(c.rows), 2] = STEP + 1
            _same(f"{tag} {kern}: row state", d.rs, want_rs)
            _same(f"{tag} {kern}: gvec", d.gvec, c.gvec_store if c.bf16 else c.gvec)


# ---------------------------------------------------------------------------------------- the step tail
N_DENSE_TAIL = 4 * 262144 + 1203          # the tail's 256-block cap (262144 vectors a round): a second round of 300
RING_N, TB, TL, TV = 3, 8, 20, 400
RING_FILL, HIST_FILL = 7.5, -1.0


class _Tail:
    """One step's inputs at B = 8, L = 20: hand-built claims over a table of 400 rows (+ 4 canary rows), three of
    the unflagged claimed rows pre-claimed by the next batch (tag high word = step + 1), the deferred-gradient
    ring, coef_hist, the norm slots (norm 2: coef about 0.5) and the counters."""

    def __init__(self, dev, D, decoupled, step, n_dense):
        self.dev, self.D, self.decoupled, self.step, self.n_dense = dev, D, decoupled, step, n_dense
        c = self.c = _claims("vec", D, False, False, B=TB, L=TL, V=TV, seed=50, step=step, pool=120)
        unfl = c.rows[~c.flagged]
        assert unfl.size >= 6 and c.flagged.any()
        self.tagged = unfl[:3]
        c.rs[torch.from_numpy(self.tagged), 1] = step + 1
        c.map = torch.cat([c.map, torch.full((4,), -1, dtype=torch.int32)])
        c.rs = torch.cat([c.rs, torch.tensor([[123, 1, step, -1]] * 4, dtype=torch.int32)])
        self.imm = c.flagged | np.isin(c.rows, self.tagged)
        self.before = _table_state(c, TV, D, 51, decoupled, dev)
        self.g64, self.gerr = _row_grads(c, TV, D)
        self.dense = ar.make_state(n_dense, 52, WD, 0.5, decoupled)
        self.parts = _slots_for(4.0, 8)
        # ---- the device side
        self.d = _DevClaims(c, dev)
        self.t = [x.to(dev) for x in self.before]
        self.dd = [_padded(x, dev) for x in self.dense]
        self.slots = torch.from_numpy(self.parts).to(dev)
        self.ring = torch.full((RING_N, TB * 2 * D), RING_FILL, device=dev)
        self.hist = torch.full((TOTAL + 1,), HIST_FILL, device=dev)
        self.ticket = torch.zeros(17, dtype=torch.int32, device=dev)
        self.rng = torch.tensor([5, 100], dtype=torch.int64, device=dev)
        self.nbt0, self.nbt1 = (torch.tensor([x], dtype=torch.int64, device=dev) for x in (11, 12))
        self.err, self.stepd = _i32(0, dev), _i32(step, dev)
        self.cout, self.nout = _f32(float("nan"), dev), _f32(float("nan"), dev)
        self.tab, self.wd, self.st = table(dev, decoupled), wd_arg(decoupled), _lib.stream_handle(dev)

    def replay_tail(self):
        """last, pend, ring, coef_hist"""
        return self.d.rs.data_ptr() + 8, self.d.rs.data_ptr() + 12, ptr(self.ring), ptr(self.hist)

    def run_tail(self):
        d, c, dd, t = self.d, self.c, self.dd, self.t
        call("fbn_adam_step_tail", ptr(dd[0]), ptr(dd[3]), ptr(dd[1]), ptr(dd[2]), self.n_dense, ptr(self.slots), 1.0,
             ptr(self.cout), ptr(self.nout), ptr(t[0]), ptr(t[1]), ptr(t[2]), self.D, ptr(d.map), *d.src(c), c.n,
             ptr(self.tab), ptr(self.stepd), self.wd, BETA2, EPS, *self.replay_tail(), RING_N, TB * 2 * self.D, TB,
             ptr(self.rng), ptr(self.nbt0), ptr(self.nbt1), ptr(self.ticket), TOTAL, ptr(self.err), self.st)
        torch.cuda.synchronize()

    def run_commit(self, coef):
        d, c, t, cin = self.d, self.c, self.t, _f32(coef, self.dev)
        call("fbn_adam_commit", ptr(t[0]), ptr(t[1]), ptr(t[2]), self.D, ptr(d.map), *d.src(c), c.n, ptr(cin),
             ptr(self.tab), ptr(self.stepd), self.wd, BETA2, EPS, *self.replay_tail(), RING_N, TB, self.st)
        torch.cuda.synchronize()

    def check_commit(self, name, coef):
        """The commit's effects: flagged claimers and pre-claimed rows stepped now; the other claimers deferred."""
        c, step = self.c, self.step
        rows = torch.from_numpy(c.rows)
        now = torch.zeros(TV + 4, dtype=torch.bool)
        now[rows[torch.from_numpy(self.imm)]] = True
        s = [x.cpu() for x in self.t]
        _check_step(f"{name}.now", [x[now] for x in self.before], self.g64[now], self.gerr[now], coef, step, self.decoupled,
                    [x[now] for x in s])
        for nm, got, was in zip("pmv", s, self.before):
            _same(f"{name}: {nm} of the deferred and the untouched rows", got[~now], was[~now])
        want = c.rs.clone()
        imm = torch.from_numpy(self.imm)
        want[rows[imm], 2] = step + 1
        want[rows[~imm], 3] = torch.from_numpy(c.vec_of[c.claimer[~self.imm]]).int()      # pend = 2 b + slot
        _same(f"{name}: row states (last of the stepped rows, pend of the deferred ones)", self.d.rs, want)
        assert bool((self.d.map == -1).all()) and bool((self.d.slot_row == -1).all()), f"{name}: map / slot_row not reset"
        assert bool((self.d.extra == 0).all()), f"{name}: a flagged claimer's extra not zeroed"
        ring = torch.full((RING_N, TB * 2 * self.D), RING_FILL)
        ring[step % RING_N] = c.gvec.flatten()
        _same(f"{name}: ring (slot step % ring_n = the vectors, the others untouched)", self.ring, ring)
        hist = torch.full((TOTAL + 1,), HIST_FILL)
        hist[step] = coef
        _same(f"{name}: coef_hist", self.hist, hist)

    def flush_and_check(self, name, coef):
        """fbn_adam_flush at step + 1: every row has then taken optimizer step ``step + 1`` exactly once -- the
        deferred ones with their ring gradient and coef_hist[step], the untouched ones with g = 0."""
        step = self.step
        self.stepd.fill_(step + 1)
        t = self.t
        call("fbn_adam_flush", ptr(t[0]), ptr(t[1]), ptr(t[2]), TV, self.D, self.d.rs.data_ptr() + 8, ptr(self.tab),
             ptr(self.stepd), self.wd, BETA2, EPS, self.d.rs.data_ptr() + 12, ptr(self.ring), ptr(self.hist), TB * 2 * self.D,
             RING_N, int(self.decoupled), self.st)
        torch.cuda.synchronize()
        s = [x.cpu() for x in t]
        _check_step(f"{name}.flush", [x[:TV] for x in self.before], self.g64[:TV], self.gerr[:TV], coef, step, self.decoupled,
                    [x[:TV] for x in s])
        for nm, got, was in zip("pmv", s, self.before):
            _same(f"{name}: {nm} of the rows past nrows after the flush", got[TV:], was[TV:])
        want = self.c.rs.clone()
        want[:TV, 2] = step + 1
        _same(f"{name}: row states after the flush", self.d.rs, want)


@pytest.mark.parametrize("D,decoupled", [(16, False), (128, True)], ids=["D16-adam", "D128-adamw"])
def test_adam_commit(hip_device, D, decoupled):
    x = _Tail(hip_device, D, decoupled, STEP, 8)
    coef = ar.f32(0.37)
    x.run_commit(coef)
    x.check_commit("commit", coef)
    assert int(x.stepd) == STEP and bool((x.ticket == 0).all())
    x.flush_and_check("commit", coef)


@pytest.mark.parametrize("D,decoupled", [(16, False), (128, True)], ids=["D16-adam", "D128-adamw"])
def test_step_tail(hip_device, D, decoupled):
    """fbn_adam_step_tail: the in-kernel clip, the dense Adam on 256 blocks and two rounds, the commit, the end of
    step; then the flush that applies the deferred gradients."""
    x = _Tail(hip_device, D, decoupled, STEP, N_DENSE_TAIL)
    x.run_tail()
    coef, norm = float(x.cout), float(x.nout)
    rn, rc = ar.clip_ref(x.parts, 1.0)
    en, ec = ar.clip_bounds(x.parts, 1.0, sq_roundings=0)
    assert abs(coef - rc) <= ec and abs(norm - rn) <= en and coef < 1.0, (coef, rc, ec, norm, rn, en)
    x.check_commit("tail", coef)
    n = x.n_dense
    _check_step("tail.dense", x.dense[:3], x.dense[3].double(), None, coef, STEP, decoupled, [t[:n] for t in x.dd[:3]])
    for nm, t in zip("pmv", x.dd[:3]):
        assert bool((t[n:] == 123.25).all()), f"dense {nm}: written past n"
    _same("dense g", x.dd[3][:n], x.dense[3])
    assert int(x.stepd) == STEP + 1 and x.rng.tolist() == [5, 101] and int(x.nbt0) == 12 and int(x.nbt1) == 13
    assert int(x.err) == 0 and bool((x.slots == 0).all()) and bool((x.ticket == 0).all())
    x.flush_and_check("tail", coef)


def test_step_tail_at_max_step(hip_device):
    """step == max_step: the counter stays put and bit 2 of err is set; the rest of the end of step happens."""
    x = _Tail(hip_device, 16, False, TOTAL, 5)
    x.run_tail()
    assert int(x.stepd) == TOTAL and int(x.err) == 2
    assert x.rng.tolist() == [5, 101] and int(x.nbt0) == 12 and int(x.nbt1) == 13
    assert bool((x.slots == 0).all()) and bool((x.ticket == 0).all())
    # the table's extra last row repeats optimizer step TOTAL
    _check_step("tail.dense", x.dense[:3], x.dense[3].double(), None, float(x.cout), TOTAL - 1, False, [t[:5] for t in x.dd[:3]])


def test_step_end(hip_device):
    dev, st = hip_device, _lib.stream_handle(hip_device)
    step, err = _i32(TOTAL - 1, dev), _i32(0, dev)
    rng = torch.tensor([5, 100], dtype=torch.int64, device=dev)
    nbt0, nbt1 = (torch.tensor([x], dtype=torch.int64, device=dev) for x in (11, 12))
    slots = torch.from_numpy(_slots_for(4.0, 8)).to(dev)
    call("fbn_step_end", ptr(step), ptr(rng), ptr(slots), ptr(nbt0), ptr(nbt1), TOTAL, ptr(err), st)
    assert int(step) == TOTAL and int(err) == 0 and rng.tolist() == [5, 101] and int(nbt0) == 12 and int(nbt1) == 13
    assert bool((slots == 0).all())
    slots.fill_(1.0)
    call("fbn_step_end", ptr(step), ptr(rng), ptr(slots), ptr(nbt0), ptr(nbt1), TOTAL, ptr(err), st)
    assert int(step) == TOTAL and int(err) == 2 and rng.tolist() == [5, 102] and int(nbt0) == 13 and int(nbt1) == 14
    assert bool((slots == 0).all())
    step.fill_(3)
    call("fbn_step_end", ptr(step), None, None, None, None, TOTAL, None, st)      # every optional pointer NULL
    assert int(step) == 4 and rng.tolist() == [5, 102] and int(err) == 2


# ----------------------------------------------------------------------------------- six locked steps
def test_six_locked_steps(hip_device):
    """Steps 3 .. 8 of 20 (the phase boundary is the step of index 5) on the device counter, advanced by
    fbn_step_end: fbn_sumsq + fbn_clip_coef, then fbn_adam_dense and fbn_adam_table mode 0, every step against
    the reference at step_consts' constants from the state read back before it."""
    dev, st = hip_device, _lib.stream_handle(hip_device)
    D, nrows, n = 16, 37, 1027
    tab = table(dev, False)
    step = _i32(3, dev)
    slots = torch.zeros(64, dtype=torch.float64, device=dev)
    rng = torch.tensor([5, 100], dtype=torch.int64, device=dev)
    err = _i32(0, dev)
    p, m, v, _ = ar.make_state(n, 31)
    dd = [t.to(dev) for t in (p, m, v)]
    c0 = _claims("vec", D, False, False, V=nrows, seed=40)
    tt = [t.to(dev) for t in _table_state(c0, nrows - 4, D, 32, False, dev)]
    gen = torch.Generator().manual_seed(33)
    scales = [0.01, 1.0, 0.02, 0.5, 0.03, 2.0]
    coefs = []
    for i, sc in enumerate(scales):
        s = 3 + i
        assert int(step) == s
        g = sc * torch.randn(n, generator=gen)
        c = ar.make_claims(ar.entry_ids(8, 20, nrows, seed=43 + i).reshape(-1), nrows, D, seed=41 + i, B=8, L=20,
                           gscale=0.02 * sc)
        d = _DevClaims(c, dev)
        gd = g.to(dev)
        call("fbn_sumsq", ptr(gd), n, None, 0, ptr(slots), st)
        call("fbn_sumsq_sparse", *d.src(c), c.n, D, ptr(slots), st)
        cf, nm = _f32(float("nan"), dev), _f32(float("nan"), dev)
        call("fbn_clip_coef", ptr(slots), 1.0, ptr(cf), ptr(nm), st)
        torch.cuda.synchronize()
        parts = [float((g.double() ** 2).sum()), float((c.grad ** 2).sum())]
        rc, ec = ar.clip_ref(parts, 1.0)[1], ar.clip_bounds(parts, 1.0, n + c.n * D, sq_roundings=3)[1]
        coef = float(cf)
        assert abs(coef - rc) <= ec, (s, coef, rc, ec)
        coefs.append(coef)
        before_d, before_t = [t.cpu() for t in dd], [t.cpu() for t in tt]
        call("fbn_adam_dense", ptr(dd[0]), ptr(gd), ptr(dd[1]), ptr(dd[2]), n, ptr(cf), ptr(tab), ptr(step), WD, BETA2, EPS,
             None, 0.0, None, None, st)
        call("fbn_adam_table", ptr(tt[0]), ptr(tt[1]), ptr(tt[2]), nrows, D, ptr(d.map), *d.src(c), ptr(cf), ptr(tab),
             ptr(step), WD, BETA2, EPS, 0, st)
        call("fbn_step_end", ptr(step), ptr(rng), ptr(slots), None, None, TOTAL, ptr(err), st)
        torch.cuda.synchronize()
        _check_step("six.dense", before_d, g.double(), None, coef, s, False, dd)
        g64, gerr = _row_grads(c, nrows - 4, D)
        _check_step("six.table", before_t, g64, gerr, coef, s, False, tt)
        assert bool((d.map == -1).all()) and bool((slots == 0).all())
    assert int(step) == 9 and rng.tolist() == [5, 106] and int(err) == 0
    assert any(cf < 1.0 for cf in coefs) and any(cf == 1.0 for cf in coefs), coefs
