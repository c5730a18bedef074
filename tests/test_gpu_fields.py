"""The fields kernels (K1 / K2 / K4: csrc/fields.hip, csrc/fields_common.h) and the element-wise pair kernels
(K5: csrc/mlp.hip) against float64, each entry point on its own (pytest -m gpu).

Inputs come from a seeded generator on the CPU (tests/_fields_ref.py: make_case), the reference is plain
torch float64 on the CPU (fields_ref / fields_bwd_ref / pairs_ref) and every output buffer starts as NaN (7
for integer buffers), so an element no kernel wrote fails.  The tolerances are the first-order error bounds
of _fields_ref.py (fwd_bounds / bwd_bounds: sums of K u S with the counts K stated there); every check
prints "[fields-ratio] <name> kernel=<worst error / bound> f32ref=<the same for the torch float32 CPU
evaluation of the reference>", and the float32 reference must itself meet the bound (ratio <= 1).

Worst ratios over the whole file on an MI355X (kernel / float32 reference): X5 0.64 / 0.64, field 4 0.30 / 0.34,
a 0.41 / 0.41, Vc 0.39 / 0.39, dhmm 0.17 / 0.20, gvec 0.54 / 0.96, gnorm 0.73 / 0.72, gtab 0.41 / 0.64, sendbuf 1.00 / 1.00
(the bf16 rows: half an ulp is the rounding itself), pairs dV 0.49 / 0.63, dU 0.66 / 0.66; the parameter gradients,
through param_grads and as partial rows: cate 0.19 / 0.30, ln_b 0.13 / 0.19, b2 0.10 / 0.05, ln_g 0.08 / 0.09,
hb 0.07 / 0.09, w2 0.07 / 0.05, w1 0.04 / 0.09, b1 0.03 / 0.04.  The bounds are worst-case sums over D- to B-term
reductions while rounding errors accumulate like a random walk, so on the sums over the batch the honest
float32 evaluation sits a factor 3 to 25 below its bound, and the kernel sits where it does; on a single case
with few samples it can sit lower still (B = 1: the reduction adds zeros).  Nothing is loosened for that.

What covers what (entry point x D x mode -> test):
  fbn_fields_fwd      D 16..256, table          test_fields_case[D*-B*-L20]          X, cnt, a, Vc, Vc16, c, c16, map
                      D 16 / 128, L 0..32       test_fields_case[...-L0 .. -L32]
                      D 16 / 256, R 1..8        test_fields_case[...-R*]
                      D 16 / 128 / 256, rows    test_fields_case[...-moderows_f32 / rows_bf16]
                      HCH 5 / 10 / 20, CMP      test_fields_case[...-hch* / -cmp]
                      grid cap (1024 blocks)    test_fields_case[D256-B4099-L2], [D16-B65539-L2]
  fbn_fields_fwd_hot  D 128, Zipf               test_fields_case[...-hot]
  fbn_fields_bwd      all of the above          the same cases: gtab + param_grads, then gvec + gnorm + partial
                                                rows (param_grads NULL, dhmm NULL, dhmm16); rows modes: sendbuf
                      grid cap (512 blocks)     test_fields_case[D256-B2051-L2], [D16-B32771-L2]
                      collisions (V = 61), Zipf test_fields_case[...-familycollide / familyzipf]
  fbn_fields_bwd_img  D 128 / 32                test_fields_bwd_img_and_slot
  fbn_fields_bwd_slot D 128 / 32                test_fields_bwd_img_and_slot
  error flag          item / history / likes / views   test_bad_id_raises_the_flag
  fbn_pairs_fwd, fbn_pairs_fwd_img, fbn_pairs_bwd, fbn_pairs_bwd_img   D 16..256, B 1 / 37 / 1000   test_pairs
"""
import copy
import ctypes

import pytest
import torch

from ctr_recommendation_amd import _lib
from tests import _fields_ref as fr

pytestmark = pytest.mark.gpu
U = fr.U
ptr = _lib.ptr


# ---------------------------------------------------------------------------------------------- helpers
def _ratio(got, ref, bound):
    err = (got.detach().double().cpu() - ref.detach().double()).abs()
    bound = bound.detach().double().expand_as(err)
    nan = bool(torch.isnan(err).any())
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))       # err > 0 = bound: inf
    return (float(ratio.max()) if ratio.numel() else 0.0), ratio, nan


def _check(name, got, ref, bound, ref32=None, w32=None):
    """|got - ref| <= bound elementwise (float64).  ref32: the float32 CPU evaluation of the reference,
    held to the same bound (w32: its ratio where it has a reference of its own).  Prints both worst
    error / bound ratios."""
    worst, ratio, nan = _ratio(got, ref, bound)
    assert not nan, f"{name}: NaN in the output (an element was not written?)"
    if w32 is None:
        w32 = _ratio(ref32, ref, bound)[0]
    print(f"[fields-ratio] {name} kernel={worst:.4f} f32ref={w32:.4f}")
    if worst > 1.0:
        i = int(ratio.flatten().argmax())
        raise AssertionError(f"{name}: error / bound = {worst:.3f} at flat index {i}: got "
                             f"{got.flatten()[i].item()!r}, reference {ref.flatten()[i].item()!r}, "
                             f"bound {bound.expand_as(ratio).flatten()[i].item():.3e}")
    assert not w32 > 1.0, f"{name}: the float32 reference exceeds the bound ({w32:.3f}): the bound is too tight"
    return worst


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dtype, device=dev)


def _sevens(shape, dev, dtype=torch.int16):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), 7, dtype=dtype, device=dev)


def _bf16_bits(t):
    """bf16 round-to-nearest-even image of a float32 tensor, as int16 bits."""
    return t.to(torch.bfloat16).view(torch.int16)


def _widen(bits):
    return bits.view(torch.bfloat16).float()


class _Dev:
    """A case's inputs on the device."""

    def __init__(self, c, dev):
        self.c, self.dev, self.st = c, dev, _lib.stream_handle(dev)
        for k in ("item_id", "item_seq", "likes", "views", "hmm", "ln_g", "ln_b", "cate", "table", "w1", "b1", "w2",
                  "b2", "dV", "rows", "pos"):
            v = getattr(c, k)
            setattr(self, k, None if v is None else v.to(dev).contiguous())
        self.rows_mode = c.mode != "table"
        self.n_entries = c.B * (c.L + 1)

    def ids(self):
        return (ptr(self.item_id), ptr(self.item_seq), ptr(self.likes), ptr(self.views))

    # ---------------------------------------------------------------- forward
    def fwd(self, c16=False, vc=True, with_map=True, hot=False):
        c, dev = self.c, self.dev
        B, D, L = c.B, c.D, c.L
        ldc = 15 * D + 8
        o = {"X": _nan((B, 2, D), dev), "Vc": _nan((B, 5, D), dev) if vc else None, "Vc16": _sevens((B, 5, D), dev),
             "c": _sevens((B, ldc), dev) if c16 else _nan((B, ldc), dev), "a": _nan((B, 6), dev), "cnt": _nan(B, dev),
             "err": torch.zeros(1, dtype=torch.int32, device=dev), "map": None, "slot_row": None}
        if with_map and not self.rows_mode:
            o["map"] = torch.full((c.V,), -1, dtype=torch.int32, device=dev)
            o["slot_row"] = torch.full((self.n_entries,), -1, dtype=torch.int32, device=dev)
        senet = (ptr(self.w1), ptr(self.b1), ptr(self.w2), ptr(self.b2), c.R)
        outs = (ptr(o["X"]), ptr(o["Vc"]), ptr(o["Vc16"]), ptr(o["c"]), ldc, int(c16), ptr(o["a"]), ptr(o["cnt"]),
                ptr(o["err"]), ptr(o["map"]), ptr(o["slot_row"]), B, L, D)
        head = (*self.ids(), ptr(self.hmm), ptr(self.ln_g), ptr(self.ln_b), c.ln_eps, ptr(self.cate), c.n_cate)
        if hot:
            H = 8192 // D
            cnt = torch.zeros(c.V, dtype=torch.int32, device=dev)
            lst, n = _sevens(H, dev, torch.int32), torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.call("fbn_hot_rows", ptr(self.item_id), ptr(self.item_seq), B, L, c.V, ptr(cnt), ptr(lst), ptr(n), H, 2,
                      0, self.st)
            _lib.call("fbn_fields_fwd_hot", *head, ptr(self.table), c.V, *senet, *outs, ptr(lst), ptr(n), H, self.st)
            torch.cuda.synchronize()
            o["hot_n"] = int(n)
        elif self.rows_mode:
            _lib.call("fbn_fields_fwd", *head, ptr(self.rows), self.n_entries, ptr(self.pos), *senet, *outs,
                      int(c.mode == "rows_bf16"), self.st)
        else:
            _lib.call("fbn_fields_fwd", *head, ptr(self.table), c.V, None, *senet, *outs, 0, self.st)
        torch.cuda.synchronize()
        return o

    # --------------------------------------------------------------- backward
    def bwd(self, f, out="gtab", params=True, dhmm=True, entry="plain", step=0, ring_n=3):
        """entry plain / img / slot; out gtab / gvec / send.  f: the forward's outputs (X, a, cnt)."""
        c, dev, lib = self.c, self.dev, _lib.lib()
        B, D, L, R = c.B, c.D, c.L, c.R
        P, nblk = lib.fbn_fields_bwd_partials_size(D, R, c.n_cate), lib.fbn_fields_bwd_grid(B, D)
        assert P == sum(fr._segments(D, R, c.n_cate)) and nblk == fr.bwd_launch_shape(B, D)[0]
        o = {"dhmm": _nan((B, D), dev) if dhmm else None, "part": _nan((nblk, P), dev),
             "dhmm16": _sevens((2, B, D) if entry == "img" else (B, D), dev), "grads": None}
        pg = None
        if params:
            o["grads"] = {k: _nan(n, dev) for k, n in zip(fr.GRAD_KEYS, fr._segments(D, R, c.n_cate))}
            arr = (ctypes.c_void_p * 8)(*[o["grads"][k].data_ptr() for k in fr.GRAD_KEYS])
            pg = ctypes.cast(arr, ctypes.c_void_p).value
        head = (*self.ids(), ptr(self.hmm), ptr(self.ln_g), ptr(self.ln_b), c.ln_eps, ptr(self.w1), ptr(self.b1),
                ptr(self.w2), R, c.n_cate, ptr(self.cate), ptr(f["X"]), ptr(f["a"]), ptr(f["cnt"]), ptr(self.dV))
        if entry == "slot":
            stride = B * 2 * D + 4
            o["ring"] = _nan((ring_n, stride), dev)
            o["cell"] = _sevens(2, dev, torch.int64)
            o["gnorm"] = _nan((B, 2), dev, torch.float64)
            stp = torch.full((1,), step, dtype=torch.int32, device=dev)
            _lib.call("fbn_fields_bwd_slot", *head, ptr(o["dhmm"]), ptr(o["dhmm16"]), 0, ptr(o["part"]), pg,
                      ptr(o["ring"]), ring_n, stride, ptr(stp), ptr(o["cell"]), ptr(o["gnorm"]), c.V, B, L, D, self.st)
        else:
            if out == "gtab":
                o["gtab"] = torch.zeros((c.V, D), device=dev)
            elif out == "gvec":
                o["gvec"], o["gnorm"] = _nan((B, 2, D), dev), _nan((B, 2), dev, torch.float64)
            else:
                bf = c.mode == "rows_bf16"
                o["send"] = torch.full((self.n_entries, D), float("nan"), dtype=torch.bfloat16 if bf else torch.float32,
                                       device=dev)
            _lib.call("fbn_fields_bwd_img" if entry == "img" else "fbn_fields_bwd", *head, ptr(o["dhmm"]),
                      ptr(o["dhmm16"]), ptr(o["part"]), pg, ptr(o.get("gtab")), ptr(o.get("gvec")), ptr(o.get("gnorm")),
                      c.V if not self.rows_mode else self.n_entries, ptr(self.pos) if out == "send" else None,
                      ptr(o.get("send")), int(c.mode == "rows_bf16"), B, L, D, self.st)
        torch.cuda.synchronize()
        return o


# ------------------------------------------------------------------------------------ forward checks
def _check_forward(tag, c, o64, o32, f, out, out16):
    B, D, L = c.B, c.D, c.L
    X, Vc, a, cnt = out["X"].cpu(), out["Vc"].cpu(), out["a"].cpu(), out["cnt"].cpu()
    # ---- exact
    assert int(out["err"]) == o64.err, f"{tag}: error flag {int(out['err'])}, expected {o64.err}"
    assert torch.equal(X[:, 0].double(), o64.X3), f"{tag}: X[:,0] is not the table row's bits"
    assert torch.equal(cnt.double(), o64.cnt), f"{tag}: cnt != max(1, nnz)"
    one = o64.nnz <= 1                               # no row: exactly zero; one live slot: exactly that row
    assert torch.equal(X[:, 1][one].double(), o64.X5[one]), f"{tag}: X[:,1] of an empty / single-slot history"
    assert bool((Vc[:, 3, 1] == 0).all()), f"{tag}: the dead LayerNorm column is not exactly 0"
    assert torch.equal(out["Vc16"].cpu(), _bf16_bits(Vc)), f"{tag}: Vc16 is not the bf16 RNE image of Vc"
    cc = out["c"].cpu()
    assert torch.equal(cc[:, :5 * D], Vc.view(B, 5 * D)), f"{tag}: c[:, :5D] != Vc"
    assert bool(torch.isnan(cc[:, 5 * D:]).all()), f"{tag}: c written at or past column 5D"
    for k in ("X", "a", "cnt", "Vc16"):                                  # c_bf16 call, Vc = NULL: the same bits
        assert torch.equal(out16[k], out[k]), f"{tag}: {k} differs with c_bf16 / Vc NULL"
    c16 = out16["c"].cpu()
    assert torch.equal(c16[:, :5 * D], out["Vc16"].cpu().view(B, 5 * D)), f"{tag}: bf16 c[:, :5D] != Vc16"
    assert bool((c16[:, 5 * D:] == 7).all()), f"{tag}: bf16 c written at or past column 5D"
    # ---- toleranced
    _check(f"{tag} fwd X5", X[:, 1], o64.X5, f.e_X5, o32.X5)
    _check(f"{tag} fwd a", a[:, 1:], o64.a[:, 1:], f.e_a[:, 1:], o32.a[:, 1:])
    _check(f"{tag} fwd Vc", Vc, o64.V, f.e_V, o32.V)
    # field 4 alone: Vc[:, 3] = fl(x4 a4), divided here in float64 by the a the kernel wrote (u |x4| for the product)
    a4_64, a4_32 = a[:, 4, None].double(), o32.a[:, 4, None].double()
    _check(f"{tag} fwd field4", Vc[:, 3].double() / a4_64, o64.X4, f.e_X4 + U * o64.X4, o32.V[:, 3].double() / a4_32)
    assert float(a[:, 0].min()) > 0 and float(a[:, 0].max()) < 1         # a_0 is written (it multiplies the zero field)
    _check(f"{tag} fwd a0", a[:, :1], o64.a[:, :1], f.e_a[:, :1], o32.a[:, :1])
    # ---- map / slot_row
    if out["map"] is not None:
        mp, sr = out["map"].cpu().long(), out["slot_row"].cpu().long()
        ids = torch.cat([c.item_id[:, None]] + ([c.item_seq] if L > 0 else []), 1).flatten()
        occurs = torch.zeros(c.V, dtype=torch.bool)
        occurs[ids[(ids > 0) & (ids < c.V)]] = True
        assert bool((mp[~occurs] == -1).all()) and mp[0] == -1, f"{tag}: map set for a row that does not occur"
        e = mp[occurs]
        rows = occurs.nonzero().flatten()
        assert bool(((e >= 0) & (e < ids.numel())).all()), f"{tag}: map entry out of range"
        assert torch.equal(ids[e], rows) and torch.equal(sr[e], rows), f"{tag}: map[r] = e, but entry e is not row r"
        rest = torch.ones(ids.numel(), dtype=torch.bool)
        rest[e] = False
        assert bool((sr[rest] == -1).all()), f"{tag}: slot_row set for an entry that claimed nothing"


# ----------------------------------------------------------------------------------- backward checks
def _bwd_refs(c, X, a, cnt):
    """(autograd float64, closed-form bounds) from the given float32 X / a / cnt."""
    args = fr.fwd_args(c)
    r = fr.fields_bwd_ref(*args, X, a, cnt, c.dV)
    _, bnd = fr.bwd_bounds(*args, X, a, cnt, c.dV)
    return r, bnd


class _BwdRef:
    """The backward's references of one case: float64 autograd and bounds from the kernel's own X / a / cnt;
    and, to place the bounds, the same from the float32 reference forward's X / a / cnt with the float32
    autograd beside it.  The float32 side is checked against ITS float64 twin, the kernel against its own."""

    def __init__(self, c, f, o32):
        self.c = c
        self.r, self.bnd = _bwd_refs(c, f["X"].cpu(), f["a"].cpu(), f["cnt"].cpu())
        X32 = torch.stack([o32.X3, o32.X5], 1)
        self.r32_64, self.bnd32 = _bwd_refs(c, X32, o32.a, o32.cnt)
        self.r32 = fr.fields_bwd_ref(*fr.fwd_args(c), X32, o32.a, o32.cnt, c.dV, dtype=torch.float32)

    def check(self, name, got, pick, pick_bound, extra=None):
        """pick(reference namespace) -> tensor; pick_bound(bounds namespace) -> tensor; extra(ref) is added
        to the bound (bf16 half ulp)."""
        ref, b = pick(self.r), pick_bound(self.bnd)
        worst, ratio, nan = _ratio(got, ref, b if extra is None else b + extra(ref))
        assert not nan, f"{name}: NaN in the output (an element was not written?)"
        ref32, b32 = pick(self.r32_64), pick_bound(self.bnd32)
        got32 = pick(self.r32)
        if extra is not None:
            got32, b32 = got32.bfloat16().float(), b32 + extra(ref32)
        w32 = _ratio(got32, ref32, b32)[0]
        print(f"[fields-ratio] {name} kernel={worst:.4f} f32ref={w32:.4f}")
        if worst > 1.0:
            i = int(ratio.flatten().argmax())
            raise AssertionError(f"{name}: error / bound = {worst:.3f} at flat index {i}: got "
                                 f"{got.flatten()[i].item()!r}, reference {ref.flatten()[i].item()!r}")
        assert not w32 > 1.0, f"{name}: the float32 reference exceeds the bound ({w32:.3f}): the bound is too tight"


def _check_common(tag, R_, o, reduced):
    """dhmm, dhmm16, and the parameter gradients (through param_grads, or the partial rows summed in float64)."""
    c = R_.c
    if o["dhmm"] is not None:
        R_.check(f"{tag} dhmm", o["dhmm"], lambda r: r.dhmm, lambda b: b.dhmm)
    segs = fr._segments(c.D, c.R, c.n_cate)
    assert not bool(torch.isnan(o["part"]).any()), f"{tag}: a partial row was not written"
    tot = o["part"].double().sum(0).cpu()
    parts = dict(zip(fr.GRAD_KEYS, torch.split(tot, segs)))
    for k in fr.GRAD_KEYS:
        if reduced:
            R_.check(f"{tag} param_grads {k}", o["grads"][k].cpu(), lambda r: r.grads[k].flatten(), lambda b: b.grads[k].flatten())
        R_.check(f"{tag} partial rows {k}", parts[k], lambda r: r.grads[k].flatten(), lambda b: b.grads_part[k].flatten())


def _check_gvec(tag, R_, gvec, gnorm):
    R_.check(f"{tag} gvec", gvec, lambda r: r.gvec, lambda b: b.gvec)
    # gnorm: a float64 sum of float32-rounded squares of the vectors the kernel wrote
    s2 = (gvec.double() ** 2).sum(2).cpu()
    g32 = R_.r32.gvec
    s2_32 = (g32.double() ** 2).sum(2)
    w32 = _ratio((g32 * g32).double().sum(2), s2_32, U * s2_32 + 1e-300)[0]
    _check(f"{tag} gnorm", gnorm.cpu(), s2, U * s2 + 1e-300, w32=w32)


# ------------------------------------------------------------------------------------ the case matrix
MATRIX = fr.shape_matrix()


@pytest.mark.parametrize("k", MATRIX, ids=fr.case_id)
def test_fields_case(hip_device, monkeypatch, k):
    """fbn_fields_fwd (or _hot) and fbn_fields_bwd of one case of the shape matrix (_fields_ref.shape_matrix)
    against float64.  Forward: twice (fp32 c + Vc + map; bf16 c, Vc NULL).  Backward from the forward's own
    X / a / cnt: table mode (A) dense gtab + param_grads and (B) gvec + gnorm with param_grads NULL, dhmm
    NULL and dhmm16; rows modes (A) sendbuf + param_grads and (B) the same with param_grads / dhmm NULL."""
    dev = hip_device
    c = fr.case_of(k)
    tag = fr.case_id(k)
    monkeypatch.setenv("FBN_FIELDS_HCH", k.get("hch", "10"))
    monkeypatch.setenv("FBN_FIELDS_CMP", "1" if k.get("cmp") else "0")
    d = _Dev(c, dev)
    o64 = fr.fields_ref(*fr.fwd_args(c))
    o32 = fr.fields_ref(*fr.fwd_args(c), dtype=torch.float32)
    fb = fr.fwd_bounds(o64, c.ln_g, c.ln_b, c.ln_eps, c.w1, c.b1, c.w2, c.b2)
    hot = bool(k.get("hot"))
    f = d.fwd(hot=hot)
    f16 = d.fwd(c16=True, vc=False, with_map=False, hot=hot)
    if hot:
        assert f["hot_n"] > 0, "no row was staged: the case does not reach the hot path"
    _check_forward(tag, c, o64, o32, fb, f, f16)

    R_ = _BwdRef(c, f, o32)
    if c.mode == "table":
        A = d.bwd(f, out="gtab", params=True)
        Bq = d.bwd(f, out="gvec", params=False, dhmm=False)
        _check_common(f"{tag} bwd(gtab)", R_, A, True)
        gt = A["gtab"].cpu()
        untouched = R_.r.adds == 0
        assert untouched[0] and bool((gt[untouched] == 0).all()), f"{tag}: gtab row 0 or an untouched row is not 0"
        R_.check(f"{tag} gtab", gt, lambda r: r.gtab, lambda b: b.gtab)
        _check_gvec(f"{tag} bwd(gvec)", R_, Bq["gvec"], Bq["gnorm"])
    else:
        A = d.bwd(f, out="send", params=True)
        Bq = d.bwd(f, out="send", params=False, dhmm=False)
        _check_common(f"{tag} bwd(send)", R_, A, True)
        bf = c.mode == "rows_bf16"
        for name, o in (("A", A), ("B", Bq)):
            got = o["send"].float().cpu()
            named = ~torch.isnan(R_.r.send[:, 0])
            assert bool(torch.isnan(got[~named]).all()), f"{tag}: a sendbuf row no pos entry names was written"
            R_.check(f"{tag} sendbuf {name}", got[named], lambda r: r.send[named], lambda b: b.send[named],
                     extra=fr.half_ulp_bf16 if bf else None)
        assert torch.equal(A["send"][named.to(dev)], Bq["send"][named.to(dev)])
    # the second call (param_grads NULL, dhmm NULL): the same partial rows and the same bf16 image
    assert torch.equal(A["part"], Bq["part"]), f"{tag}: partial rows differ between the two calls"
    assert torch.equal(A["dhmm16"], _bf16_bits(A["dhmm"])), f"{tag}: dhmm16 is not RNE(dhmm)"
    assert torch.equal(Bq["dhmm16"], A["dhmm16"]), f"{tag}: dhmm16 differs with dhmm NULL"


@pytest.mark.parametrize("k", fr.IMG_SLOT_CASES, ids=fr.case_id)
def test_fields_bwd_img_and_slot(hip_device, k):
    """fbn_fields_bwd_img: the split images of dhmm (hi = RNE(dhmm), lo = RNE(dhmm - hi) B D further) and
    everything else as fbn_fields_bwd; fbn_fields_bwd_slot: the vectors in ring slot step % ring_n only
    (the other slots and the slot's padding still NaN), the cell holding the slot's address."""
    dev = hip_device
    c = fr.case_of(k)
    D, tag = c.D, f"D{c.D}"
    d = _Dev(c, dev)
    f = d.fwd()
    o32 = fr.fields_ref(*fr.fwd_args(c), dtype=torch.float32)
    R_ = _BwdRef(c, f, o32)
    im = d.bwd(f, out="gvec", params=True, entry="img")
    _check_common(f"{tag} bwd_img", R_, im, True)
    _check_gvec(f"{tag} bwd_img", R_, im["gvec"], im["gnorm"])
    hi = _bf16_bits(im["dhmm"])
    assert torch.equal(im["dhmm16"][0], hi), "image form: hi is not RNE(dhmm)"
    assert torch.equal(im["dhmm16"][1], _bf16_bits(im["dhmm"] - _widen(hi))), "image form: lo is not RNE(dhmm - hi)"
    ring_n = 3
    for step in (0, 4):
        sl = d.bwd(f, params=False, entry="slot", step=step, ring_n=ring_n)
        s, n = step % ring_n, c.B * 2 * D
        _check_common(f"{tag} bwd_slot step {step}", R_, sl, False)
        _check_gvec(f"{tag} bwd_slot step {step}", R_, sl["ring"][s, :n].view(c.B, 2, D), sl["gnorm"])
        rest = sl["ring"].clone()
        rest[s, :n] = float("nan")
        assert bool(torch.isnan(rest).all()), "the slot form wrote outside slot step % ring_n"
        assert int(sl["cell"][0]) == sl["ring"].data_ptr() + s * sl["ring"].shape[1] * 4, "the cell is not the slot's address"
        assert torch.equal(sl["dhmm16"], hi) and torch.equal(sl["part"], im["part"]) and torch.equal(sl["dhmm"], im["dhmm"])
        assert torch.equal(sl["ring"][s, :n].view(c.B, 2, D), im["gvec"]) and torch.equal(sl["gnorm"], im["gnorm"])


@pytest.mark.parametrize("which", ["item", "history", "likes", "views"])
@pytest.mark.parametrize("bad", ["above", "negative"])
def test_bad_id_raises_the_flag(hip_device, which, bad):
    """One out-of-range id: the flag is 1, and the outputs follow the documented conventions (a zero item
    row / padding / cate row 0 without a gradient) -- checked against the reference, which implements
    them (test_fields_ref_host.py: by hand).  D = 16: eight history ids per lane at L = 23."""
    dev = hip_device
    c = copy.copy(fr.case_of(fr.BAD_ID_CASE))
    lim = c.V if which in ("item", "history") else c.n_cate
    v = lim + 3 if bad == "above" else -2
    for k in ("item_id", "item_seq", "likes", "views"):
        setattr(c, k, getattr(c, k).clone())
    if which == "item":
        c.item_id[40] = v
    elif which == "history":
        c.item_seq[40, 21] = v
    elif which == "likes":
        c.likes[40] = v
    else:
        c.views[40] = v
    o64 = fr.fields_ref(*fr.fwd_args(c))
    assert o64.err == 1 and float(o64.q.abs().min()) >= fr.MARGIN and float(o64.y.abs().min()) >= fr.MARGIN
    o32 = fr.fields_ref(*fr.fwd_args(c), dtype=torch.float32)
    fb = fr.fwd_bounds(o64, c.ln_g, c.ln_b, c.ln_eps, c.w1, c.b1, c.w2, c.b2)
    d = _Dev(c, dev)
    tag = f"bad {which} {bad}"
    f = d.fwd()
    _check_forward(tag, c, o64, o32, fb, f, d.fwd(c16=True, vc=False, with_map=False))
    R_ = _BwdRef(c, f, o32)
    A = d.bwd(f, out="gtab", params=True)
    _check_common(f"{tag} bwd", R_, A, True)
    gt = A["gtab"].cpu()
    assert bool((gt[R_.r.adds == 0] == 0).all())
    R_.check(f"{tag} gtab", gt, lambda r: r.gtab, lambda b: b.gtab)
    good = fr.case_of(fr.BAD_ID_CASE)
    assert int(_Dev(good, dev).fwd()["err"]) == 0


# -------------------------------------------------------------------------------------------- pairs
@pytest.mark.parametrize("B", [1, 37, 1000])
@pytest.mark.parametrize("D", [16, 32, 64, 128, 256])
def test_pairs(hip_device, D, B):
    """K5's element-wise kernels.  Forward products are one float32 rounding: bit-exact against torch's
    float32 product of the same inputs (fp32 Vc, or the widened bf16 Vc16), the bf16 output its RNE image,
    the split images exact given that product; columns [0, 5D) and >= 15D untouched (the image form owns
    [0, 5D): V's images).  Backward: dV / dU sum n <= 5 terms, |d| <= (n + 1) u sum|terms| (contraction may
    or may not fuse a product into the sum), dU16 / dU's images exact given the float32 dU written."""
    dev, st = hip_device, _lib.stream_handle(hip_device)
    g = torch.Generator().manual_seed(100 * D + B)
    V, Uf, dc = (torch.randn(s, generator=g) for s in ((B, 5, D), (B, 5, D), (B, 15, D)))
    ldc = 15 * D + 8
    dcp = torch.full((B, ldc), float("nan"))
    dcp[:, :15 * D] = dc.view(B, 15 * D)
    Vg, Ug, dcg = V.to(dev), Uf.to(dev), dcp.to(dev)
    V16 = _bf16_bits(V)
    V16g = V16.to(dev)
    for mode in (0, 1):
        for src in ("fp32", "bf16"):
            Vin = V if src == "fp32" else _widen(V16)
            prod = fr.pairs_ref(Vin, Uf, mode, dtype=torch.float32).reshape(B, 10 * D)
            assert torch.equal(prod.double(), fr.pairs_ref(Vin, Uf, mode).float().double().reshape(B, 10 * D))
            for c16 in (0, 1):
                c = _sevens((B, ldc), dev) if c16 else _nan((B, ldc), dev)
                _lib.call("fbn_pairs_fwd", ptr(Vg) if src == "fp32" else None, ptr(V16g) if src == "bf16" else None,
                          ptr(Ug), ptr(c), B, D, ldc, mode, c16, st)
                torch.cuda.synchronize()
                cc = c.cpu()
                what = f"pairs_fwd mode {mode} V {src} c16 {c16}"
                assert torch.equal(cc[:, 5 * D:15 * D], _bf16_bits(prod) if c16 else prod), what
                untouched = torch.cat([cc[:, :5 * D], cc[:, 15 * D:]], 1)
                assert bool((untouched == 7).all() if c16 else torch.isnan(untouched).all()), what + ": sentinel columns"
            # backward
            dVr, dUr, sV, sU, nV, nU = fr.pairs_bwd_ref(dc, Vin, Uf, mode)
            dV32, dU32 = fr.pairs_bwd_ref(dc, Vin, Uf, mode, dtype=torch.float32)[:2]
            dV, dU, dU16 = _nan((B, 5, D), dev), _nan((B, 5, D), dev), _sevens((B, 5, D), dev)
            _lib.call("fbn_pairs_bwd", ptr(dcg), ptr(Vg) if src == "fp32" else None, ptr(V16g) if src == "bf16" else None,
                      ptr(Ug), ptr(dV), ptr(dU), ptr(dU16), B, D, ldc, mode, st)
            torch.cuda.synchronize()
            what = f"pairs_bwd D{D} B{B} mode {mode} V {src}"
            _check(f"{what} dV", dV, dVr, (nV[None, :, None] + 1) * U * sV, dV32)
            _check(f"{what} dU", dU, dUr, (nU[None, :, None] + 1) * U * sU + 1e-300, dU32)
            assert torch.equal(dU16, _bf16_bits(dU)), what + ": dU16 is not RNE(dU)"
            if mode == 0 and src == "fp32":
                dV2, img = _nan((B, 5, D), dev), _sevens((2, B, 5, D), dev)
                _lib.call("fbn_pairs_bwd_img", ptr(dcg), ptr(Vg), ptr(Ug), ptr(dV2), ptr(img), B, D, ldc, st)
                torch.cuda.synchronize()
                hi = _bf16_bits(dU)
                assert torch.equal(dV2, dV), "pairs_bwd_img: dV differs from fbn_pairs_bwd"
                assert torch.equal(img[0], hi) and torch.equal(img[1], _bf16_bits(dU - _widen(hi))), "pairs_bwd_img: dU images"
    # the image form of the forward ("all"): c = [V | pairs] as hi / lo, V's lo image 5 B D further
    prod = fr.pairs_ref(V, Uf, 0, dtype=torch.float32).reshape(B, 10 * D)
    full = torch.cat([V.view(B, 5 * D), prod], 1)
    hi = _bf16_bits(full)
    lo = _bf16_bits(full - _widen(hi))
    for with_v in (True, False):
        ci, vi = _sevens((2, B, ldc), dev), _sevens((2, B, 5, D), dev)
        _lib.call("fbn_pairs_fwd_img", ptr(Vg), ptr(Ug), ptr(ci), ptr(vi) if with_v else None, B, D, ldc, st)
        torch.cuda.synchronize()
        cc, vv = ci.cpu(), vi.cpu()
        assert torch.equal(cc[0, :, :15 * D], hi) and torch.equal(cc[1, :, :15 * D], lo), "pairs_fwd_img: c images"
        assert bool((cc[:, :, 15 * D:] == 7).all()), "pairs_fwd_img: sentinel columns"
        assert bool((vv[0] == 7).all()), "pairs_fwd_img: V's hi image belongs to the gather"
        assert torch.equal(vv[1], lo[:, :5 * D].view(B, 5, D)) if with_v else bool((vv[1] == 7).all()), "pairs_fwd_img: V's lo image"
