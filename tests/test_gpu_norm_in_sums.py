"""The clip norm off the main stream (default, float-atomic mode): the dense gradients' squares come
out of the backward's sum launch (fbn_sum_jobs_sq: every block squares what it has just written, extra
blocks square the gradients the launch does not produce) and the table part follows the duplicate fold.
The published norm and clip coefficient against fbn_sumsq_sparse_norms -- the launch this replaces --
run on copies of the same inputs: both are f64 sums cast once to f32, only the order of the f64
additions differs, so they agree to 1 ulp of f32."""
import numpy as np
import pytest
import torch

from ctr_recommendation_amd import _lib
from ctr_recommendation_amd import ops as opsmod
from ctr_recommendation_amd import trainer as trmod
from ctr_recommendation_amd.data import make_batch
from ctr_recommendation_amd.trainer import FiBiNETTrainer
from oracle.fibinet_oracle import build_model as oracle_build

pytestmark = pytest.mark.gpu


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _step_with_reference(tr, batch, y, monkeypatch, poke=None):
    """One step of `tr`; returns the reference (norm, coef) computed from copies of the norm's inputs
    taken just before the step tail consumes them.  poke: (key, value) -- that dense gradient is
    overwritten right before the sum launch (it must be one the launch does not produce)."""
    real = trmod.call
    ref, names = {}, []
    ptr = _lib.ptr

    def spy(name, *args):
        names.append(name)
        if name == "fbn_sum_jobs_sq" and poke is not None and "poked" not in ref:
            tr.g[poke[0]].fill_(poke[1])
            ref["poked"] = True
        if name == "fbn_adam_step_tail":
            torch.cuda.synchronize()
            L1 = batch["item_seq"].shape[1] + 1
            n = batch["item_id"].shape[0] * L1
            step = int(tr.step_dev.item())
            vec = (tr.ring[step % tr.ring_n] if tr.gvec_slot else tr.gvec).clone()
            gnorm, extra, slot_row, dense = tr.gnorm.clone(), tr.extra.clone(), tr.slot_row.clone(), tr.flat_g.clone()
            out = torch.zeros(64, dtype=torch.float64, device=tr.device)
            real("fbn_sumsq_sparse_norms", ptr(gnorm), ptr(vec), ptr(extra), ptr(slot_row), L1, n, tr.d, ptr(out), None,
                 ptr(dense), tr.n_dense, _lib.stream_handle(tr.device))
            torch.cuda.synchronize()
            s = 0.0
            for x in out.tolist():          # clip_from_slots: the slots in order, f64
                s += x
            total = np.sqrt(np.float32(s), dtype=np.float32)
            c = np.float32(tr.max_norm) / (total + np.float32(1e-6))
            ref["norm"], ref["coef"] = float(total), float(min(c, np.float32(1.0)))
            ref["flagged"] = int((slot_row[:n] >= 0x40000000).sum())
        return real(name, *args)

    for mod in (trmod, opsmod):             # both modules bind _lib.call by name
        monkeypatch.setattr(mod, "call", spy)
    tr.step(batch, y)
    torch.cuda.synchronize()
    for mod in (trmod, opsmod):
        monkeypatch.setattr(mod, "call", real)
    return ref, names


@pytest.mark.parametrize("V,dtype", [(300, "bf16"), (2000, "bf16"), (2000, "fp32")])
def test_norm_from_sum_launch_matches_norm_launch(hip_device, monkeypatch, V, dtype):
    """bf16: the flagship's path, the weight gradients are slab jobs of the sum launch; fp32: plain
    GEMMs, every weight gradient on the range list.  V = 300: almost every claimer is flagged (vector
    + extra summed explicitly); V = 2000: a mix with the per-sample norms."""
    B, d = 256, 128
    cfg = {"embedding_dim": d, "vocab_size": V, "compute_dtype": dtype}
    torch.manual_seed(0)
    init = oracle_build(None, {"embedding_dim": d, "vocab_size": V}).state_dict()
    b, y = make_batch(31, B, V)
    b, y = {k: v.to(hip_device) for k, v in b.items()}, y.to(hip_device)
    monkeypatch.setattr(trmod, "_NORM_IN_SUMS", True)
    seen = {}
    for poke in (None, ("mlp.1.weight", 1000.0)):
        # max_norm below the norm, so the coefficient is not the constant 1
        tr = FiBiNETTrainer(cfg, total_steps=8, batch_size=B, device=hip_device, max_norm=0.05,
                            init_state={k: v.clone() for k, v in init.items()})
        assert tr.norm_in_sums and not tr.deterministic
        ref, names = _step_with_reference(tr, b, y, monkeypatch, poke)
        norm, coef = tr.norm.item(), tr.coef.item()
        print(f"V={V} {dtype} poke={poke}: norm {norm!r} ref {ref['norm']!r}; coef {coef!r} ref {ref['coef']!r}; "
              f"flagged claimers {ref['flagged']}")
        # the norm launch ran once, as the table part only (dense = NULL), and the sum launch squared
        assert "fbn_sum_jobs_sq" in names and "fbn_sum_jobs2" not in names
        assert names.count("fbn_sumsq_sparse_norms") == 1
        assert ref["flagged"] > 0
        assert abs(norm - ref["norm"]) <= _ulp(ref["norm"]), (norm, ref["norm"])
        assert abs(coef - ref["coef"]) <= _ulp(ref["coef"]), (coef, ref["coef"])
        assert coef < 1.0
        seen[poke is None] = norm
        if poke is None:
            # mlp.0.weight's gradient: the slab job (bf16) writes 15d of its 21d columns through
            # wa_remap; the others -- V_0 and the (0, j) pairs, zero inputs -- carry exact zeros
            gw = tr.g["mlp.0.weight"]
            assert gw.shape == (512, 21 * d)
            assert float(gw[:, :d].abs().max()) == 0.0 and float(gw[:, 6 * d:11 * d].abs().max()) == 0.0
            assert float(gw[:, d:6 * d].abs().max()) > 0.0 and float(gw[:, 11 * d:].abs().max()) > 0.0
    # a BN dgamma of 1000 in 512 columns (a range-list tensor): the total moved by its squares
    assert seen[False] >= 1000.0 * np.sqrt(512.0) > 100.0 * seen[True]


def test_norm_knob_keeps_the_norm_launch(hip_device, monkeypatch):
    """FBN_NORM_IN_SUMS=0: the norm launch after the sum launch, dense part included; the same norm
    to 1 ulp as the default path on the same step."""
    V, B, d = 2000, 256, 128
    cfg = {"embedding_dim": d, "vocab_size": V, "compute_dtype": "bf16"}
    torch.manual_seed(0)
    init = oracle_build(None, {"embedding_dim": d, "vocab_size": V}).state_dict()
    b, y = make_batch(31, B, V)
    b, y = {k: v.to(hip_device) for k, v in b.items()}, y.to(hip_device)
    out = {}
    for on in (False, True):
        monkeypatch.setattr(trmod, "_NORM_IN_SUMS", on)
        tr = FiBiNETTrainer(cfg, total_steps=8, batch_size=B, device=hip_device, max_norm=0.05,
                            init_state={k: v.clone() for k, v in init.items()})
        assert tr.norm_in_sums == on
        ref, names = _step_with_reference(tr, b, y, monkeypatch)
        assert ("fbn_sum_jobs_sq" in names) == on and ("fbn_sum_jobs2" in names) == (not on)
        out[on] = (tr.norm.item(), tr.coef.item(), ref)
    print("norm/coef knob off", out[False][:2], "on", out[True][:2])
    # the float-atomic fold makes two runs of a step differ in last bits of extra: each run against
    # its own reference, and the two runs against each other to the fold's own noise
    for on in (False, True):
        n, c, ref = out[on]
        assert abs(n - ref["norm"]) <= _ulp(ref["norm"]) and abs(c - ref["coef"]) <= _ulp(ref["coef"])
    assert abs(out[True][0] - out[False][0]) <= 1e-5 * out[False][0]
