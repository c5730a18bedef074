"""The step's per-sample gradient vectors written straight into their deferred-gradient ring slot
(fbn_fields_bwd_slot) and read there through the pointer cell, against the separate gvec buffer and
the step tail's ring copy (FBN_GVEC_SLOT=0): the same bits everywhere -- the kernel's outputs, and a
deterministic-mode training run (eager steps and replayed step programs) through ring wrap-arounds,
with rows whose deferred gradient waits the full rolling window (the case in which an early overwrite
of a ring slot would show)."""
import pytest
import torch

from ctr_recommendation_amd import _lib
from ctr_recommendation_amd import trainer as trmod
from ctr_recommendation_amd.data import make_batch
from ctr_recommendation_amd.trainer import FiBiNETTrainer
from oracle.fibinet_oracle import build_model as oracle_build

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", [128, 16])
def test_fields_bwd_slot_form_writes_the_ring_slot(hip_device, d):
    """Steps 0..4 over a ring of 3 slots: slot step % 3 is bitwise fbn_fields_bwd's gvec, the other
    slots keep their contents, the cell holds the slot's address; gnorm, the partial rows and dhmm
    are bitwise those of the old entry point."""
    dev = hip_device
    B, L, R, ncate, ring_n, V = 64, 4, 3, 11, 3, 1000
    lib = _lib.lib()
    P = lib.fbn_fields_bwd_partials_size(d, R, ncate)
    nblk = lib.fbn_fields_bwd_grid(B, d)
    g = torch.Generator().manual_seed(3 + d)

    def rnd(*shape):
        return torch.randn(shape, generator=g).to(dev)

    item = torch.randint(1, V, (B,), generator=g).to(dev)
    seq = torch.randint(0, V, (B, L), generator=g).to(dev)
    likes = torch.randint(0, ncate, (B,), generator=g).to(dev)
    views = torch.randint(0, ncate, (B,), generator=g).to(dev)
    hmm, ln_g, ln_b = rnd(B, d), rnd(d), rnd(d)
    w1, b1, w2, cate, X = rnd(R, 6), rnd(R), rnd(6, R), rnd(ncate, d), rnd(B, 2, d)
    a = torch.sigmoid(rnd(B, 6))
    cnt = torch.randint(1, L + 1, (B,), generator=g).float().to(dev)
    stride = B * 2 * d
    ring = rnd(ring_n, stride)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    cell = torch.zeros(2, dtype=torch.int64, device=dev)
    ptr, st = _lib.ptr, _lib.stream_handle(dev)
    for t in range(5):
        dV = rnd(B, 5, d)
        old = dict(dhmm=torch.zeros(B, d, device=dev), part=torch.zeros(nblk, P, device=dev),
                   gvec=torch.zeros(B, 2, d, device=dev), gnorm=torch.zeros(B, 2, dtype=torch.float64, device=dev))
        new = dict(dhmm=torch.zeros(B, d, device=dev), part=torch.zeros(nblk, P, device=dev),
                   gnorm=torch.zeros(B, 2, dtype=torch.float64, device=dev))
        head = (ptr(item), ptr(seq), ptr(likes), ptr(views), ptr(hmm), ptr(ln_g), ptr(ln_b), 1e-5, ptr(w1), ptr(b1),
                ptr(w2), R, ncate, ptr(cate), ptr(X), ptr(a), ptr(cnt), ptr(dV))
        _lib.call("fbn_fields_bwd", *head, ptr(old["dhmm"]), None, ptr(old["part"]), None, None, ptr(old["gvec"]),
                  ptr(old["gnorm"]), V, None, None, 0, B, L, d, st)
        before = ring.clone()
        step.fill_(t)
        _lib.call("fbn_fields_bwd_slot", *head, ptr(new["dhmm"]), None, 0, ptr(new["part"]), None, ptr(ring), ring_n,
                  stride, ptr(step), ptr(cell), ptr(new["gnorm"]), V, B, L, d, st)
        torch.cuda.synchronize()
        s = t % ring_n
        assert torch.equal(ring[s].view(B, 2, d), old["gvec"]), t
        for o in range(ring_n):
            if o != s:
                assert torch.equal(ring[o], before[o]), (t, o)
        assert int(cell[0]) == ring.data_ptr() + s * stride * 4
        for k in ("dhmm", "part", "gnorm"):
            assert torch.equal(new[k], old[k]), (t, k)
    # a ring slot smaller than the batch's vectors is refused
    with pytest.raises(RuntimeError):
        _lib.call("fbn_fields_bwd_slot", *head, ptr(new["dhmm"]), None, 0, ptr(new["part"]), None, ptr(ring), ring_n,
                  stride - 4, ptr(step), ptr(cell), ptr(new["gnorm"]), V, B, L, d, st)


_STATE = ("E", "Em", "Ev", "last", "pend", "flat_p", "flat_m", "flat_v")
_BN = ("mlp.1.running_mean", "mlp.1.running_var", "mlp.5.running_mean", "mlp.5.running_var",
       "mlp.5.num_batches_tracked")


def _run(cfg, init, batches, dev, slot, steps, mode, monkeypatch, **kw):
    """`steps` training steps over the cycled batches, each given its next batch; mode "program":
    every batch's step recorded once (a real step) and replayed afterwards."""
    monkeypatch.setattr(trmod, "_GVEC_SLOT", slot)
    tr = FiBiNETTrainer(cfg, total_steps=steps + 4, batch_size=batches[0][1].shape[0], device=dev,
                        init_state={k: v.clone() for k, v in init.items()}, **kw)
    assert tr.gvec_slot == (slot and tr.deferred)
    nb, progs, losses = len(batches), {}, []
    pool = torch.cuda.MemPool() if mode == "program" else None
    for i in range(steps):
        (b, y), nxt = batches[i % nb], batches[(i + 1) % nb][0]
        if mode == "eager" or i == 0:
            tr.step(b, y, next_batch=nxt)         # (the step ahead of the first recording prefetches its batch)
        elif i % nb not in progs:
            progs[i % nb] = tr.record_program(b, y, next_batch=nxt, pool=pool)
        else:
            tr.run_program(progs[i % nb])
        losses.append(tr.loss.item())
    torch.cuda.synchronize()
    state = {n: getattr(tr, n).clone() for n in _STATE}
    state.update({k: tr.p[k].clone() for k in _BN})
    if mode == "program":
        assert len(progs) == nb
        tr.check_program_memory(pool)
    return losses, state, tr


@pytest.fixture(scope="module")
def det_case(hip_device):
    """The trainer shape of the ring tests: B = 256, d = 128, L = 20, four batches cycled."""
    out = {}
    for V in (2000, 300):
        cfg = {"embedding_dim": 128, "vocab_size": V}
        torch.manual_seed(0)
        init = oracle_build(None, cfg).state_dict()
        batches = []
        for j in range(4):
            b, y = make_batch(700 + j, 256, V)
            batches.append(({k: v.to(hip_device) for k, v in b.items()}, y.to(hip_device)))
        out[V] = (cfg, init, batches)
    return out


@pytest.mark.parametrize("V,window", [(2000, 4), (300, 2)])
@pytest.mark.parametrize("mode", ["eager", "program"])
def test_ring_slot_path_bit_identical_to_ring_copy(hip_device, det_case, monkeypatch, V, window, mode):
    """Deterministic mode, 14 steps, ring of window + 1 slots (it wraps several times).  V = 300 with
    a window of 2: almost every row is named several times per batch and pending gradients wait the
    whole window -- the ages at which a ring slot overwritten too early would be read."""
    cfg, init, batches = det_case[V]
    kw = dict(deterministic=True, lazy_window=window)
    l_old, s_old, _ = _run(cfg, init, batches, hip_device, False, 14, "eager", monkeypatch, **kw)
    l_new, s_new, tr = _run(cfg, init, batches, hip_device, True, 14, mode, monkeypatch, **kw)
    assert tr.ring_n == window + 1 and tr.gvec_slot
    assert l_old == l_new, (l_old, l_new)
    for n in s_old:
        assert torch.equal(s_old[n], s_new[n]), n
    if V == 2000:
        assert int((s_new["pend"] >= 0).sum()) > 0    # deferred gradients are pending in the ring


def test_lazy_matches_eager_table_adam_on_ring_slot_path(hip_device, det_case, monkeypatch):
    """Lazy table Adam with the vectors in the ring slot against the eager per-step pass over every
    row, deterministic mode (duplicates folded in fixed point): losses, table, moments and the dense
    state bit-identical after the flush."""
    cfg, init, batches = det_case[2000]
    steps = 14
    monkeypatch.setattr(trmod, "_GVEC_SLOT", True)
    kw = dict(total_steps=steps + 4, batch_size=256, device=hip_device, deterministic=True)
    eager = FiBiNETTrainer(cfg, table_adam="eager", init_state={k: v.clone() for k, v in init.items()}, **kw)
    lazy = FiBiNETTrainer(cfg, table_adam="lazy", lazy_window=4, init_state={k: v.clone() for k, v in init.items()},
                          **kw)
    assert lazy.gvec_slot and not eager.gvec_slot
    for i in range(steps):
        (b, y), nxt = batches[i % 4], batches[(i + 1) % 4][0]
        le, ll = eager.step(b, y).item(), lazy.step(b, y, next_batch=nxt).item()
        assert le == ll, (i, le, ll)
    lazy.flush()
    torch.cuda.synchronize()
    for n in ("E", "Em", "Ev", "flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(eager, n), getattr(lazy, n)), n
