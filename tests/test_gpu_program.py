"""Step programs (the native step driver, csrc/plan.cpp): a recorded training step replayed by one
host call must be bit-identical to running the step eagerly (src/train_fibinet.py:113-123's loop
body), in every mode the bench times -- bf16 at d 128 (two streams, the next-batch prefetch, the
duplicate fold on the side stream), fp32 at d 128 (per-step temporaries from the program's private
memory pool), d 16 (eager steps run the side passes in sequence on the main stream, a recorded step
on the side stream: the replays must still match the eager run bit for bit) -- and when replays
interleave with eager steps (the bench's probe steps run eagerly between replays)."""
import pytest
import torch

from ctr_recommendation_amd.data import make_batch
from ctr_recommendation_amd.trainer import FiBiNETTrainer
from oracle.fibinet_oracle import build_model as oracle_build

pytestmark = pytest.mark.gpu


def _trainer(cfg, init, B, dev, det=False, total_steps=60):
    return FiBiNETTrainer(cfg, total_steps=total_steps, batch_size=B, device=dev, deterministic=det,
                          init_state={k: v.clone() for k, v in init.items()})


def _unique_ids(b, V, g, pool):
    """The batch's ids redrawn without repetition from `pool` (ids recur ACROSS batches, never within
    one: a row named twice in a batch is folded by float atomics, whose rounding follows arrival order
    -- two runs of the same step differ there unless the trainer is deterministic)."""
    B, L = b["item_seq"].shape
    ids = pool[torch.randperm(len(pool), generator=g)[:B * (L + 1)]].view(B, L + 1)
    b["item_id"] = ids[:, 0].clone()
    b["item_seq"] = torch.where(b["item_seq"] > 0, ids[:, 1:], torch.zeros_like(ids[:, 1:]))
    return b


@pytest.mark.parametrize("d,dtype,det,shared", [(128, "bf16", False, False), (128, "fp32", False, False),
                                                (16, "fp32", False, False), (16, "bf16", False, False),
                                                (128, "bf16_fwd", False, False), (128, "bf16", True, False),
                                                (128, "bf16", False, True), (128, "fp32", False, True),
                                                (16, "fp32", False, True)])
def test_program_replay_bit_identical_to_eager(hip_device, d, dtype, det, shared):
    """det=False: the bench's stream structure (duplicate fold on the side stream, float atomics),
    ids unique within a batch; det=True: deterministic mode (fixed-point fold on the main stream)
    with ids repeated inside batches.  shared: every program recorded into ONE memory pool, as
    bench.py records them (a temporary one recording freed may back a tensor another keeps)."""
    V, B, nb, steps = 40000, 512, 4, 14
    cfg = {"embedding_dim": d, "vocab_size": V, "compute_dtype": dtype}
    torch.manual_seed(0)
    init = oracle_build(None, dict(cfg, honour_config=False)).state_dict()
    g = torch.Generator().manual_seed(7)
    pool = torch.randperm(V - 1, generator=g)[:20000] + 1
    batches = []
    for j in range(nb):
        b, y = make_batch(60 + j, B, V)
        if not det:
            b = _unique_ids(b, V, g, pool)
        batches.append(({k: v.to(hip_device) for k, v in b.items()}, y.to(hip_device)))
    eager = _trainer(cfg, init, B, hip_device, det)
    prog_tr = _trainer(cfg, init, B, hip_device, det)
    progs = {}
    mem_pool = torch.cuda.MemPool() if shared else None
    le, lp = [], []
    # one step ahead of the first recording that prefetches (and pre-claims) its batch, as a replay
    # of program 0 will always follow one (program 3's step).  Its own claims have no pre-claims
    # (compare-and-swap: with repeated ids the winning entry is timing-dependent), so its batch has
    # every id once: both trainers start from the same bits
    wb, wy = make_batch(59, B, V)
    wb = _unique_ids(wb, V, g, pool)
    wb, wy = {k: v.to(hip_device) for k, v in wb.items()}, wy.to(hip_device)
    for tr in (eager, prog_tr):
        tr.step(wb, wy, next_batch=batches[0][0])
    for i in range(steps):
        b, y = batches[i % nb]
        nxt = batches[(i + 1) % nb][0]
        le.append(eager.step(b, y, next_batch=nxt).item())
        j = i % nb
        if j not in progs:
            progs[j] = prog_tr.record_program(b, y, next_batch=nxt, pool=mem_pool)   # a real step, recorded
        elif i == 9:
            prog_tr.step(b, y, next_batch=nxt)                           # an eager step between replays
        else:
            prog_tr.run_program(progs[j])
        lp.append(prog_tr.loss.item())
    assert le == lp, (le, lp)
    assert prog_tr.device_step() == eager.device_step() == steps + 1
    eager.flush()
    prog_tr.flush()
    for name in ("E", "Em", "Ev", "flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(eager, name), getattr(prog_tr, name)), name
    for k in ("mlp.1.running_mean", "mlp.1.running_var", "mlp.5.running_mean", "mlp.5.num_batches_tracked"):
        assert torch.equal(eager.p[k], prog_tr.p[k]), k
    assert all(len(p) > 10 for p in progs.values())
    # the address-lifetime invariant: nothing of the trainer's persistent state in a recording pool
    for pg in {id(p.pool): p.pool for p in progs.values()}.values():
        prog_tr.check_program_memory(pg)
    # out of the recorded order (the previous step prefetched another batch): refused
    with pytest.raises(RuntimeError, match="out of order"):
        prog_tr.run_program(progs[(steps + 1) % nb])


def test_program_replay_bit_identical_to_eager_long(hip_device):
    """The bench's configuration (C3's kernels at B = 512: bf16, d = 128, programs recorded into one
    pool, four batches cycled) replayed for 140 steps against the eager run: past the deferred-gradient
    ring's wrap-around (F + 1 = 129 slots) and through full rolling-window cycles, every loss, the
    table, its moments and the dense state stay bit-identical."""
    V, B, nb, steps = 40000, 512, 4, 140
    cfg = {"embedding_dim": 128, "vocab_size": V, "compute_dtype": "bf16"}
    torch.manual_seed(0)
    init = oracle_build(None, dict(cfg, honour_config=False)).state_dict()
    g = torch.Generator().manual_seed(17)
    pool = torch.randperm(V - 1, generator=g)[:20000] + 1
    batches = []
    for j in range(nb):
        b, y = make_batch(160 + j, B, V)
        b = _unique_ids(b, V, g, pool)
        batches.append(({k: v.to(hip_device) for k, v in b.items()}, y.to(hip_device)))
    eager = _trainer(cfg, init, B, hip_device, total_steps=steps + 8)
    prog_tr = _trainer(cfg, init, B, hip_device, total_steps=steps + 8)
    wb, wy = make_batch(159, B, V)
    wb = _unique_ids(wb, V, g, pool)
    wb, wy = {k: v.to(hip_device) for k, v in wb.items()}, wy.to(hip_device)
    for tr in (eager, prog_tr):
        tr.step(wb, wy, next_batch=batches[0][0])
    progs, mem_pool = {}, torch.cuda.MemPool()
    le, lp = [], []
    for i in range(steps):
        b, y = batches[i % nb]
        nxt = batches[(i + 1) % nb][0]
        le.append(eager.step(b, y, next_batch=nxt).item())
        j = i % nb
        if j not in progs:
            progs[j] = prog_tr.record_program(b, y, next_batch=nxt, pool=mem_pool)
        else:
            prog_tr.run_program(progs[j])
        lp.append(prog_tr.loss.item())
    assert le == lp, [(i, a, c) for i, (a, c) in enumerate(zip(le, lp)) if a != c][:4]
    assert prog_tr.device_step() == eager.device_step() == steps + 1
    eager.flush()
    prog_tr.flush()
    for name in ("E", "Em", "Ev", "flat_p", "flat_m", "flat_v", "last"):
        assert torch.equal(getattr(eager, name), getattr(prog_tr, name)), name


def test_program_refuses_rewritten_batch(hip_device):
    """A batch whose ids were rewritten in place (copy_) since its program was recorded is refused:
    the previous replay's pre-claims name the old ids."""
    V, B = 40000, 256
    cfg = {"embedding_dim": 128, "vocab_size": V, "compute_dtype": "bf16"}
    torch.manual_seed(0)
    init = oracle_build(None, dict(cfg, honour_config=False)).state_dict()
    tr = _trainer(cfg, init, B, hip_device)
    bs = [tuple(t.to(hip_device) if not isinstance(t, dict) else {k: v.to(hip_device) for k, v in t.items()}
                for t in make_batch(80 + j, B, V)) for j in range(3)]
    tr.step(*bs[0], next_batch=bs[1][0])
    p1 = tr.record_program(*bs[1], next_batch=bs[2][0])
    p2 = tr.record_program(*bs[2], next_batch=bs[1][0])
    tr.run_program(p1)
    bs[2][0]["item_id"].copy_(bs[0][0]["item_id"])            # new contents, same buffer
    with pytest.raises(RuntimeError, match="modified since it was recorded"):
        tr.run_program(p2)


def test_persistent_allocation_escapes_recording_pool(hip_device):
    """A buffer that outlives the step, first allocated while a step is recorded, must not take a
    block of the program's pool: a temporary the recording freed there is rewritten by every replay
    (the sharded step's duplicate-fold buffer did, and every replay of its program clobbered it)."""
    from ctr_recommendation_amd import _lib
    prog = _lib.StepProgram(hip_device)
    pool = torch.cuda.MemPool()
    n = 1 << 20
    with prog.recording(pool):
        tmp = torch.empty(n, device=hip_device)
        addr = tmp.data_ptr()
        del tmp                                            # freed into the pool
        kept = _lib.persistent(lambda: torch.zeros(n, device=hip_device))
        again = torch.empty(n, device=hip_device)          # a temporary takes the freed block back
    assert kept.data_ptr() != addr and again.data_ptr() == addr, (hex(kept.data_ptr()), hex(addr))
    torch.cuda.synchronize()
    assert float(kept.abs().max()) == 0.0


def test_pool_invariant_check_catches_a_pool_allocated_buffer(hip_device):
    """check_program_memory flags round 5's bug (7122b93's old allocation path): a buffer that outlives
    the step, allocated INSIDE a recording without _lib.persistent, lands in the recording pool -- the
    check names it; the same buffer through _lib.persistent passes."""
    from ctr_recommendation_amd import _lib
    V, B, d = 20000, 256, 128
    cfg = {"embedding_dim": d, "vocab_size": V, "compute_dtype": "bf16"}
    torch.manual_seed(0)
    init = oracle_build(None, dict(cfg, honour_config=False)).state_dict()
    tr = _trainer(cfg, init, B, hip_device)
    bs = [tuple(t.to(hip_device) if not isinstance(t, dict) else {k: v.to(hip_device) for k, v in t.items()}
                for t in make_batch(90 + j, B, V)) for j in range(2)]
    tr.step(*bs[0], next_batch=bs[1][0])
    pool = torch.cuda.MemPool()
    prog = tr.record_program(*bs[1], next_batch=bs[0][0], pool=pool)
    tr.check_program_memory(pool)                          # the tree: clean
    with prog.recording(pool):
        tr._fc_extra = torch.zeros((4096, d), device=hip_device)            # the old path: in the pool
    with pytest.raises(RuntimeError, match="_fc_extra"):
        tr.check_program_memory(pool)
    with prog.recording(pool):
        tr._fc_extra = _lib.persistent(lambda: torch.zeros((4096, d), device=hip_device))
    tr.check_program_memory(pool)


def test_program_refuses_unsupported_paths(hip_device):
    cfg = {"embedding_dim": 16, "vocab_size": 3000}
    torch.manual_seed(0)
    tr = FiBiNETTrainer(cfg, total_steps=10, batch_size=64, device=hip_device, table_adam="eager")
    b, y = make_batch(1, 64, 3000)
    with pytest.raises(ValueError, match="lazy table Adam"):
        tr.record_program({k: v.to(hip_device) for k, v in b.items()}, y.to(hip_device))


def test_early_wgrad_launch_bit_identical(hip_device, monkeypatch):
    """FBN_WGRAD_EARLY (A/B knob): the grouped weight-gradient GEMMs launched on the side stream beside
    the fields backward give the same slabs, hence bit-identical steps."""
    from ctr_recommendation_amd import trainer as trmod
    V, B, nb, steps, d = 40000, 512, 3, 6, 128
    cfg = {"embedding_dim": d, "vocab_size": V, "compute_dtype": "bf16"}
    torch.manual_seed(0)
    init = oracle_build(None, dict(cfg, honour_config=False)).state_dict()
    g = torch.Generator().manual_seed(7)
    pool = torch.randperm(V - 1, generator=g)[:20000] + 1
    batches = []
    for j in range(nb):
        b, y = make_batch(70 + j, B, V)
        batches.append(({k: v.to(hip_device) for k, v in _unique_ids(b, V, g, pool).items()}, y.to(hip_device)))
    res = []
    for early in (False, True):
        monkeypatch.setattr(trmod, "_WGRAD_EARLY", early)
        tr = _trainer(cfg, init, B, hip_device)
        losses = [tr.step(*batches[i % nb], next_batch=batches[(i + 1) % nb][0]).item() for i in range(steps)]
        tr.flush()
        res.append((losses, tr.E.clone(), tr.flat_p.clone()))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_program_replays_scalar_classes_the_step_never_passes(hip_device):
    """The replay thunks come from the header's prototypes, and the training step passes only pointers,
    int, long long and float.  Recorded here are the other scalar classes -- an unsigned long long above
    2^63 (fbn_digest_u64's base), a size_t beside a long long (fbn_sort_u64 over 3 tiles + 5 keys) and a
    double between integers (fbn_bn_moments_finalize, ntot = 2^25 + 1: no float holds it) -- and a replay
    into reset outputs must give the recorded run's bits, which are checked against the host forms."""
    from ctr_recommendation_amd import _lib, checkpoint
    dev = hip_device
    g = torch.Generator().manual_seed(3)
    base = 0xFFFFFFFF00000001
    keys = torch.randint(-(1 << 62), 1 << 62, (4096,), generator=g, dtype=torch.int64)
    dkeys, dig = keys.to(dev), torch.zeros(1, dtype=torch.int64, device=dev)
    n = 3 * _lib.FBN_SORT_TILE + 5
    skeys = torch.randint(0, 1 << 62, (n,), generator=g, dtype=torch.int64)
    sin, sout = skeys.to(dev), torch.full((n,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(_lib.call("fbn_sort_u64_workspace_size", n)), dtype=torch.uint8, device=dev)
    C, ntot, momentum, eps = 8, float((1 << 25) + 1), 0.1, 1e-5
    mu = torch.randn(C, generator=g, dtype=torch.float64)
    var = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    mom = torch.cat([ntot * mu, ntot * (var + mu * mu)]).to(dev)
    mean, invstd, run_mean = (torch.zeros(C, device=dev) for _ in range(3))
    run_var = torch.ones(C, device=dev)
    outs = (dig, sout, mean, invstd, run_mean, run_var)
    init = [o.clone() for o in outs]
    prog = _lib.StepProgram(dev)
    with torch.cuda.device(dev), prog.recording():
        st = _lib.stream_handle(dev)
        _lib.call("fbn_digest_u64", dkeys.data_ptr(), 2 * len(keys), base, dig.data_ptr(), st)
        _lib.call("fbn_sort_u64", sin.data_ptr(), n, 63, ws.data_ptr(), ws.numel(), sout.data_ptr(), st)
        _lib.call("fbn_bn_moments_finalize", mom.data_ptr(), ntot, C, mean.data_ptr(), invstd.data_ptr(),
                  run_mean.data_ptr(), run_var.data_ptr(), momentum, eps, 1, st)
    torch.cuda.synchronize(dev)
    assert prog.names == ["fbn_digest_u64", "fbn_sort_u64", "fbn_bn_moments_finalize"]
    recorded = [o.clone() for o in outs]
    assert dig.item() & checkpoint.MASK64 == checkpoint.digest_host(keys.numpy(), base)
    assert torch.equal(sout.cpu(), torch.sort(skeys).values)
    assert torch.allclose(mean.cpu().double(), mu, rtol=1e-6, atol=1e-7)
    assert torch.allclose(invstd.cpu().double(), (var + eps).rsqrt(), rtol=1e-5)
    assert torch.allclose(run_mean.cpu().double(), momentum * mu, rtol=1e-5, atol=1e-7)
    for o, i in zip(outs, init):
        o.copy_(i)
    prog.run()
    torch.cuda.synchronize(dev)
    for o, r in zip(outs, recorded):
        assert torch.equal(o, r)
