"""Save and resume of the full training state, bit for bit (FiBiNETTrainer.training_state /
load_training_state, checkpoint.save / load, the launcher's --resume).

The bar is the strongest one the project's reproducibility allows: stop anywhere, restart in a fresh
trainer, and every later loss and every bit of state equals the uninterrupted run's.  No tolerances.

Shapes: V = 3000, B = 32, L = 20, lazy_window = 4 (a 5-slot deferred-gradient ring), 20 scheduled
steps, 7 steps before the save and 8 after.  The bf16 cases run at B = 64, the smallest batch bf16 mode
takes (its weight-gradient GEMMs reduce over the batch and need K % 64 == 0).  Outside deterministic
mode the ids of a step are drawn without repetition from a pool of 1500 (rows recur ACROSS steps, never
within one: a row named twice in a batch is folded by float atomics whose rounding follows arrival
order).  By construction the save then has work to resolve: a step names at most 672 (B = 64: 1344) of
3000 rows, so the rows step 6 touched alone (no duplicates) carry a deferred gradient (pend >= 0), and
of the rows no batch named, only the quarter the rolling window visited at step 6 is current -- the
others lag (last < 7).
"""
import atexit
import functools
import os
import shutil
import tempfile

import pytest
import torch

from ctr_recommendation_amd import _lib, checkpoint
from ctr_recommendation_amd.data import make_batch
from ctr_recommendation_amd.trainer import BUFFERS, FiBiNETTrainer
from oracle.fibinet_oracle import build_model as oracle_build

pytestmark = pytest.mark.gpu

L, TOTAL, CUT, END = 20, 20, 7, 15
DEV = "cuda:0"
#        d    dtype   table_adam  deterministic  V  B
CASES = {"d16_fp32_lazy": (16, "fp32", "lazy", False, 3000, 32),
         "d128_bf16_lazy": (128, "bf16", "lazy", False, 3000, 64),
         "d128_fp32_eager": (128, "fp32", "eager", False, 3000, 32),
         "d128_bf16_lazy_det": (128, "bf16", "lazy", True, 400, 64)}


def _batches(V, n, seed, unique, B):
    g = torch.Generator().manual_seed(seed)
    pool = torch.randperm(V - 1, generator=g)[:1500] + 1
    out = []
    for s in range(n):
        b, y = make_batch(seed * 100 + s, B, V)
        if unique:
            ids = pool[torch.randperm(len(pool), generator=g)[:B * (L + 1)]].view(B, L + 1)
            b["item_id"] = ids[:, 0].clone()
            seq = ids[:, 1:].clone()
            seq[b["item_seq"] == 0] = 0
            b["item_seq"] = seq
        out.append(({k: v.to(DEV) for k, v in b.items()}, y.to(DEV)))
    return out


def _init(cfg, seed):
    torch.manual_seed(seed)
    return oracle_build(None, dict(cfg, honour_config=False)).state_dict()


def _trainer(cfg, init, table_adam="lazy", det=False, seed=2025, total=TOTAL, B=32):
    return FiBiNETTrainer(cfg, total_steps=total, batch_size=B, device=DEV, table_adam=table_adam, lazy_window=4,
                          deterministic=det, seed=seed, init_state={k: v.clone() for k, v in init.items()})


def _steps(tr, bs, lo, hi):
    return [tr.step(bs[s][0], bs[s][1], next_batch=bs[s + 1][0]).item() for s in range(lo, hi)]


def _final(tr):
    """The flushed state on the host, and its device digests."""
    tr.flush()
    torch.cuda.synchronize()
    return {n: t.detach().cpu().clone() for n, t in tr._state_tensors().items()}, tr.state_digests()


def _assert_same(a, b):
    (ta, da), (tb, db) = a, b
    assert set(ta) >= {"E", "Em", "Ev", "flat_p", "flat_m", "flat_v", "step_dev", "rng"} | set(BUFFERS)
    for n in ta:
        assert torch.equal(ta[n], tb[n]), n
    assert da == db


@functools.lru_cache(maxsize=None)
def _scenario(case):
    """U: 15 steps uninterrupted.  A: 7 steps, checkpoint.save to disk, 8 more.  R: a fresh trainer from
    another init and another dropout seed, checkpoint.load, the same 8 steps.  Run once per case."""
    d, dtype, table_adam, det, V, B = CASES[case]
    cfg = {"embedding_dim": d, "vocab_size": V, "compute_dtype": dtype}
    bs = _batches(V, END + 1, 31, not det, B)
    init = _init(cfg, 0)
    U = _trainer(cfg, init, table_adam, det, B=B)
    lu = _steps(U, bs, 0, END)
    A = _trainer(cfg, init, table_adam, det, B=B)
    la = _steps(A, bs, 0, CUT)
    torch.cuda.synchronize()
    pre = None
    if table_adam == "lazy":
        pre = (bool((A.pend >= 0).any()), int(A.last.min()), bool(A._pre_key is not None))
    root = tempfile.mkdtemp(prefix="fbn_resume_")
    atexit.register(shutil.rmtree, root, ignore_errors=True)
    ptrs = {p: t.data_ptr() for p, t in _lib.tensors_of(A)}
    checkpoint.save(root, A, extra={"cut": CUT})
    ptrs_after = {p: t.data_ptr() for p, t in _lib.tensors_of(A)}
    la += _steps(A, bs, CUT, END)
    R = _trainer(cfg, _init(cfg, 5), table_adam, det, seed=77, B=B)
    assert not torch.equal(R.flat_p, A.flat_p) and not torch.equal(R.rng, A.rng)
    extra = checkpoint.load(root, R)
    lr = _steps(R, bs, CUT, END)
    out = {"lu": lu, "la": la, "lr": lr, "pre": pre, "root": root, "extra": extra, "cfg": cfg, "init": init,
           "U": _final(U), "A": _final(A), "R": _final(R), "steps": (U.device_step(), A.device_step(), R.device_step()),
           "host_steps": (U.host_step, A.host_step, R.host_step), "ptrs": (ptrs, ptrs_after)}
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_resume_equals_uninterrupted_run(hip_device, case):
    """(a) A fresh trainer that loads the step-7 checkpoint and runs steps 7..14 on the same batches gives
    the uninterrupted run's losses and, after a flush, its state bit for bit (targets: a stale
    pre-claim, a ring slot or schedule row taken from the wrong step, a dropout stream not restored)."""
    sc = _scenario(case)
    if sc["pre"] is not None:
        pend_any, last_min, pre_posted = sc["pre"]
        # the save had deferred gradients and lagging rows to resolve, and pre-claims to forget
        assert pend_any and last_min < CUT and pre_posted, sc["pre"]
    assert sc["extra"] == {"cut": CUT}
    assert sc["lr"] == sc["lu"][CUT:], (sc["lr"], sc["lu"][CUT:])
    assert sc["steps"] == (END, END, END) and sc["host_steps"] == (END, END, END)
    _assert_same(sc["U"], sc["R"])
    assert checkpoint.verify(sc["root"], out=lambda s: None) == 0


@pytest.mark.parametrize("case", list(CASES))
def test_saving_does_not_perturb_the_run(hip_device, case):
    """(b) The trainer that saved at step 7 and went on equals the one that never saved (the save's
    flush is invisible: lazy == eager), and saving rebinds none of its tensors."""
    sc = _scenario(case)
    assert sc["la"] == sc["lu"], (sc["la"], sc["lu"])
    _assert_same(sc["U"], sc["A"])
    assert sc["ptrs"][0] == sc["ptrs"][1]


def test_mismatched_or_corrupt_state_is_refused(hip_device):
    """(c) meta is checked field by field (ValueError naming the field); a changed word is caught by the
    digest recomputed on the device after the upload (RuntimeError naming the tensor)."""
    sc = _scenario("d16_fp32_lazy")
    path = os.path.join(checkpoint.find(sc["root"]), "rank0.pt")
    cfg, init = sc["cfg"], sc["init"]

    def state():
        return torch.load(path, weights_only=True)["state"]

    with pytest.raises(ValueError, match="total_steps"):
        _trainer(cfg, init, total=TOTAL + 1).load_training_state(state())
    cfg32 = dict(cfg, embedding_dim=32)
    with pytest.raises(ValueError, match=r"\bd is 16"):
        _trainer(cfg32, _init(cfg32, 0)).load_training_state(state())
    st = state()
    st["meta"]["world"] = 2
    with pytest.raises(ValueError, match="world.*resharding"):
        _trainer(cfg, init).load_training_state(st)
    st = state()
    st["meta"]["table_adam"] = "sparse"
    with pytest.raises(ValueError, match="table_adam"):
        _trainer(cfg, init).load_training_state(st)
    st = state()
    st["Em"].view(torch.int32)[5, 3] ^= 1                      # one word of Em, one bit
    with pytest.raises(RuntimeError, match=r"digest of Em\b"):
        _trainer(cfg, init).load_training_state(st)
    # lazy and eager are interchangeable (bit-identical), and another batch size is allowed
    tr = FiBiNETTrainer(cfg, total_steps=TOTAL, batch_size=64, device=DEV, table_adam="eager", lazy_window=4,
                        init_state={k: v.clone() for k, v in init.items()})
    tr.load_training_state(state())
    assert tr.host_step == CUT and tr.device_step() == CUT


def test_load_in_place_under_step_programs(hip_device):
    """(d) load_training_state copies into the existing buffers: the step programs recorded before the
    load replay after it (their recorded addresses still name the trainer's state) and reproduce the
    first pass's losses and state; no tensor reachable from the trainer moved."""
    V, nb, d = 3000, 4, 128
    cfg = {"embedding_dim": d, "vocab_size": V, "compute_dtype": "bf16"}
    bs = _batches(V, nb + 1, 47, True, 64)
    warm, bs = bs[nb], bs[:nb]
    tr = _trainer(cfg, _init(cfg, 0), B=64)
    tr.step(warm[0], warm[1], next_batch=bs[0][0])
    progs = {}

    def one(i, eager=False):
        (b, y), nxt = bs[i % nb], bs[(i + 1) % nb][0]
        if eager:
            tr.step(b, y, next_batch=nxt)
        elif i % nb not in progs:
            progs[i % nb] = tr.record_program(b, y, next_batch=nxt)
        else:
            tr.run_program(progs[i % nb])
        return tr.loss.item()

    for i in range(8):
        one(i)
    assert len(progs) == nb
    state = tr.training_state()
    assert state["meta"]["host_step"] == 9
    first = [one(i) for i in range(8, 14)]
    ref = _final(tr)
    ptrs = {p: t.data_ptr() for p, t in _lib.tensors_of(tr)}
    tr.load_training_state(state)
    assert {p: t.data_ptr() for p, t in _lib.tensors_of(tr)} == ptrs
    assert tr.host_step == 9 and tr.device_step() == 9
    # a replay's claims come from the pre-claims its predecessor posted: the load forgot them
    with pytest.raises(RuntimeError, match="out of order"):
        tr.run_program(progs[0])
    again = [one(8, eager=True)] + [one(i) for i in range(9, 14)]
    assert again == first, (again, first)
    _assert_same(ref, _final(tr))
    for p in progs.values():
        tr.check_program_memory(p.pool)


# ------------------------------------------------------------------------------------------ two ranks
def _rank_worker(rank, world, port, root, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        V, Bg, steps, cut = 3001, 128, 6, 3
        per = Bg // world
        cfg = {"embedding_dim": 16, "vocab_size": V, "honour_config": True, "net_dropout": 0.0}
        bs = []
        for s in range(steps + 1):
            b, y = make_batch(700 + s, Bg, V)
            bs.append(({k: v[rank * per:(rank + 1) * per].to(DEV) for k, v in b.items()},
                       y[rank * per:(rank + 1) * per].to(DEV)))

        def mk(seed):
            torch.manual_seed(seed)
            init = oracle_build(None, cfg, honour_config=True).state_dict()
            return FiBiNETTrainer(cfg, total_steps=TOTAL, batch_size=per, device=DEV, rank=rank, world=world,
                                  init_state=init, stage_on_cpu=True, deterministic=True, lazy_window=4)

        def run(tr, lo, hi):
            return [tr.step(bs[s][0], bs[s][1], next_batch=bs[s + 1][0]).item() for s in range(lo, hi)]

        def dig(tr):
            tr.flush()
            return {n: v for n, v in tr.state_digests().items() if n in ("E", "Em", "Ev", "flat_p")}

        U = mk(0)
        lu = run(U, 0, steps)
        A = mk(0)
        run(A, 0, cut)
        checkpoint.save(os.path.join(root, "ok"), A, extra={"cut": cut})
        dist.barrier()                       # rank 0 has written the manifest and ``latest``
        R = mk(9)
        extra = checkpoint.load(os.path.join(root, "ok"), R)
        lr = run(R, cut, steps)
        same = lr == lu[cut:] and dig(R) == dig(U) and extra == {"cut": cut}
        # a replica whose dense parameters drifted: rank 0 refuses to make the save ``latest``
        if rank == 1:
            A.flat_p[3] += 1.0
        err = ""
        try:
            checkpoint.save(os.path.join(root, "bad"), A)
        except RuntimeError as e:
            err = str(e)
        dist.barrier()
        refused = ("replicas diverged: flat_p" in err) if rank == 0 else err == ""
        no_latest = not os.path.exists(os.path.join(root, "bad", "latest"))
        q.put((rank, "ok", same, refused and no_latest, (lr, lu[cut:])))
    except Exception as e:  # surface worker failures in the test
        q.put((rank, repr(e), False, False, None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_resume_and_replica_drift_check(hip_device, tmp_path):
    """(e) Two ranks sharing the device (gloo, host-staged collectives, deterministic): 3 steps, save,
    a fresh pair of trainers loads and runs 3 more -- per-rank losses and E / Em / Ev / flat_p digests
    equal the uninterrupted 6-step run's; a rank whose flat_p was corrupted before the save makes
    rank 0 raise "replicas diverged" and nothing becomes ``latest``."""
    import socket
    from tests._spawn import spawn_and_wait
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    res = spawn_and_wait(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, rank_args=True, timeout=300.0)
    for rank, status, same, refused, losses in sorted(res):
        assert status == "ok", (rank, status)
        assert same, (rank, losses)
        assert refused, rank


# ------------------------------------------------------------------------------------------ launcher
CONFIG = """
base_expid: MM_FiBiNET_Run
dataset_id: MicroLens_1M_x1
dataset_config:
  MicroLens_1M_x1:
    data_format: parquet
    train_data: {train}
    valid_data: {valid}
    test_data: {test}
    item_info: {info}
MM_FiBiNET_Run:
  model: MM_FiBiNET
  learning_rate: 0.001
  batch_size: 512
  embedding_dim: 16
  max_len: 20
  epochs: 2
  weight_decay: 1e-5
  net_dropout: 0.25
  deterministic: true
"""


def test_launcher_resume_reproduces_the_uninterrupted_run(hip_device, tmp_path):
    """(f) 2 epochs x 8 steps: run(max_steps=11, save_every=4) then run(resume=dir) against one
    uninterrupted run -- the same history and valid log-loss as Python floats, the same final state
    digests; the resumed run says where it picks up (epoch 2, step 3)."""
    from ctr_recommendation_amd.data import write_microlens_parquet
    from ctr_recommendation_amd.train import run
    p = write_microlens_parquet(str(tmp_path), n_train=4096, n_valid=2048, n_test=1024, n_items=600, seq_width=20,
                                item_id_stride=3, seed=21)
    cfg = str(tmp_path / "fibinet_config.yaml")
    with open(cfg, "w") as f:
        f.write(CONFIG.format(train=p["train_data"], valid=p["valid_data"], test=p["test_data"], info=p["item_info"]))
    sdir = str(tmp_path / "state")
    full = run(cfg, checkpoint=str(tmp_path / "a" / "best.pth"), log=lambda s: None)
    assert not os.path.exists(sdir) and "stopped" not in full          # nothing extra without the new arguments
    logs = []
    part = run(cfg, checkpoint=str(tmp_path / "b" / "best.pth"), log=logs.append, max_steps=11, save_every=4,
               state_dir=sdir)
    assert part["stopped"] and [h[0] for h in part["history"]] == [1] and part["trainer"].host_step == 11
    assert sorted(n for n in os.listdir(sdir) if n.startswith("step-")) == ["step-00000008", "step-00000011"]
    assert any(ln.startswith("Stopped after 11 steps at Epoch 2 | Step 3") for ln in logs)
    del part
    logs = []
    res = run(cfg, checkpoint=str(tmp_path / "b" / "best.pth"), log=logs.append, resume=sdir)
    assert logs[1].startswith(f"Resumed from {sdir} | Epoch 2 | Step 3 |"), logs[:3]
    assert res["history"] == full["history"] and len(res["history"]) == 2
    assert res["valid_logloss"] == full["valid_logloss"]
    assert res["best_auc"] == full["best_auc"]
    _assert_same(_final(full["trainer"]), _final(res["trainer"]))
    assert res["trainer"].host_step == 16
    a = torch.load(str(tmp_path / "a" / "best.pth"), weights_only=True)
    b = torch.load(str(tmp_path / "b" / "best.pth"), weights_only=True)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert checkpoint.verify(sdir, out=lambda s: None) == 0
