"""Training launcher: the process-per-GPU counterpart of src/train_fibinet.py.

    python -m ctr_recommendation_amd.train [--config ../config/fibinet_config.yaml] [--epochs E]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \\
        -m ctr_recommendation_amd.train [--config ...]

Same surface and loop as the reference script:

* the YAML config (src/train_fibinet.py:18-28) -- the keys it reads: ``dataset_id``,
  ``base_expid``, ``dataset_config[id].{train_data, valid_data, item_info}`` and
  ``model_cfg.{embedding_dim, batch_size, max_len, learning_rate, weight_decay, epochs, seed}``;
  optional keys this build adds: ``compute_dtype`` ("fp32" default; "bf16": every GEMM operand bf16;
  "bf16_fwd": forward GEMMs bf16, backward fp32 -- C3's "bf16 fwd / fp32 grad accum"),
  ``table_adam`` ("lazy" default: exact), and ``honour_config`` (see model_fibinet.build_model);
* ``set_seed(seed)`` then ``build_model`` (:33, :67): the seeded init of the reference;
* Adam(lr, weight_decay) + BCELoss + clip_grad_norm_(10) + OneCycleLR(max_lr = 10 lr,
  epochs x steps_per_epoch, pct_start 0.3, div 25, final_div 1000) (:74-92, :113-123) -- all inside
  FiBiNETTrainer's device step;
* the epoch loop (:103-152): loss printed every 200 steps with the current lr, the epoch's mean
  train loss, valid AUC and log-loss (:133-146; counted on the device by metrics.DeviceMetrics, the
  AUC equal to utils.compute_auc's double), and the best-AUC checkpoint (App. B keys, no
  ``module.`` prefix: :148-152).

What the reference lacks and this launcher adds (opt-in; without these arguments nothing changes and
nothing extra is written): full-state checkpoints (checkpoint.py: weights, Adam moments, schedule
position, dropout stream, loader position, the epoch's running loss) every ``--save-every`` optimizer
steps and at each epoch's end under ``--state-dir``, ``--max-steps K`` (stop cleanly after K steps of
this invocation, saving first: preemptible jobs), and ``--resume DIR``: the run continues mid-epoch
and every later loss, metric and bit of state equals the uninterrupted run's.

What differs is underneath: batches come from the HBM-resident loader (loader.py: one collate
launch per batch, no worker processes, no pageable copies); the loss is accumulated on the device
and read at the print points (the reference syncs every step with ``loss.item()``); at N > 1
each process owns one GPU and a block of table rows (row-sharded trainer, SyncBN statistics,
one dense all-reduce) instead of DataParallel (:69-70), and the trainer drops the final partial
training batch so every rank steps on an equal share (the schedule's total follows).
"""
from __future__ import annotations

import argparse
import os
import struct
import time
from typing import Dict, Optional, Tuple

import numpy as np
import torch


def load_config(path: Optional[str] = None) -> Tuple[Dict, Dict, Dict]:
    """(cfg, dataset_cfg, model_cfg) as src/train_fibinet.py:18-28 reads them."""
    import yaml
    if path is None:
        path = "../config/fibinet_config.yaml"
        if not os.path.exists(path):
            path = "config/fibinet_config.yaml"
    with open(path) as f:
        cfg = yaml.safe_load(f)
    dataset_cfg = cfg["dataset_config"][cfg["dataset_id"]]
    model_cfg = cfg[cfg["base_expid"]]
    return cfg, dataset_cfg, model_cfg


def set_seed(seed: int) -> None:
    """src/utils.py:6-16 (python, numpy, torch; the device generators are seeded by torch)."""
    import random
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def _f64_bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _f64_from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<q", int(b)))[0]


def run(config: Optional[str] = None, *, epochs: Optional[int] = None, checkpoint: Optional[str] = None,
        log=print, overrides: Optional[Dict] = None, resume: Optional[str] = None,
        save_every: Optional[int] = None, state_dir: Optional[str] = None,
        max_steps: Optional[int] = None) -> Dict:
    """Train as src/train_fibinet.py does; returns {"best_auc", "history": [(epoch, loss, auc)],
    "valid_logloss": [per epoch], "trainer"}; with the model-config key ``valid_group_by`` (a batch
    column, e.g. user_id) also "valid_gauc": [per epoch] and a `` | Valid GAUC: `` field on the epoch line;
    with ``valid_calibration_bins`` (B in [1, 1024]) also "valid_ece", "valid_pcoc", "valid_ne": [per epoch]
    and `` | Valid ECE: ... | PCOC: ... | NE: ... `` on the epoch line; with ``valid_auc_ci`` (true, or a
    level in (0, 1)) also "valid_auc_se": [per epoch], DeLong's standard error of the validation AUC, and
    `` | AUC SE: 0.0012`` on the epoch line; with ``valid_isotonic: true`` the exact isotonic calibrator of
    each epoch's validation scores is fitted on the device, `` | iso blocks: K`` is appended
    to the epoch line, "valid_iso_blocks": [per epoch] is returned, and at each new best AUC the calibrator
    is saved next to the checkpoint as ``<checkpoint stem>.isotonic.json`` (predict.py --calibrator reads it).

    Weighted training loss: the model-config keys ``loss_pos_weight`` and
    ``loss_label_smoothing`` and the dataset-config key ``weight_col`` (a train-split column of per-sample
    weights) reach FiBiNETTrainer; validation and the epoch line stay unweighted.

    Full-state checkpoints (checkpoint.py; also the model-config keys ``resume_from``,
    ``checkpoint_every_steps``, ``state_dir``): save_every: one every that many optimizer steps and at
    each epoch's end, under state_dir (default: the resume directory, else ../checkpoints/state);
    max_steps: stop after that many steps of THIS call, saving first (the result then has
    "stopped": True); resume: continue the run saved under that directory, mid-epoch, one batch ahead
    as before -- its losses, metrics and state equal the uninterrupted run's bit for bit."""
    import torch.distributed as dist

    from . import checkpoint as state_ckpt
    from .loader import make_loaders
    from .model_fibinet import build_model
    from .trainer import FiBiNETTrainer

    cfg, dataset_cfg, model_cfg = load_config(config)
    model_cfg = dict(model_cfg, **(overrides or {}))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl", device_id=device)
    seed = int(model_cfg.get("seed", 2025))
    set_seed(seed)
    log0 = log if rank == 0 else (lambda *a, **k: None)
    log0(f"Training FiBiNET on {world} x {torch.cuda.get_device_name(device)}")

    train_loader, valid_loader, _ = make_loaders(dataset_cfg, model_cfg, device, rank, world, seed)
    if world > 1:
        train_loader.drop_last = True
    n_epochs = int(epochs if epochs is not None else model_cfg.get("epochs", 30))
    steps_per_epoch = len(train_loader)
    set_seed(seed)                                        # build_model after set_seed, as :33 / :67
    init = build_model(None, model_cfg).state_dict()
    trainer = FiBiNETTrainer(model_cfg, total_steps=n_epochs * steps_per_epoch,
                             batch_size=train_loader.batch_size // world, device=device, rank=rank, world=world,
                             init_state=init, seed=seed, table_adam=str(model_cfg.get("table_adam", "lazy")),
                             pos_weight=float(model_cfg.get("loss_pos_weight", 1.0)),
                             label_smoothing=float(model_cfg.get("loss_label_smoothing", 0.0)))
    del init
    best_auc, history, valid_logloss = 0.0, [], []
    group_by = model_cfg.get("valid_group_by")            # e.g. user_id: also report the per-group AUC
    valid_gauc = []
    calib_bins = model_cfg.get("valid_calibration_bins")  # e.g. 10: also report the calibration of the probabilities
    valid_ece, valid_pcoc, valid_ne = [], [], []
    auc_ci = model_cfg.get("valid_auc_ci")                # true or a level: also report DeLong's standard error of the AUC
    valid_auc_se = []
    fit_iso = bool(model_cfg.get("valid_isotonic"))       # also fit the isotonic calibrator of the validation scores
    valid_iso_blocks = []
    ev_args = {}
    if fit_iso:
        ev_args["fit_isotonic"] = True
    if auc_ci:
        ev_args["auc_ci"] = auc_ci
    if group_by:
        ev_args["group_by"] = str(group_by)
    if calib_bins:
        ev_args["calibration_bins"] = int(calib_bins)
    ckpt = checkpoint or os.path.join("..", "checkpoints", "FiBiNET_best.pth")
    resume = resume if resume is not None else model_cfg.get("resume_from")
    save_every = int(save_every if save_every is not None else model_cfg.get("checkpoint_every_steps") or 0)
    state_dir = state_dir if state_dir is not None else model_cfg.get("state_dir")
    saving = bool(state_dir) or save_every > 0 or max_steps is not None
    if saving and not state_dir:
        state_dir = resume or os.path.join("..", "checkpoints", "state")
    lists = {"valid_logloss": valid_logloss, "valid_gauc": valid_gauc, "valid_ece": valid_ece,
             "valid_pcoc": valid_pcoc, "valid_ne": valid_ne, "valid_auc_se": valid_auc_se}
    if fit_iso:
        lists["valid_iso_blocks"] = valid_iso_blocks

    def save_state(epoch: int, steps: int, loss_sum: float) -> None:
        """The run as it stands: `steps` steps of (0-based) `epoch` done, their losses summing to loss_sum."""
        state_ckpt.save(state_dir, trainer, extra={
            "epoch": epoch, "steps": steps, "loss_sum_bits": _f64_bits(loss_sum), "best_auc": best_auc,
            "history": [list(h) for h in history], "lists": {k: list(v) for k, v in lists.items()},
            "loader": train_loader.state_dict()})

    start_epoch = start_steps = 0
    start_sum = 0.0
    if resume:
        extra = state_ckpt.load(resume, trainer)
        start_epoch, start_steps = int(extra["epoch"]), int(extra["steps"])
        start_sum = _f64_from_bits(extra["loss_sum_bits"])
        best_auc = float(extra["best_auc"])
        history += [tuple(h) for h in extra["history"]]
        for k, v in lists.items():
            v += list(extra["lists"].get(k, []))          # a list added after the state was saved: empty
        train_loader.load_state_dict(extra["loader"], skip=start_steps)
        log0(f"Resumed from {resume} | Epoch {start_epoch + 1} | Step {start_steps} | "
             f"LR: {trainer.current_lr():.6f}")
    done_here, stopped = 0, False
    for epoch in range(start_epoch, n_epochs):
        t0 = time.perf_counter()
        total = torch.zeros((), dtype=torch.float64, device=device)
        steps = 0
        if epoch == start_epoch and start_steps:
            total.fill_(start_sum)
            steps = start_steps
        # one batch ahead: step() gets the following batch too, whose ids are routed (N > 1) and
        # whose table rows are caught up (lazy table Adam) during the current step
        it = iter(train_loader)
        cur = next(it, None)
        while cur is not None:
            nxt = next(it, None)
            batch, labels = cur
            loss = trainer.step(batch, labels, next_batch=nxt[0] if nxt is not None else None)
            cur = nxt
            total += loss[0].double()
            steps += 1
            if steps % 200 == 0:
                log0(f"Epoch {epoch + 1} | Step {steps} | Loss: {loss.item():.4f} | LR: {trainer.current_lr():.6f}")
                # the print's sync anyway: an item_id without item_info raises here, within 200
                # steps of the batch (the reference raises at that batch, src/dataloader.py:104-106)
                train_loader.check(world=world)
            done_here += 1
            stopped = max_steps is not None and done_here >= max_steps
            # mid-epoch state (the epoch's last step is saved after its validation, below)
            if saving and cur is not None and (stopped or (save_every and trainer.host_step % save_every == 0)):
                trainer.check_ids()
                train_loader.check(world=world)
                save_state(epoch, steps, float(total.item()))
            if stopped:
                break
        if stopped and cur is not None:
            log0(f"Stopped after {done_here} steps at Epoch {epoch + 1} | Step {steps}; state saved under {state_dir}")
            break
        trainer.check_ids()
        train_loader.check(world=world)
        avg_loss = float(total.item()) / steps if steps else 0.0
        dt = time.perf_counter() - t0
        # validation (:133-146): eval-mode probabilities of the whole split, packed and counted on the
        # device (metrics.DeviceMetrics: the exact AUC, the double utils.compute_auc returns on them)
        ev = trainer.evaluate(valid_loader, **ev_args)
        valid_loader.check(world=world)
        auc = logloss = None
        if len(valid_loader):
            auc, logloss = float(ev["auc"]), float(ev["logloss"])
        history.append((epoch + 1, avg_loss, auc))
        valid_logloss.append(logloss)
        line = (f"Epoch {epoch + 1} | Train Loss: {avg_loss:.4f} | Valid AUC: {auc if auc is None else round(auc, 4)} | "
                f"{steps * train_loader.batch_size / dt:.0f} samples/s | "
                f"Valid LogLoss: {logloss if logloss is None else round(logloss, 4)}")
        if group_by:
            gauc = float(ev["gauc"]) if len(valid_loader) else None
            valid_gauc.append(gauc)
            line += f" | Valid GAUC: {gauc if gauc is None else f'{gauc:.4f}'}"
        if calib_bins:
            ece, pcoc, ne = ((float(ev[k]) for k in ("ece", "pcoc", "ne")) if len(valid_loader) else (None,) * 3)
            valid_ece.append(ece)
            valid_pcoc.append(pcoc)
            valid_ne.append(ne)
            fmt = lambda v: v if v is None else f"{v:.4f}"            # noqa: E731
            line += f" | Valid ECE: {fmt(ece)} | PCOC: {fmt(pcoc)} | NE: {fmt(ne)}"
        if auc_ci:
            se = float(ev["auc_se"]) if len(valid_loader) else None
            valid_auc_se.append(se)
            line += f" | AUC SE: {se if se is None else f'{se:.4f}'}"
        iso = ev.get("calibrator") if fit_iso else None
        if fit_iso:
            valid_iso_blocks.append(None if iso is None else len(iso))
            line += f" | iso blocks: {None if iso is None else len(iso)}"
        log0(line)
        if auc is not None and auc > best_auc:
            best_auc = auc
            sd = trainer.state_dict()                     # collective at N > 1 (table on rank 0 only)
            if rank == 0:
                os.makedirs(os.path.dirname(os.path.abspath(ckpt)), exist_ok=True)
                torch.save(sd, ckpt)
                log0(f"New best FiBiNET AUC; saved to {ckpt}")
                if iso is not None:
                    iso.save(os.path.splitext(ckpt)[0] + ".isotonic.json")
        if saving:
            save_state(epoch + 1, 0, 0.0)
        if stopped:
            log0(f"Stopped after {done_here} steps at the end of Epoch {epoch + 1}; state saved under {state_dir}")
            break
    if not stopped:
        log0(f"Done. Best AUC: {best_auc:.4f}")
    out = {"best_auc": best_auc, "history": history, "valid_logloss": valid_logloss, "trainer": trainer}
    if stopped:
        out["stopped"] = True
    if group_by:
        out["valid_gauc"] = valid_gauc
    if calib_bins:
        out.update(valid_ece=valid_ece, valid_pcoc=valid_pcoc, valid_ne=valid_ne)
    if auc_ci:
        out["valid_auc_se"] = valid_auc_se
    if fit_iso:
        out["valid_iso_blocks"] = valid_iso_blocks
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config")
    ap.add_argument("--epochs", type=int)
    ap.add_argument("--checkpoint")
    ap.add_argument("--resume", metavar="DIR", help="continue the run whose full state was saved under DIR")
    ap.add_argument("--save-every", type=int, metavar="S", help="save the full training state every S optimizer steps")
    ap.add_argument("--state-dir", metavar="DIR", help="where the full-state checkpoints go")
    ap.add_argument("--max-steps", type=int, metavar="K", help="save the state and stop after K steps of this invocation")
    args = ap.parse_args(argv)
    out = run(args.config, epochs=args.epochs, checkpoint=args.checkpoint, resume=args.resume,
              save_every=args.save_every, state_dir=args.state_dir, max_steps=args.max_steps)
    out["trainer"].close()
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
