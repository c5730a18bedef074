"""Validation AUC and log-loss computed on the device, exactly (csrc/metrics.hip).

The reference's validation (src/train_fibinet.py:133-146) copies every batch's probabilities to the
host and runs roc_auc_score / log_loss there (src/utils.py:18-32).  :class:`DeviceMetrics` keeps one
uint32 key per sample on the device -- ``(bits(p) << 1) | y`` for an fp32 probability p in [0, 1] --
and counts: the AUC is ``U2 / (2 n_pos n_neg)`` with U2 an exact integer (Python int / int: correctly
rounded), the same double ``utils.compute_auc`` returns on the same fp32 probabilities while
``n_pos * n_neg < 2^53``; the log-loss is ``utils.compute_logloss``'s float64 expression summed as a
fixed-shape tree (bitwise reproducible for the same sample sequence).

    m = DeviceMetrics(capacity=len(valid_rows), device="cuda")
    for batch, labels in valid_batches:
        m.update(model(batch), labels)          # one launch, no host sync
    out = m.compute()                           # {"auc", "logloss", "n", "n_pos"}: one 40-byte read
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import call

_STATUS = ((1, "a probability is NaN"),
           (2, "a probability lies outside [0, 1]"),
           (4, "a label is neither 0.0 nor 1.0"),
           (8, "a key was not written by fbn_eval_pack (score bits above 1.0)"))
_MAX_N = (1 << 31) - 1


class DeviceMetrics:
    """Streaming exact ROC-AUC + log-loss of up to ``capacity`` samples held as keys on ``device``."""

    def __init__(self, capacity: int, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("DeviceMetrics runs on a HIP device only (no CPU fallback)")
        capacity = int(capacity)
        if not 0 <= capacity <= _MAX_N:
            raise ValueError(f"capacity must be in [0, 2^31), not {capacity}")
        self.capacity = capacity
        # keys are below 2^31 (score bits < 2^30), so the int32 view orders as the uint32 keys do
        self.keys = torch.empty(max(1, capacity), dtype=torch.int32, device=self.device)
        # {u64 U2, u64 n_pos, u64 n_neg, f64 logloss_sum} + the status word: read back in one copy
        self.rec = torch.zeros(5, dtype=torch.int64, device=self.device)
        self.count = 0
        self._ws: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ streaming
    def reset(self) -> None:
        self.count = 0
        self.rec.zero_()

    def update(self, probs: torch.Tensor, labels: torch.Tensor) -> None:
        """Append a batch: one pack launch, no host sync (bad values surface in compute())."""
        _lib.require_hip(probs, "probs")
        _lib.require_hip(labels, "labels")
        n = probs.numel()
        if labels.numel() != n:
            raise ValueError(f"probs has {n} elements, labels {labels.numel()}")
        if self.count + n > self.capacity:
            raise ValueError(f"DeviceMetrics capacity {self.capacity} exceeded ({self.count} held + {n} new)")
        if n == 0:
            return
        p = probs.detach().reshape(-1).to(torch.float32).contiguous()
        y = labels.detach().reshape(-1).to(torch.float32).contiguous()
        with torch.cuda.device(self.device):
            call("fbn_eval_pack", p.data_ptr(), y.data_ptr(), n, self.keys.data_ptr() + 4 * self.count,
                 self.rec.data_ptr() + 32, _lib.stream_handle(self.device))
        self.count += n

    # ------------------------------------------------------------------ result
    def _workspace(self, n: int) -> torch.Tensor:
        need = int(call("fbn_eval_workspace_size", n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _reduce(self, keys: torch.Tensor, n: int, rec: torch.Tensor) -> Dict:
        ws = self._workspace(n)
        with torch.cuda.device(self.device):
            call("fbn_eval_reduce", keys.data_ptr(), n, ws.data_ptr(), ws.numel(), rec.data_ptr(),
                 rec.data_ptr() + 32, _lib.stream_handle(self.device))
        host = rec.cpu().numpy()                 # the one device-to-host read: record + status
        status = int(host[4]) & 0xFFFFFFFF
        if status:
            raise ValueError("DeviceMetrics: " + "; ".join(msg for bit, msg in _STATUS if status & bit))
        u2, n_pos, n_neg = int(host[0]), int(host[1]), int(host[2])
        ll_sum = float(host[3:4].view(np.float64)[0])
        total = n_pos + n_neg
        auc = 0.5 if n_pos == 0 or n_neg == 0 else u2 / (2 * n_pos * n_neg)
        return {"auc": auc, "logloss": ll_sum / total if total else float("nan"), "n": total, "n_pos": n_pos}

    def compute(self, group=None, stage_on_cpu: bool = False) -> Dict:
        """{"auc", "logloss", "n", "n_pos"} of the samples held (they stay: compute() can be repeated).

        group: a torch.distributed process group -- collective; every rank's keys are all-gathered
        (4 B per sample, padded to the largest count) and reduced on every rank, in rank-major order:
        key order does not enter the AUC and the log-loss tree sees the same sequence everywhere, so
        all ranks return identical numbers.  stage_on_cpu: gather through host tensors (gloo)."""
        if group is None:
            return self._reduce(self.keys, self.count, self.rec)
        import torch.distributed as dist
        world = dist.get_world_size(group)
        counts = [None] * world
        dist.all_gather_object(counts, int(self.count), group=group)     # host-side ints
        maxc, total = max(counts), sum(counts)
        if total > _MAX_N:
            raise ValueError(f"{total} samples over the group: the device reduce needs n < 2^31")
        # one buffer per rank: its keys, padding, and its status word in the last slot
        send = torch.zeros(maxc + 1, dtype=torch.int32, device=self.device)
        send[:self.count] = self.keys[:self.count]
        send[maxc:] = self.rec.view(torch.int32)[8:9]
        if stage_on_cpu:
            parts = [torch.empty(maxc + 1, dtype=torch.int32) for _ in range(world)]
            dist.all_gather(parts, send.cpu(), group=group)
            got = torch.stack(parts).to(self.device)
        else:
            got = torch.empty((world, maxc + 1), dtype=torch.int32, device=self.device)
            dist.all_gather_into_tensor(got.view(-1), send, group=group)
        keys = torch.cat([got[r, :counts[r]] for r in range(world)]) if total else self.keys[:0]
        rec = torch.zeros(5, dtype=torch.int64, device=self.device)
        status = got[0, maxc:].clone()
        for r in range(1, world):
            status |= got[r, maxc:]
        rec.view(torch.int32)[8:9] = status
        return self._reduce(keys.contiguous(), total, rec)
