"""Full-state checkpoints: save a training run and resume it in a fresh process, bit for bit.

The reference saves the best-AUC weights only (src/train_fibinet.py:148-152; SURVEY.md: "no optimizer
or scheduler state, no resume").  Here ``FiBiNETTrainer.training_state()`` holds everything a later
step reads -- weights, Adam moments, the device step counter (the OneCycleLR position), the dropout
stream, BatchNorm buffers -- after a flush of the lazy table Adam, and this module puts it on disk:

    dir/step-00000123/rank0.pt           this rank's training state + the caller's ``extra``
    dir/step-00000123/rank0.digests.json its tensors' digests (what rank 0 compares across ranks)
    dir/step-00000123/manifest.json      step, world size, file names, every rank's digests
    dir/latest                           the name of the newest complete step directory

Every file is written under a temporary name and renamed; ``latest`` is replaced last, after the
manifest, so a save that dies half-way never becomes ``latest``.

Integrity is an order-independent 64-bit digest of each tensor's 32-bit words,
computed on the device by ``fbn_digest_u64`` (:func:`digest`: one launch, 8 bytes read back) and on
the host by :func:`digest_host` (numpy; the reference and the offline verifier):

    python -m ctr_recommendation_amd.checkpoint verify DIR

re-reads every shard of DIR's latest step on the CPU and prints one line per tensor (no GPU needed).
"""
from __future__ import annotations

import json
import os
import re
import shutil
import sys
from typing import Dict, Optional

import numpy as np
import torch

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
_STEP_DIR = re.compile(r"^step-(\d{8,})$")
REPLICATED = ("flat_p", "flat_m", "flat_v")     # equal on every rank of a healthy run


# ---------------------------------------------------------------------------------------- digests
def digest_host(a: np.ndarray, base: int = 0) -> int:
    """fbn_digest_u64 in numpy: sum over the 32-bit words w_i of a (C order) of
    mix64((base + i + 1) * 0x9E3779B97F4A7C15 + w_i) mod 2^64, mix64 the splitmix64 finaliser."""
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize % 4:
        raise ValueError(f"digest_host: element size {a.dtype.itemsize} is not a multiple of 4 bytes")
    w = a.reshape(-1).view(np.uint32)
    total = 0
    chunk = 1 << 22
    with np.errstate(over="ignore"):
        for lo in range(0, w.size, chunk):
            c = w[lo:lo + chunk].astype(np.uint64)
            first = (int(base) + lo + 1) & MASK64
            x = (np.arange(c.size, dtype=np.uint64) + np.uint64(first)) * np.uint64(GOLDEN) + c
            x ^= x >> np.uint64(30)
            x *= np.uint64(0xBF58476D1CE4E5B9)
            x ^= x >> np.uint64(27)
            x *= np.uint64(0x94D049BB133111EB)
            x ^= x >> np.uint64(31)
            total = (total + int(np.add.reduce(x, dtype=np.uint64))) & MASK64
    return total


def _words(t: torch.Tensor) -> int:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError("digest takes a device tensor (digest_host is the CPU form)")
    if not t.is_contiguous():
        raise ValueError("digest needs a contiguous tensor (a strided view has no single word sequence; "
                         "digest its base, or .contiguous() it)")
    if t.element_size() not in (4, 8):
        raise ValueError(f"digest needs 4- or 8-byte elements, not {t.dtype}")
    return t.numel() * t.element_size() // 4


def digest_add(out: torch.Tensor, t: torch.Tensor, base: int = 0) -> None:
    """Add t's digest (its first word at index `base`) to the device cell out (int64 [1])."""
    from . import _lib
    n = _words(t)
    if out.dtype != torch.int64 or out.numel() != 1 or out.device != t.device:
        raise ValueError("digest_add: out is one int64 on t's device")
    _lib.call("fbn_digest_u64", _lib.ptr(t) if n else None, n, int(base) & MASK64, _lib.ptr(out),
              _lib.stream_handle(t.device))


def digest(t: torch.Tensor, base: int = 0) -> int:
    """The digest of a contiguous device tensor of 4- or 8-byte elements: one launch, 8 bytes read."""
    _words(t)
    out = torch.zeros(1, dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        digest_add(out, t, base)
    return int(out.item()) & MASK64


def _host_digest_of(t: torch.Tensor) -> int:
    return digest_host(t.detach().cpu().contiguous().numpy())


# ---------------------------------------------------------------------------------------- files
def _atomic_write(path: str, write) -> None:
    tmp = f"{path}.tmp{os.getpid()}"
    write(tmp)
    os.replace(tmp, path)


def _write_json(path: str, obj) -> None:
    def w(tmp):
        with open(tmp, "w") as f:
            json.dump(obj, f, indent=1, sort_keys=True)
            f.flush()
            os.fsync(f.fileno())
    _atomic_write(path, w)


def _step_name(step: int) -> str:
    return f"step-{step:08d}"


def _step_dirs(root: str):
    """[(step, name)] of root's step directories, newest first."""
    out = []
    if os.path.isdir(root):
        for n in os.listdir(root):
            m = _STEP_DIR.match(n)
            if m and os.path.isdir(os.path.join(root, n)):
                out.append((int(m.group(1)), n))
    return sorted(out, reverse=True)


def _bn_names(digests: Dict[str, int]):
    return [k for k in digests if "running_" in k or "num_batches_tracked" in k]


def save(dir: str, trainer, extra: Optional[Dict] = None, keep: int = 2) -> str:
    """Write trainer.training_state() and `extra` (ints, floats, strings, lists, dicts and CPU tensors:
    what torch.load(weights_only=True) reads back) as dir/step-%08d/rank%d.pt; returns the step
    directory.  N > 1: every rank calls it (one barrier); rank 0 then compares the ranks' digests of the
    replicated dense state (and of the BatchNorm buffers under sync_bn) and raises RuntimeError
    ("replicas diverged: <tensor>") before anything becomes ``latest``."""
    state = trainer.training_state()
    meta = state["meta"]
    step, rank, world = int(meta["host_step"]), int(meta["rank"]), int(meta["world"])
    sdir = os.path.join(dir, _step_name(step))
    os.makedirs(sdir, exist_ok=True)
    digests = {k: int(v) for k, v in state["digests"].items()}
    _atomic_write(os.path.join(sdir, f"rank{rank}.pt"),
                  lambda tmp: torch.save({"state": state, "extra": extra if extra is not None else {}}, tmp))
    _write_json(os.path.join(sdir, f"rank{rank}.digests.json"), {k: f"{v:016x}" for k, v in digests.items()})
    if world > 1:
        import torch.distributed as dist
        dist.barrier(group=getattr(trainer, "group", None))
    if rank != 0:
        return sdir
    per_rank = {}
    for r in range(world):
        with open(os.path.join(sdir, f"rank{r}.digests.json")) as f:
            per_rank[r] = json.load(f)
    same = list(REPLICATED) + (_bn_names(digests) if meta.get("sync_bn", True) else [])
    for r in range(1, world):
        for name in same:
            if per_rank[r].get(name) != per_rank[0].get(name):
                raise RuntimeError(f"replicas diverged: {name} (rank {r} {per_rank[r].get(name)} vs rank 0 "
                                   f"{per_rank[0].get(name)} at step {step}); nothing was made latest")
    _write_json(os.path.join(sdir, "manifest.json"),
                {"step": step, "world": world, "files": [f"rank{r}.pt" for r in range(world)],
                 "digests": {str(r): per_rank[r] for r in range(world)}})
    _atomic_write(os.path.join(dir, "latest"), lambda tmp: open(tmp, "w").write(_step_name(step) + "\n"))
    for _, name in _step_dirs(dir)[max(1, int(keep)):]:
        shutil.rmtree(os.path.join(dir, name), ignore_errors=True)
    return sdir


def _complete(root: str, name: str, rank: int) -> bool:
    d = os.path.join(root, name)
    return os.path.exists(os.path.join(d, "manifest.json")) and os.path.exists(os.path.join(d, f"rank{rank}.pt"))


def find(dir: str, rank: int = 0) -> str:
    """The step directory load() reads: ``latest``'s when its manifest and this rank's shard exist, else
    the newest step directory where both do."""
    cands = []
    latest = os.path.join(dir, "latest")
    if os.path.exists(latest):
        name = open(latest).read().strip()
        if _STEP_DIR.match(name):
            cands.append(name)
    cands += [n for _, n in _step_dirs(dir) if n not in cands]
    for name in cands:
        if _complete(dir, name, rank):
            return os.path.join(dir, name)
    raise FileNotFoundError(f"no complete checkpoint (manifest.json + rank{rank}.pt) under {dir!r}")


def load(dir: str, trainer) -> Dict:
    """Load this rank's shard of dir's newest complete step into `trainer` (load_training_state: meta
    checked, tensors copied in place, digests re-checked on the device); returns the saved `extra`."""
    sdir = find(dir, int(getattr(trainer, "rank", 0)))
    blob = torch.load(os.path.join(sdir, f"rank{int(getattr(trainer, 'rank', 0))}.pt"), map_location="cpu",
                      weights_only=True)
    trainer.load_training_state(blob["state"])
    return blob["extra"]


def verify(dir: str, out=print) -> int:
    """Re-read every shard of dir's newest complete step on the CPU and compare digest_host of each
    tensor with the digest saved beside it and the manifest's; one line per tensor.  Returns the number
    of mismatches (0: intact)."""
    sdir = find(dir, 0)
    with open(os.path.join(sdir, "manifest.json")) as f:
        man = json.load(f)
    bad = 0
    for r, fname in enumerate(man["files"]):
        path = os.path.join(sdir, fname)
        if not os.path.exists(path):
            out(f"{os.path.basename(sdir)} rank{r} {fname} MISSING")
            bad += 1
            continue
        state = torch.load(path, map_location="cpu", weights_only=True)["state"]
        for name, want in sorted(state["digests"].items()):
            got = _host_digest_of(state[name])
            listed = man["digests"].get(str(r), {}).get(name)
            ok = got == int(want) and listed == f"{got:016x}"
            bad += not ok
            out(f"{os.path.basename(sdir)} rank{r} {name} {got:016x} {'OK' if ok else 'MISMATCH'}"
                + ("" if ok else f" (saved {int(want):016x}, manifest {listed})"))
    return bad


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) != 2 or argv[0] != "verify":
        print("usage: python -m ctr_recommendation_amd.checkpoint verify DIR", file=sys.stderr)
        return 2
    return 1 if verify(argv[1]) else 0


if __name__ == "__main__":
    sys.exit(main())
