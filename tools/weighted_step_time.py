"""Step time of the C3 training step (d 128, V 1.25 M, B 8192, bf16, step programs) with and without
the weighted loss: one trainer per arm in one process, every batch's step recorded once and then
replayed in order, the arms timed in alternating blocks of whole program cycles at steady state.
Prints one JSON line: per arm the ms/step of every block, their median, min and max.

  python tools/weighted_step_time.py                      # arms: plain, weighted
  python tools/weighted_step_time.py --arms plain --tree /path/to/another/checkout
      (the plain arm uses nothing this feature added, so it also times a checkout without it: the
       run-to-run spread of the unweighted step, and the comparison against it)"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--arms", default="plain,weighted")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--cycles", type=int, default=3, help="program cycles (of --batches steps) per timed block")
ap.add_argument("--batches", type=int, default=160)
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, args.tree)
import torch

from ctr_recommendation_amd.data import make_device_batches
from ctr_recommendation_amd.trainer import FiBiNETTrainer

dev = torch.device("cuda", 0)
V, B, nb, R = 1_250_000, 8192, args.batches, args.rounds
K = args.cycles * nb
cfg = {"embedding_dim": 128, "vocab_size": V, "compute_dtype": "bf16"}
batches = make_device_batches(nb, B, V, 20, dev, seed=2025)
# down-sampling weights: every negative as if kept at rate 1/4 (weight 4), positives at 1
wbatches = [(dict(b, sample_weight=torch.where(y > 0, 1.0, 4.0).float().contiguous()), y) for b, y in batches]
arms = {}
for name in args.arms.split(","):
    kw = {"pos_weight": 2.0, "label_smoothing": 0.05} if name == "weighted" else {}
    tr = FiBiNETTrainer(cfg, total_steps=2 + 2 * nb + (R + 1) * K, batch_size=B, device=dev, **kw)
    data = wbatches if name == "weighted" else batches
    tr.step(*data[-1], next_batch=data[0][0])            # prefetches (and pre-claims) batch 0 for the first recording
    pool = torch.cuda.MemPool()
    progs = [tr.record_program(data[j][0], data[j][1], next_batch=data[(j + 1) % nb][0], pool=pool) for j in range(nb)]
    arms[name] = (tr, progs)


def replay(name, n):
    tr, progs = arms[name]
    for k in range(n):
        tr.run_program(progs[k % nb])


for name in arms:                                         # steady state of the lazy table Adam (~2 F steps)
    replay(name, nb)
torch.cuda.synchronize()
res = {name: [] for name in arms}
for _ in range(R):
    for name in arms:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        replay(name, K)
        torch.cuda.synchronize()
        res[name].append((time.perf_counter() - t0) / K * 1e3)
out = {"label": args.label, "tree": args.tree, "B": B, "d": 128, "V": V, "steps_per_block": K, "rounds": R, "arms": {}}
for name, v in res.items():
    tr, progs = arms[name]
    tr.check_ids()
    s = sorted(v)
    names = getattr(progs[0], "names", None)
    out["arms"][name] = {"ms_per_step": [round(x, 5) for x in v], "median": round(s[len(s) // 2], 5),
                         "min": round(s[0], 5), "max": round(s[-1], 5), "loss": float(tr.loss.item()),
                         "weighted_head_calls": None if names is None else sum(n.endswith("_w") for n in names)}
print(json.dumps(out))
