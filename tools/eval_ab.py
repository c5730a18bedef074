"""Validation on the device vs on the host, timed in one process (not part of bench.py).

A synthetic 1 M-row validation split at d = 128, batch 8192 (HBM-resident batches, the last one
short), an untrained FiBiNETTrainer:
  (a) host_loop_ms   the launcher's former loop: predict().cpu().numpy() per batch + utils.compute_auc
  (b) evaluate_ms    FiBiNETTrainer.evaluate(): pack per batch, one device reduce, one 40-byte read
  (c) reduce_ms      fbn_eval_reduce alone on the split's keys
  (d) sort_ms        torch.sort of the same key tensor (what a sort-based AUC would have to beat)
plus (c) on uniform random scores (reduce_uniform_ms: keys spread over every bucket, the counting
scheme's least favourable input).  Each figure is the median of RUNS timed runs after a warm-up:
HIP events around device-only work, perf_counter around the host loops (which end in a synchronise).

    python tools/eval_ab.py [--rows 1000000] [--out profiles/eval_device_vs_host.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ctr_recommendation_amd import _lib
from ctr_recommendation_amd.data import make_device_batches
from ctr_recommendation_amd.metrics import DeviceMetrics
from ctr_recommendation_amd.trainer import FiBiNETTrainer
from ctr_recommendation_amd.utils import compute_auc

RUNS = 5


def _host_ms(fn):
    fn()                                                    # warm-up
    out = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), r


def _device_ms(fn):
    fn()
    out = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=1_250_000)
    ap.add_argument("--out", default=os.path.join("profiles", "eval_device_vs_host.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, L = args.batch, 20
    full, rest = divmod(args.rows, B)
    batches = make_device_batches(full, B, args.vocab, L, dev, seed=11)
    if rest:
        batches += make_device_batches(1, rest, args.vocab, L, dev, seed=12)
    cfg = {"embedding_dim": args.d, "vocab_size": args.vocab, "compute_dtype": "bf16"}
    tr = FiBiNETTrainer(cfg, total_steps=10, batch_size=B, device=dev, seed=7)

    def host_loop():
        ys, ps = [], []
        for batch, labels in batches:
            ps.append(tr.predict(batch).cpu().numpy())
            ys.append(labels.cpu().numpy())
        return float(compute_auc(np.concatenate(ys), np.concatenate(ps)))

    host_ms, auc_host = _host_ms(host_loop)
    eval_ms, ev = _host_ms(lambda: tr.evaluate(batches))
    assert ev["auc"] == auc_host and ev["n"] == args.rows, (ev, auc_host)

    m = tr._eval_metrics                                    # the split's keys, as evaluate() left them
    n = m.count
    rec = torch.zeros(5, dtype=torch.int64, device=dev)
    ws = m._workspace(n)

    def reduce(keys):
        _lib.call("fbn_eval_reduce", keys.data_ptr(), n, ws.data_ptr(), ws.numel(), rec.data_ptr(), rec.data_ptr() + 32,
                  _lib.stream_handle(dev))

    keys = m.keys[:n]
    reduce_ms = _device_ms(lambda: reduce(keys))
    sort_ms = _device_ms(lambda: torch.sort(keys))
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    um = DeviceMetrics(n, dev)
    um.update(torch.rand(n, generator=g, device=dev), (torch.rand(n, generator=g, device=dev) < 0.17).float())
    ukeys = um.keys[:n]
    reduce_uniform_ms = _device_ms(lambda: reduce(ukeys))
    sort_uniform_ms = _device_ms(lambda: torch.sort(ukeys))
    out = {"device": torch.cuda.get_device_name(dev), "rows": args.rows, "batch": B, "d": args.d, "runs": RUNS,
           "statistic": "median", "host_loop_ms": round(host_ms, 3), "evaluate_ms": round(eval_ms, 3),
           "reduce_ms": round(reduce_ms, 4), "sort_ms": round(sort_ms, 4),
           "reduce_uniform_ms": round(reduce_uniform_ms, 4), "sort_uniform_ms": round(sort_uniform_ms, 4),
           "auc": ev["auc"], "logloss": ev["logloss"], "auc_equal_host": True}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
