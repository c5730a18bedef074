"""Calibration metrics on the device vs on the host, timed in one process (not part of bench.py).

A synthetic 1 M-row validation split at d = 128, bf16, batch 8192 (HBM-resident batches, the last one
short), an untrained FiBiNETTrainer:
  (a) host_loop_ms        what a user had to write: predict().cpu() per batch, labels to the host, then
                          numpy binning there (equal-width and equal-mass reliability tables, ECE, PCOC, Brier)
  (b) evaluate_calib_ms   FiBiNETTrainer.evaluate(calibration_bins=10)
  (c) evaluate_ms         FiBiNETTrainer.evaluate() without calibration
  (d) calib_reduce_ms     fbn_calib_reduce alone on the split's keys
Each figure is the median of RUNS timed runs after a warm-up: HIP events around device-only work,
perf_counter around the host loops (which end in a synchronise).  (b)'s table must equal (a)'s.

    python tools/calibration_ab.py [--rows 1000000] [--bins 10] [--out profiles/calibration_device_vs_host.json]
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
from ctr_recommendation_amd.trainer import FiBiNETTrainer

RUNS = 5
COLS = ("n", "n_pos", "sum_p", "sum_p_pos", "sum_p2")


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


def host_tables(y, p, bins):
    """Both planes with numpy on the host, in the device's definitions (float64 bin rule, ranks of the sorted
    keys, 2^32 fixed point), so that the tables can be compared exactly.  The sums stay below 2^63 / 2^32 =
    2^31 samples, so int64 holds them."""
    p = p.astype(np.float32)
    bits = np.where(p == 0, np.uint32(0), p.view(np.uint32)).astype(np.uint32)
    key = np.sort((bits << np.uint32(1)) | (y == 1).astype(np.uint32))
    n = len(key)
    pd = (key >> np.uint32(1)).astype(np.uint32).view(np.float32).astype(np.float64)
    pos = (key & np.uint32(1)).astype(np.int64)
    fx = np.rint(pd * 2.0 ** 32).astype(np.int64)
    fx2 = np.rint(pd * pd * 2.0 ** 32).astype(np.int64)
    cum = [np.r_[0, np.cumsum(v)] for v in (pos, fx, fx * pos, fx2)]
    wb = np.minimum(bins - 1, np.floor(pd * bins).astype(np.int64))
    wbounds = np.searchsorted(wb, np.arange(bins + 1), side="left")
    wbounds[bins] = n
    mbounds = (np.arange(bins + 1, dtype=np.int64) * n) // bins
    out = {}
    for name, bd in (("width", wbounds), ("mass", mbounds)):
        plane = {"n": np.diff(bd).astype(np.int64)}
        for c, v in zip(COLS[1:], cum):
            plane[c] = (v[bd[1:]] - v[bd[:-1]]).astype(np.int64)
        out[name] = plane
    n_pos = int(pos.sum())
    gap = np.abs(out["width"]["n_pos"] * 2.0 ** 32 - out["width"]["sum_p"])
    out["ece"] = float(gap.sum() / (n * 2.0 ** 32))
    out["pcoc"] = float(fx.sum() / (n_pos * 2.0 ** 32)) if n_pos else float("nan")
    out["brier"] = float((fx2.sum() - 2 * (fx * pos).sum() + n_pos * 2.0 ** 32) / (n * 2.0 ** 32))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--bins", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=1_250_000)
    ap.add_argument("--out", default=os.path.join("profiles", "calibration_device_vs_host.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, L, bins = args.batch, 20, args.bins
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
        return host_tables(np.concatenate(ys), np.concatenate(ps), bins)

    host_ms, host = _host_ms(host_loop)
    calib_ms, ev = _host_ms(lambda: tr.evaluate(batches, calibration_bins=bins))
    cal = ev["calibration"]
    assert ev["n"] == args.rows
    for plane in ("width", "mass"):
        for c in COLS:
            assert np.array_equal(cal[plane][c], host[plane][c]), f"{plane}.{c} differs from the host table"
    assert abs(ev["ece"] - host["ece"]) <= 1e-12 and abs(ev["brier"] - host["brier"]) <= 1e-12
    m = tr._eval_metrics                                    # the split's keys, as evaluate() left them
    n = m.count
    keys = m.keys[:n].clone()
    plain_ms, ev_plain = _host_ms(lambda: tr.evaluate(batches))
    assert ev_plain["auc"] == ev["auc"] and ev_plain["logloss"] == ev["logloss"]

    status = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.call("fbn_calib_workspace_size", n)), dtype=torch.uint8, device=dev)
    tab = torch.empty(2 * bins * _lib.FBN_CALIB_BIN_WORDS + 1, dtype=torch.int64, device=dev)
    reduce_ms = _device_ms(lambda: _lib.call("fbn_calib_reduce", keys.data_ptr(), n, bins, ws.data_ptr(), ws.numel(),
                                             tab.data_ptr(), status.data_ptr(), _lib.stream_handle(dev)))
    out = {"device": torch.cuda.get_device_name(dev), "rows": args.rows, "bins": bins, "batch": B, "d": args.d,
           "runs": RUNS, "statistic": "median", "host_loop_ms": round(host_ms, 3), "evaluate_calib_ms": round(calib_ms, 3),
           "evaluate_ms": round(plain_ms, 3), "calibration_cost_ms": round(calib_ms - plain_ms, 3),
           "calib_reduce_ms": round(reduce_ms, 4), "ece": ev["ece"], "mce": ev["mce"], "ece_mass": ev["ece_mass"],
           "pcoc": ev["pcoc"], "brier": ev["brier"], "ne": ev["ne"], "auc": ev["auc"], "table_equal_host": True}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
