"""DeLong standard errors on the device vs on the host, timed in one process (not part of bench.py).

Two synthetic score sets over the same 1 M labels (CTR-shaped: scores piled up near 0.03, 4 % positives; the
second set is the first plus noise, rounded so that it ties), held as fp32 device tensors -- what a
validation pass leaves behind:
  (a) auc_ci_ms        DeviceMetrics.auc_ci(): one placement pass (sort, scan, search), one reduce, one read
  (b) compare_auc_ms   metrics.compare_auc(): two placement passes, three reduces, one read
  (c) host_ci_ms       what a user had to write: the probabilities copied to the host (the copy included),
                       then the same integers with numpy (searchsorted per class) and Python integers
  (d) host_compare_ms  the same for the paired test (both sets copied)
  (e) place_ms / reduce_ms   fbn_auc_place and fbn_delong_reduce alone, HIP events
Each figure is the median of RUNS timed runs after a warm-up: HIP events around device-only work,
perf_counter around what ends in a host read.  The integer records of (a) / (b) must equal (c) / (d)'s.

    python tools/delong_ab.py [--rows 1000000] [--out profiles/delong_device_vs_host.json]
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
from ctr_recommendation_amd.metrics import DeviceMetrics, compare_auc, delong_from_record

RUNS = 5
MASK32 = (1 << 32) - 1


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


def host_placements(pos, p):
    sp, sn = np.sort(p[pos]), np.sort(p[~pos])
    out = np.empty(len(p), dtype=np.int64)
    lo, hi = np.searchsorted(sn, p[pos], "left"), np.searchsorted(sn, p[pos], "right")
    out[pos] = lo + hi
    lo, hi = np.searchsorted(sp, p[~pos], "left"), np.searchsorted(sp, p[~pos], "right")
    out[~pos] = 2 * len(sp) - hi - lo
    return out


def host_record(pos, a, b):
    """fbn_delong_reduce's 8 words from two placement arrays: the products' 32-bit halves summed in uint64
    (each sum stays below 2^63), the totals as Python integers."""
    prod = a.astype(np.uint64) * b.astype(np.uint64)        # placements are below 2^32: no wrap
    lo, hi = prod & np.uint64(MASK32), prod >> np.uint64(32)
    return [int(pos.sum()), int((~pos).sum()), int(a[pos].sum()), int(b[pos].sum()),
            int(lo[pos].sum()), int(hi[pos].sum()), int(lo[~pos].sum()), int(hi[~pos].sum())]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join("profiles", "delong_device_vs_host.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.rows
    rng = np.random.default_rng(23)
    p1 = rng.beta(2.0, 60.0, n).astype(np.float32)
    y = (rng.random(n) < np.minimum(1.0, 1.3 * p1.astype(np.float64))).astype(np.float32)
    p2 = np.round(np.clip(p1.astype(np.float64) + rng.normal(0.0, 0.01, n), 0.0, 1.0), 4).astype(np.float32)
    yd, pd1, pd2 = (torch.from_numpy(v).to(dev) for v in (y, p1, p2))
    ma, mb = DeviceMetrics(n, dev), DeviceMetrics(n, dev)
    ma.update(pd1, yd)
    mb.update(pd2, yd)

    def host_ci():
        pos = yd.cpu().numpy() == 1
        a = host_placements(pos, pd1.cpu().numpy())
        rec = host_record(pos, a, a)
        return rec, delong_from_record(rec)

    def host_compare():
        pos = yd.cpu().numpy() == 1
        a, b = host_placements(pos, pd1.cpu().numpy()), host_placements(pos, pd2.cpu().numpy())
        recs = {"aa": host_record(pos, a, a), "bb": host_record(pos, b, b), "ab": host_record(pos, a, b)}
        return recs, delong_from_record(recs["aa"], recs["bb"], recs["ab"])

    ci_ms, ci = _host_ms(ma.auc_ci)
    cmp_ms, cmp_ = _host_ms(lambda: compare_auc(ma, mb))
    host_ci_ms, (hrec, hci) = _host_ms(host_ci)
    host_cmp_ms, (hrecs, hcmp) = _host_ms(host_compare)
    equal = ci["record"] == hrec and cmp_["records"] == hrecs
    assert equal, "the device's integer records differ from the host's"
    assert ci["auc_se"] == hci["auc_se"] and cmp_["p_value"] == hcmp["p_value"]

    status = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.call("fbn_auc_place_workspace_size", n)), dtype=torch.uint8, device=dev)
    place = torch.empty(n, dtype=torch.int32, device=dev)
    rec = torch.empty(_lib.FBN_DELONG_REC_WORDS + 1, dtype=torch.int64, device=dev)
    keys = ma.keys[:n]
    place_ms = _device_ms(lambda: _lib.call("fbn_auc_place", keys.data_ptr(), n, ws.data_ptr(), ws.numel(), place.data_ptr(),
                                            status.data_ptr(), _lib.stream_handle(dev)))
    reduce_ms = _device_ms(lambda: _lib.call("fbn_delong_reduce", keys.data_ptr(), place.data_ptr(), keys.data_ptr(),
                                             place.data_ptr(), n, rec.data_ptr(), status.data_ptr(), _lib.stream_handle(dev)))
    assert [int(v) for v in rec.cpu().numpy()[:-1]] == hrec and int(status[0].item()) == 0
    out = {"device": torch.cuda.get_device_name(dev), "rows": n, "n_pos": ci["n_pos"], "runs": RUNS, "statistic": "median",
           "auc_ci_ms": round(ci_ms, 3), "compare_auc_ms": round(cmp_ms, 3), "host_ci_ms": round(host_ci_ms, 3),
           "host_compare_ms": round(host_cmp_ms, 3), "place_ms": round(place_ms, 4), "reduce_ms": round(reduce_ms, 4),
           "auc": ci["auc"], "auc_se": ci["auc_se"], "ci_lo": ci["ci_lo"], "ci_hi": ci["ci_hi"], "auc_b": cmp_["auc_b"],
           "delta": cmp_["delta"], "delta_se": cmp_["delta_se"], "z": cmp_["z"], "p_value": cmp_["p_value"],
           "records_equal_host": equal}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
