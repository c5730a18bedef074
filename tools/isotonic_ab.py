"""The isotonic calibrator on the device vs on the host, timed in one process (not part of bench.py).

A synthetic 1 M-row validation split at d = 128, bf16, batch 8192 (HBM-resident batches, the last one
short), an untrained FiBiNETTrainer:
  (a) host_loop_ms         what a user had to write: predict().cpu() per batch, labels to the host, then
                           sklearn's IsotonicRegression.fit there (the integer PAV of tests/_isotonic_ref.py
                           where sklearn is missing)
  (b) evaluate_iso_ms      FiBiNETTrainer.evaluate(fit_isotonic=True)
  (c) evaluate_ms          FiBiNETTrainer.evaluate()
  (d) fit_ms               fbn_isotonic_fit alone on the split's keys; fit_ctr_ms on the tests' `ctr` family at the
                           same rows (every score distinct, as a trained fp32 model gives: a full tile of points
                           per 1024 samples); fit_adversarial_ms on farey_repeat(16, r) sized to the same rows
                           (every group a hull vertex of its piece) and fit_distinct_ms on distinct_blocks(170)
                           (every score distinct AND thousands of vertices up to the last merge level);
                           calib_reduce_ms = fbn_calib_reduce on the split's keys, the yardstick (the same widen
                           and sort, no hull); sort_ms = fbn_sort_u64 alone on the split's widened keys, and
                           hull_over_sort = (fit_ms - sort_ms) / sort_ms: everything the fit adds to the sort
  (e) apply_ms             fbn_isotonic_apply on the split's scores, against its 8 B / sample traffic floor
Each figure is the median of RUNS timed runs after a warm-up: HIP events around device-only work,
perf_counter around the host loops (which end in a synchronise).  (b)'s blocks must equal the host PAV's
as integers.

    python tools/isotonic_ab.py [--rows 1000000] [--out profiles/isotonic_device_vs_host.json]
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
from tests import _isotonic_ref as R

RUNS = 5
HBM_GBS = 8000.0                                            # MI355X peak HBM bandwidth, for the apply kernel's floor


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


def _fit_alone(keys, n, dev):
    """(median ms, K) of fbn_isotonic_fit on keys[:n]."""
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.call("fbn_isotonic_workspace_size", n)), dtype=torch.uint8, device=dev)
    words = 2 * int(_lib.lib().fbn_isotonic_max_blocks(n)) + 2
    tab = torch.empty(words, dtype=torch.int64, device=dev)
    ms = _device_ms(lambda: _lib.call("fbn_isotonic_fit", keys.data_ptr(), n, ws.data_ptr(), ws.numel(), tab.data_ptr(),
                                      words, status.data_ptr(), _lib.stream_handle(dev)))
    return ms, int(tab[0].item())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=1_250_000)
    ap.add_argument("--out", default=os.path.join("profiles", "isotonic_device_vs_host.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, L = args.batch, 20
    full, rest = divmod(args.rows, B)
    batches = make_device_batches(full, B, args.vocab, L, dev, seed=11)
    if rest:
        batches += make_device_batches(1, rest, args.vocab, L, dev, seed=12)
    cfg = {"embedding_dim": args.d, "vocab_size": args.vocab, "compute_dtype": "bf16"}
    tr = FiBiNETTrainer(cfg, total_steps=10, batch_size=B, device=dev, seed=7)
    try:
        from sklearn.isotonic import IsotonicRegression
        host_fit = "sklearn"
    except ImportError:
        IsotonicRegression, host_fit = None, "integer PAV (tests/_isotonic_ref.py)"

    def host_loop():
        ys, ps = [], []
        for batch, labels in batches:
            ps.append(tr.predict(batch).cpu().numpy())
            ys.append(labels.cpu().numpy())
        y, p = np.concatenate(ys), np.concatenate(ps)
        if IsotonicRegression is not None:
            IsotonicRegression(out_of_bounds="clip").fit(p.astype(np.float64), y.astype(np.float64))
        else:
            R.fit_ref(y, p)
        return y, p

    host_ms, (y, p) = _host_ms(host_loop)
    iso_ms, ev = _host_ms(lambda: tr.evaluate(batches, fit_isotonic=True))
    cal = ev["calibrator"]
    assert ev["n"] == args.rows
    ref = R.fit_ref(y, p)
    assert R.same_blocks(cal.blocks, ref) is None, "the device blocks differ from the host PAV's"
    m = tr._eval_metrics                                    # the split's keys, as evaluate() left them
    n = m.count
    keys = m.keys[:n].clone()
    plain_ms, ev_plain = _host_ms(lambda: tr.evaluate(batches))
    assert ev_plain["auc"] == ev["auc"] and ev_plain["logloss"] == ev["logloss"]

    fit_ms, K = _fit_alone(keys, n, dev)
    assert K == len(cal)
    pieces = max(1, args.rows // sum(b for _, b in R.farey_sequence(16)))
    ya, pa = R.scores(f"farey_repeat:16,{pieces}")
    keys_a = torch.from_numpy(R.keys_of(ya, pa).view(np.int32)).to(dev)
    adv_ms, K_adv = _fit_alone(keys_a, len(ya), dev)
    assert K_adv == len(R.fit_ref(ya, pa)["n"])
    extra = {}
    for name, fam, arg in (("ctr", "ctr", min(args.rows, n)), ("distinct", "distinct_blocks:170", None)):
        ye, pe = R.scores(fam, arg)
        ke = torch.from_numpy(R.keys_of(ye, pe).view(np.int32)).to(dev)
        ms, Ke = _fit_alone(ke, len(ye), dev)
        assert Ke == len(R.fit_ref(ye, pe)["n"]), name
        extra.update({f"{name}_rows": len(ye), f"fit_{name}_ms": round(ms, 4), f"blocks_{name}": Ke,
                      f"groups_{name}": len(np.unique(pe))})
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    cws = torch.empty(int(_lib.call("fbn_calib_workspace_size", n)), dtype=torch.uint8, device=dev)
    ctab = torch.empty(2 * 10 * _lib.FBN_CALIB_BIN_WORDS + 1, dtype=torch.int64, device=dev)
    reduce_ms = _device_ms(lambda: _lib.call("fbn_calib_reduce", keys.data_ptr(), n, 10, cws.data_ptr(), cws.numel(),
                                             ctab.data_ptr(), status.data_ptr(), _lib.stream_handle(dev)))
    reduce_adv_ms = _device_ms(lambda: _lib.call("fbn_calib_reduce", keys_a.data_ptr(), len(ya), 10, cws.data_ptr(), cws.numel(),
                                                 ctab.data_ptr(), status.data_ptr(), _lib.stream_handle(dev))) if len(ya) <= n else None
    wide = keys.to(torch.int64)                             # the sort the fit and the reduce share, alone
    sorted_ = torch.empty_like(wide)
    sws = torch.empty(int(_lib.call("fbn_sort_u64_workspace_size", n)), dtype=torch.uint8, device=dev)
    sort_ms = _device_ms(lambda: _lib.call("fbn_sort_u64", wide.data_ptr(), n, 31, sws.data_ptr(), sws.numel(),
                                           sorted_.data_ptr(), _lib.stream_handle(dev)))
    extra.update(sort_ms=round(sort_ms, 4), hull_over_sort=round((fit_ms - sort_ms) / sort_ms, 2),
                 hull_over_sort_distinct=round((extra["fit_distinct_ms"] - sort_ms) / sort_ms, 2))
    scores = torch.from_numpy(p).to(dev)
    out_t = torch.empty_like(scores)
    apply_ms = _device_ms(lambda: cal.apply(scores, out=out_t))
    assert out_t.cpu().numpy().tobytes() == R.apply_ref(ref, p).tobytes()
    floor_ms = 8.0 * n / (HBM_GBS * 1e9) * 1e3
    out = {"device": torch.cuda.get_device_name(dev), "rows": args.rows, "batch": B, "d": args.d, "runs": RUNS,
           "statistic": "median", "host_fit": host_fit, "host_loop_ms": round(host_ms, 3),
           "evaluate_iso_ms": round(iso_ms, 3), "evaluate_ms": round(plain_ms, 3), "isotonic_cost_ms": round(iso_ms - plain_ms, 3),
           "fit_ms": round(fit_ms, 4), "calib_reduce_ms": round(reduce_ms, 4), "fit_over_reduce": round(fit_ms / reduce_ms, 2),
           "blocks": K, "max_blocks": int(_lib.lib().fbn_isotonic_max_blocks(n)),
           "adversarial_rows": len(ya), "fit_adversarial_ms": round(adv_ms, 4), "blocks_adversarial": K_adv,
           "calib_reduce_adversarial_ms": None if reduce_adv_ms is None else round(reduce_adv_ms, 4),
           "apply_ms": round(apply_ms, 4), "apply_floor_ms": round(floor_ms, 5), "apply_gbs": round(8.0 * n / apply_ms / 1e6, 1),
           "blocks_equal_host": True, "apply_equal_host": True}
    out.update(extra)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
