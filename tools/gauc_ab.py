"""Per-user grouped AUC on the device vs on the host, timed in one process (not part of bench.py).

A synthetic 1 M-row validation split at d = 128, bf16, batch 8192 (HBM-resident batches, the last one
short), user_id uniform over 50 000 users, an untrained FiBiNETTrainer:
  (a) host_loop_ms     what a user had to write: predict().cpu() per batch, labels and user ids to the
                       host, a group-by there and utils.compute_auc per user
  (b) evaluate_gauc_ms FiBiNETTrainer.evaluate(group_by="user_id")
  (c) evaluate_ms      FiBiNETTrainer.evaluate() without groups
  (d) gauc_reduce_ms   fbn_gauc_reduce alone on the split's keys and group ids
  (e) torch_sort_ms    torch.sort of the same composite int64 keys (the floor of a torch-based design)
  (f) sort_u64_ms      fbn_sort_u64(bits = 63) alone on them
Each figure is the median of RUNS timed runs after a warm-up: HIP events around device-only work,
perf_counter around the host loops (which end in a synchronise).  (b)'s group table must equal (a)'s.

    python tools/gauc_ab.py [--rows 1000000] [--users 50000] [--out profiles/gauc_device_vs_host.json]
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
    ap.add_argument("--users", type=int, default=50_000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=1_250_000)
    ap.add_argument("--out", default=os.path.join("profiles", "gauc_device_vs_host.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, L = args.batch, 20
    full, rest = divmod(args.rows, B)
    batches = make_device_batches(full, B, args.vocab, L, dev, seed=11)
    if rest:
        batches += make_device_batches(1, rest, args.vocab, L, dev, seed=12)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    for batch, labels in batches:
        batch["user_id"] = torch.randint(0, args.users, (labels.numel(),), generator=g, device=dev, dtype=torch.int64)
    cfg = {"embedding_dim": args.d, "vocab_size": args.vocab, "compute_dtype": "bf16"}
    tr = FiBiNETTrainer(cfg, total_steps=10, batch_size=B, device=dev, seed=7)

    def host_loop():
        ys, ps, us = [], [], []
        for batch, labels in batches:
            ps.append(tr.predict(batch).cpu().numpy())
            ys.append(labels.cpu().numpy())
            us.append(batch["user_id"].cpu().numpy())
        y, p, u = np.concatenate(ys), np.concatenate(ps), np.concatenate(us)
        order = np.argsort(u, kind="stable")
        y, p, u = y[order], p[order], u[order]
        starts = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
        ends = np.r_[starts[1:], len(u)]
        n_pos = np.add.reduceat(y, starts).astype(np.int64)
        n_neg = (ends - starts) - n_pos
        auc = np.full(len(starts), np.nan)
        for k in np.flatnonzero((n_pos > 0) & (n_neg > 0)):
            auc[k] = compute_auc(y[starts[k]:ends[k]], p[starts[k]:ends[k]])
        mixed = ~np.isnan(auc)
        w = (n_pos + n_neg)[mixed]
        return {"group": u[starts], "n_pos": n_pos, "n_neg": n_neg, "auc": auc,
                "gauc": float((w * auc[mixed]).sum() / w.sum())}

    host_ms, host = _host_ms(host_loop)
    gauc_ms, ev = _host_ms(lambda: tr.evaluate(batches, group_by="user_id"))
    m = tr._eval_metrics                                    # the split's keys and ids, as evaluate() left them
    n = m.count
    table = {k: v.cpu().numpy() for k, v in m.group_table().items()}
    assert ev["n"] == args.rows and np.array_equal(table["group"], host["group"]), "groups differ"
    assert np.array_equal(table["n_pos"], host["n_pos"]) and np.array_equal(table["n_neg"], host["n_neg"])
    mixed = (table["n_pos"] > 0) & (table["n_neg"] > 0)
    dev_auc = table["u2"][mixed].astype(np.float64) / (2 * table["n_pos"][mixed] * table["n_neg"][mixed]).astype(np.float64)
    assert np.array_equal(dev_auc, host["auc"][mixed]), "a user's AUC differs from compute_auc"
    assert abs(ev["gauc"] - host["gauc"]) <= 1e-11 * host["gauc"]
    keys, gids = m.keys[:n].clone(), m.gids[:n].clone()
    plain_ms, ev_plain = _host_ms(lambda: tr.evaluate(batches))
    assert ev_plain["auc"] == ev["auc"]

    rec = torch.zeros(5 + _lib.FBN_GAUC_REC_WORDS, dtype=torch.int64, device=dev)
    ws = torch.empty(int(_lib.call("fbn_gauc_workspace_size", n)), dtype=torch.uint8, device=dev)
    tab = torch.empty((n, 4), dtype=torch.int64, device=dev)
    reduce_ms = _device_ms(lambda: _lib.call("fbn_gauc_reduce", keys.data_ptr(), gids.data_ptr(), n, ws.data_ptr(),
                                             ws.numel(), tab.data_ptr(), rec.data_ptr() + 40, rec.data_ptr() + 32,
                                             _lib.stream_handle(dev)))
    comp = ((gids.to(torch.int64) & 0xFFFFFFFF) << 31) | keys.to(torch.int64)
    out_keys = torch.empty_like(comp)
    sws = torch.empty(int(_lib.call("fbn_sort_u64_workspace_size", n)), dtype=torch.uint8, device=dev)
    torch_sort_ms = _device_ms(lambda: torch.sort(comp))
    sort_ms = _device_ms(lambda: _lib.call("fbn_sort_u64", comp.data_ptr(), n, 63, sws.data_ptr(), sws.numel(),
                                           out_keys.data_ptr(), _lib.stream_handle(dev)))
    assert torch.equal(out_keys, torch.sort(comp).values), "fbn_sort_u64 differs from torch.sort"
    out = {"device": torch.cuda.get_device_name(dev), "rows": args.rows, "users": args.users, "batch": B, "d": args.d,
           "runs": RUNS, "statistic": "median", "host_loop_ms": round(host_ms, 3), "evaluate_gauc_ms": round(gauc_ms, 3),
           "evaluate_ms": round(plain_ms, 3), "gauc_reduce_ms": round(reduce_ms, 4), "torch_sort_ms": round(torch_sort_ms, 4),
           "sort_u64_ms": round(sort_ms, 4), "gauc": ev["gauc"], "gauc_macro": ev["gauc_macro"],
           "gauc_clicks": ev["gauc_clicks"], "n_groups": ev["n_groups"], "n_groups_mixed": ev["n_groups_mixed"],
           "auc": ev["auc"], "table_equal_host": True}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
