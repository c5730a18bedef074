"""The bf16 margin of tests/test_gpu_recommend_lists.py, measured (not part of bench.py).

For every (mode, d) of that file's BF16_SPREAD_BOUND: max |dlogit| of the project's eval forward
(ops.forward) against itself on the 900 expanded rows of the test's shortlists, run as one batch and as
two halves (the test's _list_forward_spread), the bound max(4 x spread, 1e-4) that follows, and for
information the distance of Recommender.score_lists to that forward under both chunkings.

    python tools/recommend_lists_parity.py [--out profiles/recommend_lists_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import test_gpu_recommend_lists as T


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join("profiles", "recommend_lists_parity.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev), "users": T.U_HIST, "slots": T.S_C, "rows": T.U_HIST * T.S_C,
           "what": "forward_spread: max |dlogit| of ops.forward (eval) on the expanded list rows, one batch vs two "
                   "halves; bound = max(4 x forward_spread, 1e-4); lists_vs_forward: Recommender.score_lists "
                   "against that forward, per chunk_rows",
           "cases": []}
    pos = T._short_lists().to(dev)
    live = pos >= 0
    for mode, d in sorted(T.BF16_SPREAD_BOUND):
        spread, whole = T._list_forward_spread(d, mode, dev)
        case = {"mode": mode, "d": d, "forward_spread": spread, "bound": max(4 * spread, 1e-4), "lists_vs_forward": {}}
        for chunk_rows in (T.S_CHUNKED, T.S_SINGLE):
            rec = T._rec(d, dev, chunk_rows, mode=mode)
            lg = rec.score_lists(T._histories().to(dev), pos, by="index", logits=True)
            case["lists_vs_forward"][str(chunk_rows)] = (lg - whole.view(T.U_HIST, T.S_C))[live].abs().max().item()
        out["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
