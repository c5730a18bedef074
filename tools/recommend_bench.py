"""Top-K recommendation: the serving path vs expanded rows, timed in one process (not part of bench.py).

C3-shaped weights (d = 128, bf16, the reference's 91,718-row table as the catalogue), U = 64 user
histories of L = 20, K = 10:
  (a) topk_ms       Recommender.topk: per-user and per-candidate caches, pair composition, the eval
                    forward's tail per chunk, device-side selection
  (b) expanded_ms   the route without it: the U x M pairs expanded into ordinary batches of 8192 rows
                    (row gathers on the device), each through the eval forward (ops.forward, same
                    weights and dtype), the logits collected into [U, M], then torch.topk
Each figure is the median of RUNS timed runs after a warm-up (HIP events, one process, the two routes
interleaved).  stage_ms: kernel spans of (a)'s stages summed over the chunks of one probed run (the
library's kernel probes; "forward" is the whole chunk forward, fields included).

    python tools/recommend_bench.py [--users 64] [--out profiles/recommend_vs_expanded.json]

--rank-eval: the same shape and method for the rank evaluation, one target per user:
  (a) rank_ms       Recommender.rank + RankMetrics.update: the sweep into a [U, M] buffer of logits,
                    fbn_rec_rank, fbn_rank_hist
  (b) topk_ms       Recommender.topk(k = 10) of the same users
with (a)'s kernel spans per stage; written to profiles/recommend_rank_eval.json.

--lists: per-user shortlists, U = 64 users, C = 500 slots each (5 % empty), K = 10,
d = 128, once in fp32 and once in bf16:
  (a) topk_lists_ms  Recommender.topk_lists over the U x C pairs
  (b) topk_ms        Recommender.topk of the same users over the whole catalogue (U x M pairs)
per call, the two routes interleaved after a warm-up; a run times several back-to-back calls with one
HIP event pair so the window is not a single short call.  No threshold: the two figures and their
ratio, written to profiles/recommend_lists.json.

--retrieve: the two-stage path at the first leg's shape (d = 128, bf16, M = 91,718, U = 64,
L = 20, K = 10), same method:
  (a) topk_ms        Recommender.topk(k = 10) over the whole catalogue
  (b) recommend_ms   Recommender.recommend(k = 10, n_candidates = 200): retrieval in the content space,
                     then topk_lists over each user's 200
and fbn_knn_scores alone at Q = 64 and Q = 8192 over the whole catalogue beside fbn_gemm (fp32, transB)
on the same normalised operands (back-to-back calls per timed run, the two interleaved), with the largest
difference between their outputs.  Written to profiles/retrieve_two_stage.json.

--diversify: MMR re-ranking behind the retrieval stage, same shape and method:
  (a) recommend_ms      Recommender.recommend(k = 10, n_candidates = 200): retrieve + topk_lists
  (b) recommend_lam_ms  Recommender.recommend(..., lam = 0.7): retrieve + diversify
and, from separate probed runs of (b), the kernel span of fbn_mmr_select.  Written to
profiles/diversify.json.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ctr_recommendation_amd import _lib, ops
from ctr_recommendation_amd.model_fibinet import build_model
from ctr_recommendation_amd.recommend import Recommender

RUNS = 10


def _span(probes):
    return sum(max(0.0, kp.elapsed_time()) for kp, _ in probes)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def rank_eval(args, rec, seq, target):
    """(a) rank() + RankMetrics.update vs (b) topk(k) of the same users; target: [U] catalogue positions."""
    import ctr_recommendation_amd.rank_metrics as mmod
    import ctr_recommendation_amd.recommend as rmod
    dev, U, K = rec.device, seq.shape[0], args.k
    metrics = mmod.RankMetrics(dev)

    def ranking():
        out = rec.rank(seq, target, by="index")
        metrics.update(out["rank"])
        return out

    def selecting():
        return rec.topk(seq, K)

    ranking(), selecting()                                  # warm-up (allocations, bf16 images)
    ta, tb = [], []
    for _ in range(args.runs):                              # interleaved A/B
        ta.append(_timed(ranking)[0])
        t, top = _timed(selecting)
        tb.append(t)
    out = ranking()
    rec.check_ids()
    rank, index = out["rank"].cpu(), top["index"].cpu()
    tpos = target.cpu()
    agree = all((int(rank[u]) <= K) == (int(tpos[u]) in index[u].tolist()) for u in range(U) if int(rank[u]) >= 1)

    # one probed run of (a): kernel spans per stage, summed over the chunks
    stages, whole = {}, []
    call0, mcall0, fwd0 = rmod.call, mmod.call, rec._forward_chunk

    def probed_call(name, *a):
        if name in ("fbn_rec_hist_pool", "fbn_rec_rank", "fbn_rank_hist"):
            kp = _lib.KernelProbe()
            stages.setdefault(name, []).append((kp, None))
            try:
                return call0(name, *a)
            finally:
                kp.done()
        return call0(name, *a)

    def probed_forward(*a):
        kp = _lib.KernelProbe()
        whole.append((kp, None))
        try:
            return fwd0(*a)
        finally:
            kp.done()

    rmod.call = mmod.call = probed_call
    rec._forward_chunk = probed_forward
    ranking()
    torch.cuda.synchronize()
    rmod.call, mmod.call, rec._forward_chunk = call0, mcall0, fwd0
    stage_ms = {"hist_pool": _span(stages["fbn_rec_hist_pool"]), "forward": _span(whole),
                "rank": _span(stages["fbn_rec_rank"]), "rank_hist": _span(stages["fbn_rank_hist"])}
    # the sweep's copies of each chunk's logits into the [U, M] buffer (torch's strided copy_), alone
    chunks = list(rec._chunks(U))
    n_chunks, (m0, Mc) = len(chunks), chunks[0]
    full, chunk = torch.empty((U, rec.M), device=dev), torch.zeros(U * Mc, device=dev)

    def copies():
        for _ in range(n_chunks):
            full[:, m0:m0 + Mc].copy_(chunk.view(U, Mc))

    copies()
    stage_ms["buffer_copies_event_ms"] = statistics.median(_timed(copies)[0] for _ in range(5))

    ma, mb = statistics.median(ta), statistics.median(tb)
    res = {"device": torch.cuda.get_device_name(dev), "users": U, "items": rec.M, "k": K, "d": rec.d,
           "dtype": args.dtype, "chunk_rows": rec.chunk_rows, "chunks": n_chunks, "runs": args.runs,
           "statistic": "median", "rank_ms": round(ma, 3), "topk_ms": round(mb, 3),
           "ratio_rank_over_topk": round(ma / mb, 3), "rank_ms_min_max": [round(min(ta), 3), round(max(ta), 3)],
           "topk_ms_min_max": [round(min(tb), 3), round(max(tb), 3)],
           "logits_buffer_bytes": 4 * U * rec.M, "stage_ms": {k: round(v, 3) for k, v in stage_ms.items()},
           "rank_agrees_with_topk": bool(agree), "metrics": metrics.compute((5, 10, 20))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def _catalogue(M, g):
    x = torch.randn((M, 128), generator=g)
    return {"item_id": torch.arange(M), "likes_level": torch.randint(0, 11, (M,), generator=g),
            "views_level": torch.randint(0, 11, (M,), generator=g), "item_emb_d128": x / x.norm(dim=1, keepdim=True)}


def lists_bench(args):
    """--lists: topk_lists over per-user shortlists beside the full-catalogue topk of the same users."""
    dev = torch.device("cuda", 0)
    U, M, C, K, d, L = args.users, args.items, args.slots, args.k, args.d, 20
    res = {"device": torch.cuda.get_device_name(dev), "users": U, "items": M, "slots": C, "k": K, "d": d,
           "runs": args.runs, "statistic": "median of runs; each run times `calls` back-to-back calls with one "
                                           "HIP event pair and divides by `calls`; the two routes interleaved",
           "modes": {}}
    for dtype in ("fp32", "bf16"):
        cfg = {"embedding_dim": d, "vocab_size": M, "compute_dtype": dtype}
        torch.manual_seed(3)
        model = build_model(None, cfg).eval()
        g = torch.Generator().manual_seed(5)
        cat = _catalogue(M, g)
        seq = torch.randint(1, M, (U, L), generator=g)
        seq[torch.rand((U, L), generator=g) < 0.3] = 0
        cand = torch.randint(0, M, (U, C), generator=g)
        cand[torch.rand((U, C), generator=g) < 0.05] = -1          # ragged lists: 5 % empty slots
        seq, cand = seq.to(dev), cand.to(dev)
        rec = Recommender(model.state_dict(), cfg, cat, device=dev, chunk_rows=args.chunk_rows)
        calls = {"lists": args.list_calls, "catalogue": 2}

        def lists():
            for _ in range(calls["lists"]):
                out = rec.topk_lists(seq, cand, K, by="index")
            return out

        def catalogue():
            for _ in range(calls["catalogue"]):
                out = rec.topk(seq, K)
            return out

        lists(), catalogue()                                    # warm-up (allocations, bf16 images, both shapes)
        ta, tb = [], []
        for _ in range(args.runs):                              # interleaved A/B
            t, la = _timed(lists)
            ta.append(t / calls["lists"])
            t, lb = _timed(catalogue)
            tb.append(t / calls["catalogue"])
        rec.check_ids()
        # the shortlist's winners come from the catalogue's scores: every returned logit is that pair's
        full = rec.score(seq, logits=True)
        live = la["index"] >= 0
        same = (full.gather(1, la["index"].clamp(min=0)) - la["logit"])[live].abs().max().item()
        ma, mb = statistics.median(ta), statistics.median(tb)
        res["modes"][dtype] = {
            "chunk_rows": rec.chunk_rows, "list_chunks": len(list(rec._chunks(U, C))),
            "catalogue_chunks": len(list(rec._chunks(U))), "calls_per_run": dict(calls),
            "topk_lists_ms": round(ma, 4), "topk_ms": round(mb, 4), "ratio_topk_over_topk_lists": round(mb / ma, 2),
            "topk_lists_ms_min_max": [round(min(ta), 4), round(max(ta), 4)],
            "topk_ms_min_max": [round(min(tb), 4), round(max(tb), 4)],
            "pairs_scored": {"lists": U * C, "catalogue": U * M},
            "max_abs_dlogit_vs_catalogue_scores": same}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def retrieve_bench(args, rec, seq):
    """--retrieve: topk vs recommend, then fbn_knn_scores vs fbn_gemm on the same operands."""
    import ctr_recommendation_amd.recommend as rmod
    dev, U, K, M = rec.device, seq.shape[0], args.k, rec.M
    n_cand, space = args.candidates, "content"

    def full():
        return rec.topk(seq, K)

    def two_stage():
        return rec.recommend(seq, K, n_candidates=n_cand, space=space)

    full(), two_stage()                                     # warm-up (allocations, bf16 images, the space)
    ta, tb = [], []
    for _ in range(args.runs):                              # interleaved A/B
        t, ra = _timed(full)
        ta.append(t)
        t, rb = _timed(two_stage)
        tb.append(t)
    rec.check_ids()
    # how much of the full sweep's top K the shortlist kept (random weights and vectors: a property of
    # this synthetic input, not of any model)
    overlap = sum(len(set(ra["index"][u].tolist()) & set(rb["index"][u].tolist())) for u in range(U)) / (U * K)

    # one probed run of (b): kernel spans per stage
    stages = {}
    call0 = rmod.call

    def probed_call(name, *a):
        if name.startswith("fbn_knn_") or name in ("fbn_rec_topk", "fbn_rec_topk_list"):
            kp = _lib.KernelProbe()
            stages.setdefault(name, []).append((kp, None))
            try:
                return call0(name, *a)
            finally:
                kp.done()
        return call0(name, *a)

    rmod.call = probed_call
    two_stage()
    torch.cuda.synchronize()
    rmod.call = call0
    stage_ms = {k[4:]: round(_span(v), 4) for k, v in stages.items()}

    # the scores kernel alone beside fbn_gemm on the same normalised operands
    st = _lib.stream_handle(dev)
    xn = rec._space(space, st)
    D = int(xn.shape[1])
    g = torch.Generator().manual_seed(11)
    kernels = {}
    for Q, calls in ((64, 20), (8192, 1)):
        q = torch.randn((Q, D), generator=g)
        qn = (q / q.norm(dim=1, keepdim=True)).to(dev).contiguous()
        Sa = torch.empty((Q, M), dtype=torch.float32, device=dev)
        Sb = torch.empty((Q, M), dtype=torch.float32, device=dev)

        def knn():
            for _ in range(calls):
                _lib.call("fbn_knn_scores", _lib.ptr(qn), D, None, _lib.ptr(xn), M, Q, 0, M, D, _lib.ptr(Sa), st)

        def gemm():
            for _ in range(calls):
                ops.gemm(qn, xn, Sb, Q, M, D, D, D, M, False, True, stream=st)

        knn(), gemm()
        ka, kb = [], []
        for _ in range(args.runs):
            ka.append(_timed(knn)[0] / calls)
            kb.append(_timed(gemm)[0] / calls)
        ma, mb = statistics.median(ka), statistics.median(kb)
        kernels[f"Q{Q}"] = {"calls_per_run": calls, "knn_scores_ms": round(ma, 4), "gemm_fp32_ms": round(mb, 4),
                            "ratio_gemm_over_knn": round(mb / ma, 3),
                            "knn_scores_ms_min_max": [round(min(ka), 4), round(max(ka), 4)],
                            "gemm_fp32_ms_min_max": [round(min(kb), 4), round(max(kb), 4)],
                            "knn_gbytes_per_s": round((4.0 * M * D + 4.0 * Q * M) / ma / 1e6, 1),
                            "knn_tflops": round(2.0 * Q * M * D / ma / 1e9, 2),
                            "max_abs_diff_vs_gemm": (Sa - Sb).abs().max().item()}
        del Sa, Sb

    ma, mb = statistics.median(ta), statistics.median(tb)
    res = {"device": torch.cuda.get_device_name(dev), "users": U, "items": M, "k": K, "d": rec.d, "dtype": args.dtype,
           "space": space, "space_dim": D, "n_candidates": n_cand, "runs": args.runs,
           "statistic": "median of runs (HIP events, one process, the two routes interleaved)",
           "topk_ms": round(ma, 3), "recommend_ms": round(mb, 3), "ratio_topk_over_recommend": round(ma / mb, 2),
           "topk_ms_min_max": [round(min(ta), 3), round(max(ta), 3)],
           "recommend_ms_min_max": [round(min(tb), 3), round(max(tb), 3)],
           "pairs_scored": {"topk": U * M, "recommend": U * n_cand},
           "recommend_stage_kernel_ms": stage_ms, "topk_overlap_on_random_input": round(overlap, 4),
           "scores_kernel": kernels}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def diversify_bench(args, rec, seq):
    """--diversify: recommend(lam=None) beside recommend(lam=args.lam), then fbn_mmr_select's kernel span."""
    import ctr_recommendation_amd.recommend as rmod
    dev, U, K = rec.device, seq.shape[0], args.k
    n_cand, space, lam = args.candidates, "content", args.lam

    def plain():
        return rec.recommend(seq, K, n_candidates=n_cand, space=space)

    def diverse():
        return rec.recommend(seq, K, n_candidates=n_cand, space=space, lam=lam)

    plain(), diverse()                                      # warm-up (allocations, bf16 images, the space)
    ta, tb = [], []
    for _ in range(args.runs):                              # interleaved A/B
        t, ra = _timed(plain)
        ta.append(t)
        t, rb = _timed(diverse)
        tb.append(t)
    rec.check_ids()
    # what the re-ranking did to these lists (random weights and vectors: a property of this synthetic
    # input, not of any model)
    ild = {n: rec.list_diversity(r["index"], space=space) for n, r in (("plain", ra), ("diverse", rb))}
    ild = {n: round(float(v["ild"][v["n_pairs"] > 0].mean().item()), 6) for n, v in ild.items()}
    overlap = sum(len(set(ra["index"][u].tolist()) & set(rb["index"][u].tolist())) for u in range(U)) / (U * K)

    # a separate probed run of the diversified route: kernel spans per stage
    stages = {}
    call0 = rmod.call

    def probed_call(name, *a):
        if name.startswith("fbn_knn_") or name in ("fbn_rec_topk", "fbn_mmr_select", "fbn_rec_hist_pool"):
            kp = _lib.KernelProbe()
            stages.setdefault(name, []).append((kp, None))
            try:
                return call0(name, *a)
            finally:
                kp.done()
        return call0(name, *a)

    rmod.call = probed_call
    spans = []
    for _ in range(args.runs):
        stages.clear()
        diverse()
        torch.cuda.synchronize()
        spans.append(_span(stages["fbn_mmr_select"]))
    rmod.call = call0
    stage_ms = {k[4:]: round(_span(v), 4) for k, v in stages.items()}

    ma, mb = statistics.median(ta), statistics.median(tb)
    D = int(rec._knn[space].shape[1])
    res = {"device": torch.cuda.get_device_name(dev), "users": U, "items": rec.M, "k": K, "d": rec.d,
           "dtype": args.dtype, "space": space, "space_dim": D, "n_candidates": n_cand, "lam": lam, "runs": args.runs,
           "statistic": "median of runs (HIP events, one process, the two routes interleaved)",
           "recommend_ms": round(ma, 4), "recommend_lam_ms": round(mb, 4), "added_ms": round(mb - ma, 4),
           "ratio_lam_over_plain": round(mb / ma, 3),
           "recommend_ms_min_max": [round(min(ta), 4), round(max(ta), 4)],
           "recommend_lam_ms_min_max": [round(min(tb), 4), round(max(tb), 4)],
           "raw_recommend_ms": [round(t, 4) for t in ta], "raw_recommend_lam_ms": [round(t, 4) for t in tb],
           "mmr_select_kernel_ms": round(statistics.median(spans), 4),
           "mmr_select_kernel_ms_min_max": [round(min(spans), 4), round(max(spans), 4)],
           "lam_route_stage_kernel_ms": stage_ms,
           "mean_ild_on_random_input": ild, "list_overlap_on_random_input": round(overlap, 4)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--users", type=int, default=64)
    ap.add_argument("--items", type=int, default=91718)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--chunk-rows", type=int, default=None)
    ap.add_argument("--runs", type=int, default=RUNS)
    ap.add_argument("--rank-eval", action="store_true", help="time rank() + RankMetrics.update against topk")
    ap.add_argument("--lists", action="store_true", help="time topk_lists on per-user shortlists against topk")
    ap.add_argument("--slots", type=int, default=500, help="--lists: slots per user")
    ap.add_argument("--list-calls", type=int, default=20, help="--lists: topk_lists calls per timed run")
    ap.add_argument("--retrieve", action="store_true", help="time recommend (retrieve + topk_lists) against topk")
    ap.add_argument("--candidates", type=int, default=200, help="--retrieve / --diversify: shortlist length per user")
    ap.add_argument("--diversify", action="store_true", help="time recommend(lam) against recommend(lam=None)")
    ap.add_argument("--lam", type=float, default=0.7, help="--diversify: the MMR trade-off")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join("profiles", "recommend_lists.json" if args.lists else
                                "diversify.json" if args.diversify else
                                "retrieve_two_stage.json" if args.retrieve else
                                "recommend_rank_eval.json" if args.rank_eval else "recommend_vs_expanded.json")
    if args.lists:
        return lists_bench(args)
    dev = torch.device("cuda", 0)
    U, M, K, d, L, B = args.users, args.items, args.k, args.d, 20, args.batch
    cfg = {"embedding_dim": d, "vocab_size": M, "compute_dtype": args.dtype}
    torch.manual_seed(3)
    model = build_model(None, cfg).eval()
    g = torch.Generator().manual_seed(5)
    x = torch.randn((M, 128), generator=g)
    cat = {"item_id": torch.arange(M), "likes_level": torch.randint(0, 11, (M,), generator=g),
           "views_level": torch.randint(0, 11, (M,), generator=g), "item_emb_d128": x / x.norm(dim=1, keepdim=True)}
    seq = torch.randint(1, M, (U, L), generator=g)
    seq[torch.rand((U, L), generator=g) < 0.3] = 0
    seq = seq.to(dev)
    rec = Recommender(model.state_dict(), cfg, cat, device=dev, chunk_rows=args.chunk_rows)
    if args.retrieve:
        return retrieve_bench(args, rec, seq)
    if args.diversify:
        return diversify_bench(args, rec, seq)
    if args.rank_eval:
        return rank_eval(args, rec, seq, torch.randint(0, M, (U,), generator=g).to(dev))
    catd = {k: v.to(dev) for k, v in rec.cat.items()}
    catd["item_emb_d128"] = rec._x
    fcfg = ops.FwdConfig(**{**rec.cfg.__dict__, "L": L})
    acts = {}

    def expanded():
        out = torch.empty(U * M, dtype=torch.float32, device=dev)
        for r0 in range(0, U * M, B):
            r = torch.arange(r0, min(r0 + B, U * M), device=dev)
            u, m = r // M, r % M
            batch = {k: v[m] for k, v in catd.items()}
            batch["item_seq"] = seq[u]
            a = ops.forward(rec.p, batch, fcfg, acts=acts.setdefault(r.numel(), {}))
            out[r0:r0 + r.numel()] = a["logits"]
        return torch.topk(out.view(U, M), K, dim=1)

    def serving():
        return rec.topk(seq, K, exclude_history=False)

    serving(), expanded()                                   # warm-up (allocations, bf16 images)
    ta, tb = [], []
    for _ in range(args.runs):                              # interleaved A/B
        t, ra = _timed(serving)
        ta.append(t)
        t, rb = _timed(expanded)
        tb.append(t)
    rec.check_ids()
    same = (ra["index"] == rb.indices).float().mean().item()

    # one probed run of (a): kernel spans per stage, summed over the chunks
    stages = {}
    probe = {}
    rec._probe = probe
    call0 = _lib.call

    def probed_call(name, *a):
        if name in ("fbn_rec_hist_pool", "fbn_rec_topk"):
            kp = _lib.KernelProbe()
            stages.setdefault(name, []).append((kp, None))
            try:
                return call0(name, *a)
            finally:
                kp.done()
        return call0(name, *a)

    import ctr_recommendation_amd.recommend as rmod
    rmod.call = probed_call
    serving()
    torch.cuda.synchronize()
    rmod.call = call0
    rec._probe = None
    stage_ms = {"hist_pool": _span(stages["fbn_rec_hist_pool"]), "fields": _span(probe["fields_fwd"]),
                "gemm_mlp0": _span(probe["gemm_mlp0"]), "topk": _span(stages["fbn_rec_topk"])}
    whole = []
    fwd0 = rec._forward_chunk

    def probed_forward(*a):
        kp = _lib.KernelProbe()
        whole.append((kp, None))
        try:
            return fwd0(*a)
        finally:
            kp.done()

    rec._forward_chunk = probed_forward
    serving()
    torch.cuda.synchronize()
    rec._forward_chunk = fwd0
    stage_ms["forward"] = _span(whole)

    ma, mb = statistics.median(ta), statistics.median(tb)
    out = {"device": torch.cuda.get_device_name(dev), "users": U, "items": M, "k": K, "d": d, "dtype": args.dtype,
           "expanded_batch": B, "chunk_rows": rec.chunk_rows, "chunks": len(list(rec._chunks(U))), "runs": args.runs,
           "statistic": "median", "topk_ms": round(ma, 3), "expanded_ms": round(mb, 3),
           "ratio_expanded_over_topk": round(mb / ma, 3), "topk_ms_min_max": [round(min(ta), 3), round(max(ta), 3)],
           "expanded_ms_min_max": [round(min(tb), 3), round(max(tb), 3)],
           "stage_ms": {k: round(v, 3) for k, v in stage_ms.items()},
           "index_agreement_with_expanded": round(same, 6)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
