"""HR@K, NDCG@K and MRR@K of held-out items from an integer record kept on the device.

``Recommender.rank`` gives each evaluation user the rank of its held-out item among the eligible
catalogue items.  :class:`RankMetrics` adds such ranks to a 260-word uint64 record with
``fbn_rank_hist`` (csrc/recommend.hip) -- a histogram of the ranks 1..256, the count above, the count
of users that were not ranked, the sum and the number of the ranks -- and every metric is a float64
function of those exact integers, computed on the host by :func:`rank_metrics_from_record`.  The
record is additive: over ``update`` calls here, and over devices by an integer sum.

    m = RankMetrics(device="cuda")
    for seq, target in blocks:
        m.update(rec.rank(seq, target)["rank"])     # one launch, no host sync
    out = m.compute(ks=(5, 10, 20))                 # one 2,080-byte read
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import call

REC_WORDS = _lib.FBN_RANK_REC_WORDS      # 8-byte words of the record
K_MAX = 256          # the ranks the record keeps one by one
_NOT_RANKED, _ABOVE, _SUM, _COUNT = 0, 257, 258, 259


def _check_ks(ks: Iterable[int]):
    out = []
    for k in ks:
        if int(k) != k or not 1 <= int(k) <= K_MAX:
            raise ValueError(f"K must be an integer in 1..{K_MAX}, not {k!r}")
        out.append(int(k))
    return out


def rank_metrics_from_record(rec: Sequence[int], ks: Iterable[int] = (5, 10, 20)) -> Dict:
    """The metrics of a 260-word rank record (``fbn_rank_hist``'s layout) over its n = rec[259] ranked
    users: ``{"n", "n_skipped", "mean_rank", "hr": {K: }, "ndcg": {K: }, "mrr": {K: }}`` with

        hr[K]   = sum_{r <= K} rec[r] / n
        ndcg[K] = sum_{r <= K} rec[r] / log2(r + 1) / n      (one relevant item per user: IDCG = 1)
        mrr[K]  = sum_{r <= K} rec[r] / r / n
        mean_rank = rec[258] / n

    in float64 from exact integers (an integer ratio is correctly rounded; the at most 256 terms of a
    sum go through math.fsum).  n == 0: every metric is nan.  Each K must be in 1..256."""
    ks = _check_ks(ks)
    r = [int(x) for x in rec]
    if len(r) != REC_WORDS:
        raise ValueError(f"a rank record has {REC_WORDS} words, not {len(r)}")
    n = r[_COUNT]
    nan = float("nan")
    out = {"n": n, "n_skipped": r[_NOT_RANKED], "mean_rank": r[_SUM] / n if n else nan, "hr": {}, "ndcg": {}, "mrr": {}}
    for k in ks:
        if not n:
            out["hr"][k] = out["ndcg"][k] = out["mrr"][k] = nan
            continue
        out["hr"][k] = sum(r[1:k + 1]) / n
        out["ndcg"][k] = math.fsum(r[j] / math.log2(j + 1) for j in range(1, k + 1)) / n
        out["mrr"][k] = math.fsum(r[j] / j for j in range(1, k + 1)) / n
    return out


class RankMetrics:
    """Streaming HR / NDCG / MRR@K: the rank record lives on ``device``; ``update`` is one launch."""

    def __init__(self, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("RankMetrics runs on a HIP device only (no CPU fallback)")
        # uint64 words (counts stay far below 2^63, so the int64 view reads them as they are)
        self.rec = torch.zeros(REC_WORDS, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        self.rec.zero_()

    def update(self, rank: torch.Tensor) -> None:
        """Add a batch of ranks (int32, ``Recommender.rank``'s ``"rank"``; 0 or negative: not ranked):
        one ``fbn_rank_hist`` launch, no host sync."""
        _lib.require_hip(rank, "rank")
        if rank.dtype != torch.int32:
            raise TypeError(f"rank must be int32, not {rank.dtype}")
        n = rank.numel()
        if n == 0:
            return
        r = rank.detach().reshape(-1).contiguous()
        with torch.cuda.device(self.device):
            call("fbn_rank_hist", r.data_ptr(), n, self.rec.data_ptr(), _lib.stream_handle(self.device))

    def record(self) -> np.ndarray:
        """The record on the host, uint64 [260]: the one device-to-host read (2,080 bytes)."""
        return self.rec.cpu().numpy().view(np.uint64)

    def compute(self, ks: Iterable[int] = (5, 10, 20)) -> Dict:
        """:func:`rank_metrics_from_record` of the ranks added so far (they stay: compute() can be repeated)."""
        ks = _check_ks(ks)
        return rank_metrics_from_record(self.record(), ks)
