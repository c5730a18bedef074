"""Validation AUC and log-loss computed on the device, exactly (csrc/metrics.hip).

The reference's validation (src/train_fibinet.py:133-146) copies every batch's probabilities to the
host and runs roc_auc_score / log_loss there (src/utils.py:18-32).  :class:`DeviceMetrics` keeps one
uint32 key per sample on the device -- ``(bits(p) << 1) | y`` for an fp32 probability p in [0, 1] --
and counts: the AUC is ``U2 / (2 n_pos n_neg)`` with U2 an exact integer (Python int / int: correctly
rounded), the same double ``utils.compute_auc`` returns on the same fp32 probabilities while
``n_pos * n_neg < 2^53``; the log-loss is ``utils.compute_logloss``'s float64 expression summed as a
fixed-shape tree (bitwise reproducible for the same sample sequence).

    m = DeviceMetrics(capacity=len(valid_rows), device="cuda")
    for batch, labels in valid_batches:
        m.update(model(batch), labels)          # one launch, no host sync
    out = m.compute()                           # {"auc", "logloss", "n", "n_pos"}: one 40-byte read

``grouped=True`` adds the per-group AUC (GAUC, §19): ``update(..., group_ids=batch["user_id"])`` keeps
4 more bytes per sample, and compute() also returns the AUC averaged over the groups that hold both
classes -- exact integer counts per group, float64 sums in ascending id order, so the numbers do not
depend on the samples' order, on the update sizes or on the rank split.

``calibration(bins)`` is the other half of validation (§20): the reliability table of the samples held, in
equal-width and in equal-mass bins, as exact integers from one device sort and one prefix sum, and the
ECE / MCE / PCOC / Brier score derived from it on the host with Python integers.

``isotonic()`` closes the loop (§25): the exact isotonic fit of the samples held, as an
:class:`IsotonicCalibrator` -- a monotone map applied on the device (``cal(probs)``) and saved as the
integers it is made of.
"""
from __future__ import annotations

import json
import math
import statistics
from fractions import Fraction
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import call

_STATUS = ((1, "a probability is NaN"),
           (2, "a probability lies outside [0, 1]"),
           (4, "a label is neither 0.0 nor 1.0"),
           (8, "a key was not written by fbn_eval_pack (score bits above 1.0)"),
           (1 << 16, "a group id lies outside [0, 2^32)"))
_MAX_N = (1 << 31) - 1
_REC = 5                                         # int64 words of the ungrouped record + the status word


def gauc_from_table(table: Dict) -> Dict:
    """The three GAUC averages from the integer group table (``group_table()``'s dict, tensors or
    arrays), on the host in float64: ``AUC_g = u2 / (2 n_pos n_neg)`` per mixed group (both classes
    present), then ``gauc`` weighted by the group's samples, ``gauc_macro`` unweighted, ``gauc_clicks``
    weighted by its positives, each numerator summed with ``math.fsum``.  NaN without a mixed group.
    The reference for the device's sums, and the starting point for any other weighting."""
    def col(k):
        v = table[k]
        return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.int64)
    u2, n_pos, n_neg = col("u2"), col("n_pos"), col("n_neg")
    mixed = (n_pos > 0) & (n_neg > 0)
    u2, n_pos, n_neg = u2[mixed], n_pos[mixed], n_neg[mixed]
    n = n_pos + n_neg
    auc = u2.astype(np.float64) / (2 * n_pos * n_neg).astype(np.float64)     # exact integers: one IEEE division
    n_mixed, n_groups_mixed, clicks = int(n.sum()), int(mixed.sum()), int(n_pos.sum())
    nan = float("nan")
    return {"gauc": math.fsum(n.astype(np.float64) * auc) / n_mixed if n_groups_mixed else nan,
            "gauc_macro": math.fsum(auc) / n_groups_mixed if n_groups_mixed else nan,
            "gauc_clicks": math.fsum(n_pos.astype(np.float64) * auc) / clicks if n_groups_mixed else nan,
            "n_groups": int(len(mixed)), "n_groups_mixed": n_groups_mixed, "n_mixed": n_mixed}


_FX_ONE = 1 << 32                                # the fixed-point 1.0 of the calibration sums
_CALIB_COLS = ("n", "n_pos", "sum_p", "sum_p_pos", "sum_p2")


def _entropy(n: int, n_pos: int) -> float:
    """-(r ln r + (1 - r) ln(1 - r)) of the base rate r = n_pos / n; 0 for a single class, NaN for n == 0."""
    n, n_pos = int(n), int(n_pos)
    if n == 0:
        return float("nan")
    if n_pos == 0 or n_pos == n:
        return 0.0
    r, q = n_pos / n, (n - n_pos) / n            # both correctly rounded
    return -(r * math.log(r) + q * math.log(q))


def normalized_entropy(logloss: float, n: int, n_pos: int) -> float:
    """The log-loss over the entropy of the base rate n_pos / n (below 1: better than predicting the
    base rate everywhere).  NaN when the entropy is 0 (a single class) or n == 0."""
    h = _entropy(n, n_pos)
    return float(logloss) / h if h > 0.0 else float("nan")


def calibration_from_table(table: Dict) -> Dict:
    """The calibration scalars of a reliability table: ``table["width"]`` and ``table["mass"]`` (the
    equal-width and the equal-mass plane, as ``DeviceMetrics.calibration()`` returns them), each a dict
    of integer arrays of length B: n, n_pos, sum_p, sum_p_pos, sum_p2 with sum_p = sum of
    rint(p 2^32) and sum_p2 = sum of rint(p^2 2^32).  Python integers throughout: every result is an
    exact numerator over an exact denominator, divided once (int / int is correctly rounded).  With
    S = 2^32:
      ece      sum_b |n_pos_b S - sum_p_b| / (n S) over the width plane; ece_mass over the mass plane
      mce      max over the non-empty width bins of |n_pos_b S - sum_p_b| / (n_b S)
      pcoc     sum_p / (n_pos S): predicted over observed clicks; NaN without a positive
      brier    (sum_p2 - 2 sum_p_pos + n_pos S) / (n S)
      entropy  of the base rate n_pos / n; 0 for a single class
    All NaN when n == 0.  Needs no GPU."""
    def col(plane, k):
        v = table[plane][k]
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        return [int(x) for x in v.reshape(-1)]
    S = _FX_ONE
    w = {k: col("width", k) for k in _CALIB_COLS}
    m = {k: col("mass", k) for k in ("n", "n_pos", "sum_p")}
    B = len(w["n"])
    n, n_pos = sum(w["n"]), sum(w["n_pos"])
    out = {"bins": B, "n": n, "n_pos": n_pos}
    nan = float("nan")
    if n == 0:
        out.update(ece=nan, mce=nan, ece_mass=nan, pcoc=nan, brier=nan, entropy=nan)
        return out
    gap_w = [abs(a * S - b) for a, b in zip(w["n_pos"], w["sum_p"])]
    gap_m = [abs(a * S - b) for a, b in zip(m["n_pos"], m["sum_p"])]
    worst = max(Fraction(g, c * S) for g, c in zip(gap_w, w["n"]) if c)
    sum_p = sum(w["sum_p"])
    out.update(ece=sum(gap_w) / (n * S), mce=worst.numerator / worst.denominator, ece_mass=sum(gap_m) / (n * S),
               pcoc=sum_p / (n_pos * S) if n_pos else nan,
               brier=(sum(w["sum_p2"]) - 2 * sum(w["sum_p_pos"]) + n_pos * S) / (n * S),
               entropy=_entropy(n, n_pos))
    return out


_PAIR_STATUS = 1 << 17                           # fbn_delong_reduce: the two key sets' labels differ
_DELONG_SINGLE = ("auc_var", "auc_se", "ci_lo", "ci_hi")
_DELONG_PAIR = ("cov", "delta_var", "delta_se", "z", "p_value")


def _check_level(level) -> float:
    if isinstance(level, (bool, str)) or not isinstance(level, (int, float)) or not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must be a number in (0, 1), not {level!r}")
    return float(level)


def _delong_ints(rec):
    v = rec.detach().cpu().numpy() if isinstance(rec, torch.Tensor) else rec
    w = [int(x) for x in np.asarray(v, dtype=object).reshape(-1)[:_lib.FBN_DELONG_REC_WORDS]]
    if len(w) != _lib.FBN_DELONG_REC_WORDS or min(w) < 0:
        raise ValueError(f"a DeLong record is {_lib.FBN_DELONG_REC_WORDS} non-negative integers")
    m, n, ua, ub = w[:4]
    return m, n, ua, ub, w[4] + (w[5] << 32), w[6] + (w[7] << 32)


def _delong_cov(m: int, n: int, ua: int, ub: int, c10: int, c01: int) -> Fraction:
    """[(m C10 - Ua Ub)(n - 1) + (n C01 - Ua Ub)(m - 1)] / [4 m^2 n^2 (m - 1)(n - 1)], exact; m, n >= 2."""
    return Fraction((m * c10 - ua * ub) * (n - 1) + (n * c01 - ua * ub) * (m - 1),
                    4 * m * m * n * n * (m - 1) * (n - 1))


def _ratio(f: Fraction) -> float:
    return f.numerator / f.denominator           # int / int: correctly rounded, at any size


def delong_from_record(rec_aa, rec_bb=None, rec_ab=None, level: float = 0.95) -> Dict:
    """DeLong's variance of an AUC, and the paired test of two AUCs over the same samples, from the
    integer records of fbn_delong_reduce (``DeviceMetrics.auc_ci()["record"]``): 8 integers
    {n_pos, n_neg, sum_pos place_a, sum_pos place_b, low / high 32-bit part sums of sum_pos place_a place_b,
    the same over the negatives}.  Python integers throughout, one division per number; needs no GPU.

    One record (a set against itself): {"auc", "auc_var", "auc_se", "ci_lo", "ci_hi", "level", "n",
    "n_pos"}; the interval is auc -+ z se clipped to [0, 1], z the normal quantile of (1 + level) / 2.
    Three records (A against A, B against B, A against B): the above for A, plus {"auc_a", "auc_b",
    "delta" = auc_a - auc_b, "cov", "delta_var" = var_A + var_B - 2 cov, "delta_se", "z", "p_value"}
    (two-sided: erfc(|z| / sqrt 2)); delta_var == 0 gives z NaN and p_value 1.0.
    With fewer than 2 positives or 2 negatives every variance, se, bound, z and p is NaN; auc keeps
    compute()'s rule (0.5 for an empty class)."""
    level = _check_level(level)
    if (rec_bb is None) != (rec_ab is None):
        raise ValueError("delong_from_record takes one record, or three (A-A, B-B, A-B)")
    m, n, ua, ua2, c10, c01 = _delong_ints(rec_aa)
    if ua != ua2:
        raise ValueError("rec_aa is not the record of a set against itself")
    nan = float("nan")
    ok = m >= 2 and n >= 2
    auc = 0.5 if m == 0 or n == 0 else ua / (2 * m * n)
    out = {"auc": auc, "level": level, "n": m + n, "n_pos": m}
    out.update({k: nan for k in _DELONG_SINGLE})
    if ok:
        var_a = _delong_cov(m, n, ua, ua, c10, c01)
        zq = statistics.NormalDist().inv_cdf((1.0 + level) / 2.0)
        se = math.sqrt(_ratio(var_a))
        out.update(auc_var=_ratio(var_a), auc_se=se, ci_lo=max(0.0, auc - zq * se), ci_hi=min(1.0, auc + zq * se))
    if rec_bb is None:
        return out
    mb, nb, ub, ub2, d10, d01 = _delong_ints(rec_bb)
    mx, nx, xa, xb, e10, e01 = _delong_ints(rec_ab)
    if ub != ub2 or (mb, nb) != (m, n) or (mx, nx) != (m, n) or (xa, xb) != (ua, ub):
        raise ValueError("the three records do not describe the same samples (class counts or U2 differ)")
    out["auc_a"] = auc
    out["auc_b"] = 0.5 if m == 0 or n == 0 else ub / (2 * m * n)
    out["delta"] = 0.0 if m == 0 or n == 0 else (ua - ub) / (2 * m * n)
    out.update({k: nan for k in _DELONG_PAIR})
    if ok:
        cov = _delong_cov(m, n, ua, ub, e10, e01)
        dvar = var_a + _delong_cov(m, n, ub, ub, d10, d01) - 2 * cov       # one Fraction, divided once
        out.update(cov=_ratio(cov), delta_var=_ratio(dvar), delta_se=math.sqrt(_ratio(dvar)), p_value=1.0)
        if dvar > 0:
            z = out["delta"] / out["delta_se"]
            out.update(z=z, p_value=math.erfc(abs(z) / math.sqrt(2.0)))
    return out


_ISO_MODES = {"interp": 0, "step": 1}
_ISO_ONE_BITS = 0x3F800000                       # bits(1.0f): a key's score bits are at most this


class IsotonicCalibrator:
    """The exact isotonic fit of a set of (probability, label) samples (csrc/isotonic.hip):
    K blocks of consecutive scores [lo_j, hi_j] with n_j samples, n_pos_j of them positive; the block
    values n_pos_j / n_j increase strictly and lo_j <= hi_j < lo_{j+1}.  ``cal(probs)`` maps fp32
    probabilities on the device: a score inside a block gets the block's value, a score between two
    blocks the linear interpolation (``mode="step"``: the value of the next block up), a score below
    (above) every block the first (last) value -- sklearn's IsotonicRegression(out_of_bounds="clip").
    The map is non-decreasing, so a ranking changes by new ties only.

    ``blocks``: numpy lo, hi (float32) and n, n_pos (int64); ``table``: the device tensor the apply
    kernel reads (int64 words: K, then bits(lo) | bits(hi) << 32 and n | n_pos << 32 per block).
    Built by DeviceMetrics.isotonic(), from_dict() or load(); to_dict() / save() hold integers only."""

    def __init__(self, blocks: Dict, device=None):
        lo = np.ascontiguousarray(blocks["lo"], dtype=np.float32).reshape(-1)
        hi = np.ascontiguousarray(blocks["hi"], dtype=np.float32).reshape(-1)
        n = np.ascontiguousarray(blocks["n"], dtype=np.int64).reshape(-1)
        n_pos = np.ascontiguousarray(blocks["n_pos"], dtype=np.int64).reshape(-1)
        K = len(n)
        if K == 0:
            raise ValueError("IsotonicCalibrator: no blocks (fitted on no sample)")
        if not (len(lo) == len(hi) == len(n_pos) == K):
            raise ValueError("IsotonicCalibrator: lo, hi, n and n_pos differ in length")
        lb, hb = lo.view(np.uint32).astype(np.int64), hi.view(np.uint32).astype(np.int64)
        if lb.max() > _ISO_ONE_BITS or hb.max() > _ISO_ONE_BITS:
            raise ValueError("IsotonicCalibrator: a block score lies outside [0, 1]")
        if np.any(lb > hb) or np.any(hb[:-1] >= lb[1:]):
            raise ValueError("IsotonicCalibrator: the blocks are unsorted or overlap (need lo_j <= hi_j < lo_{j+1})")
        if np.any(n < 1) or np.any(n_pos < 0) or np.any(n_pos > n) or int(n.sum()) > _MAX_N:
            raise ValueError("IsotonicCalibrator: need 1 <= n_j, 0 <= n_pos_j <= n_j and fewer than 2^31 samples")
        if any(int(n_pos[j]) * int(n[j + 1]) >= int(n_pos[j + 1]) * int(n[j]) for j in range(K - 1)):
            raise ValueError("IsotonicCalibrator: the block values n_pos / n do not increase strictly")
        self.blocks = {"lo": lo, "hi": hi, "n": n, "n_pos": n_pos}
        for v in self.blocks.values():
            v.setflags(write=False)
        words = np.empty(2 * K + 1, dtype=np.int64)
        words[0] = K
        words[1::2] = lb | (hb << 32)
        words[2::2] = n | (n_pos << 32)
        self._words = words
        self.table: Optional[torch.Tensor] = None
        self.device: Optional[torch.device] = None
        if device is not None:
            self.to(device)

    def __len__(self) -> int:
        return len(self.blocks["n"])

    @property
    def values(self) -> np.ndarray:
        """The block values n_pos / n (float64, strictly increasing)."""
        return self.blocks["n_pos"].astype(np.float64) / self.blocks["n"].astype(np.float64)

    def to(self, device) -> "IsotonicCalibrator":
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("IsotonicCalibrator applies on a HIP device only (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.table is None or self.device != device:
            self.table = torch.from_numpy(self._words).to(device)
            self.device = device
        return self

    def apply(self, probs: torch.Tensor, mode: str = "interp", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The calibrated probabilities (float32, probs' shape): one launch, no host sync.  ``out``: a
        contiguous float32 tensor of the same size, or probs itself (in place).  NaN passes through."""
        if mode not in _ISO_MODES:
            raise ValueError(f"mode must be 'interp' or 'step', not {mode!r}")
        _lib.require_hip(probs, "probs")
        self.to(probs.device)
        p = probs.detach()
        if p.dtype != torch.float32 or not p.is_contiguous():
            if out is probs:
                raise ValueError("in-place apply needs a contiguous float32 tensor")
            p = p.to(torch.float32).contiguous()
        if out is None:
            out = torch.empty_like(p)
        else:
            _lib.require_hip(out, "out")
            if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != p.numel() or out.device != p.device:
                raise ValueError("out must be a contiguous float32 tensor of probs' size on probs' device")
        with torch.cuda.device(self.device):
            call("fbn_isotonic_apply", p.data_ptr(), p.numel(), self.table.data_ptr(), _ISO_MODES[mode], out.data_ptr(),
                 _lib.stream_handle(self.device))
        return out

    __call__ = apply

    def to_dict(self) -> Dict:
        """Integers only: the score bits and the counts (what save() writes)."""
        b = self.blocks
        return {"format": "fibinet-isotonic-1",
                "lo_bits": [int(v) for v in b["lo"].view(np.uint32)], "hi_bits": [int(v) for v in b["hi"].view(np.uint32)],
                "n": [int(v) for v in b["n"]], "n_pos": [int(v) for v in b["n_pos"]]}

    @classmethod
    def from_dict(cls, d: Dict, device=None) -> "IsotonicCalibrator":
        if not isinstance(d, dict) or d.get("format") != "fibinet-isotonic-1":
            raise ValueError("not an isotonic calibrator (format 'fibinet-isotonic-1' expected)")
        cols = []
        for k in ("lo_bits", "hi_bits", "n", "n_pos"):
            v = d.get(k)
            if not isinstance(v, list) or any(isinstance(x, bool) or not isinstance(x, int) or not 0 <= x < (1 << 32) for x in v):
                raise ValueError(f"isotonic calibrator: {k} must be a list of integers in [0, 2^32)")
            cols.append(v)
        lo, hi, n, n_pos = cols
        return cls({"lo": np.array(lo, dtype=np.uint32).view(np.float32), "hi": np.array(hi, dtype=np.uint32).view(np.float32),
                    "n": np.array(n, dtype=np.int64), "n_pos": np.array(n_pos, dtype=np.int64)}, device=device)

    def save(self, path: str) -> None:
        with open(path, "w") as fh:
            json.dump(self.to_dict(), fh)
            fh.write("\n")

    @classmethod
    def load(cls, path: str, device=None) -> "IsotonicCalibrator":
        with open(path) as fh:
            return cls.from_dict(json.load(fh), device=device)


class DeviceMetrics:
    """Streaming exact ROC-AUC + log-loss of up to ``capacity`` samples held as keys on ``device``;
    ``grouped``: also their group ids, for the per-group AUC."""

    def __init__(self, capacity: int, device=None, grouped: bool = False):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("DeviceMetrics runs on a HIP device only (no CPU fallback)")
        capacity = int(capacity)
        if not 0 <= capacity <= _MAX_N:
            raise ValueError(f"capacity must be in [0, 2^31), not {capacity}")
        self.capacity = capacity
        self.grouped = bool(grouped)
        # keys are below 2^31 (score bits < 2^30), so the int32 view orders as the uint32 keys do
        self.keys = torch.empty(max(1, capacity), dtype=torch.int32, device=self.device)
        # uint32 group ids (the int32 view holds their bits)
        self.gids = torch.empty(max(1, capacity), dtype=torch.int32, device=self.device) if self.grouped else None
        # {u64 U2, u64 n_pos, u64 n_neg, f64 logloss_sum} + the status word (+ the grouped record):
        # read back in one copy
        self.rec = self._new_rec()
        self.count = 0
        self._ws: Optional[torch.Tensor] = None
        self._gws: Optional[torch.Tensor] = None
        self._table: Optional[torch.Tensor] = None         # [n][4] int64 of the last grouped reduce
        self._table_rows: Optional[int] = None             # its G; None: stale
        self._cws: Optional[torch.Tensor] = None           # calibration(): workspace and table
        self._ctab: Optional[torch.Tensor] = None
        self._iws: Optional[torch.Tensor] = None           # isotonic(): workspace and table
        self._itab: Optional[torch.Tensor] = None
        self._pws: Optional[torch.Tensor] = None           # placements(): workspace and the uint32 placements
        self._place: Optional[torch.Tensor] = None

    def _new_rec(self) -> torch.Tensor:
        return torch.zeros(_REC + (_lib.FBN_GAUC_REC_WORDS if self.grouped else 0), dtype=torch.int64, device=self.device)

    # ------------------------------------------------------------------ streaming
    def reset(self) -> None:
        self.count = 0
        self.rec.zero_()
        self._table_rows = None

    def update(self, probs: torch.Tensor, labels: torch.Tensor, group_ids: Optional[torch.Tensor] = None) -> None:
        """Append a batch: one pack launch (two when grouped), no host sync (bad values surface in
        compute()).  group_ids: one integer id in [0, 2^32) per sample, of any integer dtype or a float
        tensor holding integers; required by a grouped instance, refused by any other."""
        _lib.require_hip(probs, "probs")
        _lib.require_hip(labels, "labels")
        n = probs.numel()
        if labels.numel() != n:
            raise ValueError(f"probs has {n} elements, labels {labels.numel()}")
        if self.grouped:
            if group_ids is None:
                raise ValueError("a grouped DeviceMetrics needs group_ids with every update()")
            _lib.require_hip(group_ids, "group_ids")
            if group_ids.numel() != n:
                raise ValueError(f"probs has {n} elements, group_ids {group_ids.numel()}")
        elif group_ids is not None:
            raise ValueError("group_ids given to a DeviceMetrics built without grouped=True")
        if self.count + n > self.capacity:
            raise ValueError(f"DeviceMetrics capacity {self.capacity} exceeded ({self.count} held + {n} new)")
        if n == 0:
            return
        p = probs.detach().reshape(-1).to(torch.float32).contiguous()
        y = labels.detach().reshape(-1).to(torch.float32).contiguous()
        with torch.cuda.device(self.device):
            call("fbn_eval_pack", p.data_ptr(), y.data_ptr(), n, self.keys.data_ptr() + 4 * self.count,
                 self.rec.data_ptr() + 32, _lib.stream_handle(self.device))
            if self.grouped:
                g = group_ids.detach().reshape(-1).to(torch.int64).contiguous()
                call("fbn_eval_pack_groups", g.data_ptr(), n, self.gids.data_ptr() + 4 * self.count,
                     self.rec.data_ptr() + 32, _lib.stream_handle(self.device))
        self.count += n
        self._table_rows = None

    # ------------------------------------------------------------------ result
    def _workspace(self, n: int) -> torch.Tensor:
        need = int(call("fbn_eval_workspace_size", n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _group_buffers(self, n: int):
        need = int(call("fbn_gauc_workspace_size", n))
        if self._gws is None or self._gws.numel() < need:
            self._gws = None
            self._gws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self._table is None or self._table.shape[0] < n:
            self._table = None
            self._table = torch.empty((max(1, n), 4), dtype=torch.int64, device=self.device)
        return self._gws, self._table

    @staticmethod
    def _check_status(word: int) -> None:
        status = int(word) & 0xFFFFFFFF
        if status:
            raise ValueError("DeviceMetrics: " + "; ".join(msg for bit, msg in _STATUS if status & bit))

    def _reduce(self, keys: torch.Tensor, n: int, rec: torch.Tensor, gids: Optional[torch.Tensor] = None) -> Dict:
        ws = self._workspace(n)
        with torch.cuda.device(self.device):
            call("fbn_eval_reduce", keys.data_ptr(), n, ws.data_ptr(), ws.numel(), rec.data_ptr(),
                 rec.data_ptr() + 32, _lib.stream_handle(self.device))
            if self.grouped:
                gws, table = self._group_buffers(n)
                call("fbn_gauc_reduce", keys.data_ptr(), gids.data_ptr(), n, gws.data_ptr(), gws.numel(),
                     table.data_ptr(), rec.data_ptr() + 8 * _REC, rec.data_ptr() + 32, _lib.stream_handle(self.device))
        self._table_rows = None
        host = rec.cpu().numpy()                 # the one device-to-host read: record(s) + status
        self._check_status(int(host[4]))
        u2, n_pos, n_neg = int(host[0]), int(host[1]), int(host[2])
        ll_sum = float(host[3:4].view(np.float64)[0])
        total = n_pos + n_neg
        auc = 0.5 if n_pos == 0 or n_neg == 0 else u2 / (2 * n_pos * n_neg)
        out = {"auc": auc, "logloss": ll_sum / total if total else float("nan"), "n": total, "n_pos": n_pos}
        if self.grouped:
            g = host[_REC:]
            n_groups, n_groups_mixed, n_mixed, clicks = int(g[0]), int(g[1]), int(g[2]), int(g[3])
            s_n, s_1, s_p = (float(v) for v in g[4:7].view(np.float64))
            nan = float("nan")
            out.update(gauc=s_n / n_mixed if n_groups_mixed else nan,
                       gauc_macro=s_1 / n_groups_mixed if n_groups_mixed else nan,
                       gauc_clicks=s_p / clicks if n_groups_mixed else nan,
                       n_groups=n_groups, n_groups_mixed=n_groups_mixed, n_mixed=n_mixed)
            self._table_rows = n_groups
        return out

    def group_table(self) -> Dict[str, torch.Tensor]:
        """{"group", "u2", "n_pos", "n_neg"}: int64 device tensors of length G, one entry per group in
        ascending id order -- the exact integers behind the last compute() (run now, over the samples
        held, if there was none since the last update()).  An analysis call: it reads G from the host."""
        if not self.grouped:
            raise ValueError("group_table() needs a DeviceMetrics built with grouped=True")
        if self._table_rows is None:
            self.compute()
        t = self._table[:self._table_rows]
        return {"group": t[:, 0].clone(), "u2": t[:, 1].clone(), "n_pos": t[:, 2].clone(), "n_neg": t[:, 3].clone()}

    def compute(self, group=None, stage_on_cpu: bool = False) -> Dict:
        """{"auc", "logloss", "n", "n_pos"} of the samples held (they stay: compute() can be repeated);
        grouped: plus {"gauc", "gauc_macro", "gauc_clicks", "n_groups", "n_groups_mixed", "n_mixed"}
        (the averages are NaN when no group holds both classes).

        group: a torch.distributed process group -- collective; every rank's keys (and group ids) are
        all-gathered (4 B each per sample, padded to the largest count) and reduced on every rank, in
        rank-major order: key order does not enter the AUC or the grouped numbers, and the log-loss
        tree sees the same sequence everywhere, so all ranks return identical numbers.
        stage_on_cpu: gather through host tensors (gloo)."""
        return self._reduce(*self._gather(group, stage_on_cpu))

    def _gather(self, group, stage_on_cpu: bool):
        """(keys, n, rec, gids) a reduce runs over: this instance's own, or with a process group every
        rank's, all-gathered in rank-major order (collective), with a fresh record holding the OR of the
        ranks' status words.  compute(group=) and calibration(group=) share it."""
        if group is None:
            return self.keys, self.count, self.rec, self.gids
        import torch.distributed as dist
        world = dist.get_world_size(group)
        counts = [None] * world
        dist.all_gather_object(counts, int(self.count), group=group)     # host-side ints
        maxc, total = max(counts), sum(counts)
        if total > _MAX_N:
            raise ValueError(f"{total} samples over the group: the device reduce needs n < 2^31")
        # one buffer per rank: its keys, padding, (its group ids, padding,) and its status word in the last slot
        cols = 2 if self.grouped else 1
        width = cols * maxc + 1
        send = torch.zeros(width, dtype=torch.int32, device=self.device)
        send[:self.count] = self.keys[:self.count]
        if self.grouped:
            send[maxc:maxc + self.count] = self.gids[:self.count]
        send[width - 1:] = self.rec.view(torch.int32)[8:9]
        if stage_on_cpu:
            parts = [torch.empty(width, dtype=torch.int32) for _ in range(world)]
            dist.all_gather(parts, send.cpu(), group=group)
            got = torch.stack(parts).to(self.device)
        else:
            got = torch.empty((world, width), dtype=torch.int32, device=self.device)
            dist.all_gather_into_tensor(got.view(-1), send, group=group)
        keys = torch.cat([got[r, :counts[r]] for r in range(world)]) if total else self.keys[:0]
        gids = None
        if self.grouped:
            gids = (torch.cat([got[r, maxc:maxc + counts[r]] for r in range(world)]) if total else self.gids[:0]).contiguous()
        rec = self._new_rec()
        status = got[0, width - 1:].clone()
        for r in range(1, world):
            status |= got[r, width - 1:]
        rec.view(torch.int32)[8:9] = status
        return keys.contiguous(), total, rec, gids

    @staticmethod
    def _check_bins(bins) -> int:
        if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= _lib.FBN_CALIB_MAX_BINS:
            raise ValueError(f"calibration bins must be an integer in [1, {_lib.FBN_CALIB_MAX_BINS}], not {bins!r}")
        return int(bins)

    def _calibrate(self, keys: torch.Tensor, n: int, rec: torch.Tensor, bins: int) -> Dict:
        need = int(call("fbn_calib_workspace_size", n))
        if self._cws is None or self._cws.numel() < need:
            self._cws = None
            self._cws = torch.empty(need, dtype=torch.uint8, device=self.device)
        words = 2 * bins * _lib.FBN_CALIB_BIN_WORDS + 1
        if self._ctab is None or self._ctab.numel() < words:
            self._ctab = torch.empty(words, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            call("fbn_calib_reduce", keys.data_ptr(), n, bins, self._cws.data_ptr(), self._cws.numel(),
                 self._ctab.data_ptr(), rec.data_ptr() + 32, _lib.stream_handle(self.device))
        host = self._ctab[:words].cpu().numpy()  # the one device-to-host read: both planes + status
        self._check_status(int(host[-1]))
        t = host[:-1].reshape(2, bins, _lib.FBN_CALIB_BIN_WORDS)
        planes = {}
        for k, name in enumerate(("width", "mass")):
            plane = {c: t[k, :, w].copy() for w, c in enumerate(_CALIB_COLS)}      # sums below 2^63: int64 holds them
            ends = t[k, :, 5].copy().view(np.uint32).reshape(bins, 2)              # little-endian: {p_min, p_max} bits
            empty = plane["n"] == 0
            for c, e in (("p_lo", 0), ("p_hi", 1)):
                v = ends[:, e].copy().view(np.float32)
                v[empty] = np.nan
                plane[c] = v
            planes[name] = plane
        out = calibration_from_table(planes)
        out.update(planes)
        return out

    def calibration(self, bins: int = 10, group=None, stage_on_cpu: bool = False) -> Dict:
        """The reliability table of the samples held (they stay: the call can be repeated with other
        bins, before or after compute()) and the calibration scalars derived from it (§20):
        {"bins", "n", "n_pos", "ece", "mce", "ece_mass", "pcoc", "brier", "entropy", "width", "mass"}.
        "width" (equal-width bins: min(B - 1, floor(p B)) in float64) and "mass" (equal-mass bins: ranks
        [floor(b n / B), floor((b + 1) n / B)) of the sorted keys, ties split with the negatives first)
        are dicts of numpy arrays of length B: n, n_pos, sum_p, sum_p_pos, sum_p2 (int64; the sums are of
        rint(p 2^32) and rint(p^2 2^32)) and p_lo, p_hi (float32; NaN for an empty bin).  Every number
        is exact and independent of the samples' order, the update sizes and the rank split; the scalars
        are calibration_from_table()'s.  One sort of the keys, one read.  Raises the ValueError compute()
        raises for the same status word.  group / stage_on_cpu: as in compute() (the same all-gather)."""
        bins = self._check_bins(bins)
        keys, n, rec, _ = self._gather(group, stage_on_cpu)
        return self._calibrate(keys, n, rec, bins)

    def compute_and_calibrate(self, bins: int, group=None, stage_on_cpu: bool = False):
        """(compute(), calibration(bins)) over one gather of the keys."""
        bins = self._check_bins(bins)
        keys, n, rec, gids = self._gather(group, stage_on_cpu)
        return self._reduce(keys, n, rec, gids), self._calibrate(keys, n, rec, bins)

    # ------------------------------------------------------------------ isotonic calibrator
    def _isotonic(self, keys: torch.Tensor, n: int, rec: torch.Tensor) -> IsotonicCalibrator:
        need = int(call("fbn_isotonic_workspace_size", n))
        if self._iws is None or self._iws.numel() < need:
            self._iws = None
            self._iws = torch.empty(need, dtype=torch.uint8, device=self.device)
        words = 2 * int(_lib.lib().fbn_isotonic_max_blocks(n)) + 2
        if self._itab is None or self._itab.numel() < words:
            self._itab = torch.empty(words, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            call("fbn_isotonic_fit", keys.data_ptr(), n, self._iws.data_ptr(), self._iws.numel(), self._itab.data_ptr(),
                 words, rec.data_ptr() + 32, _lib.stream_handle(self.device))
        host = self._itab[:words].cpu().numpy()  # the one device-to-host read: K, the blocks, the status word
        K = int(host[0])
        self._check_status(int(host[1 + 2 * K]))
        if K == 0:
            raise ValueError("DeviceMetrics.isotonic: no samples held")
        ends = host[1:1 + 2 * K:2].copy().view(np.uint32).reshape(K, 2)        # little-endian: {lo, hi} bits
        cnt = host[2:2 + 2 * K:2].copy().view(np.uint32).reshape(K, 2)         # {n, n_pos}
        return IsotonicCalibrator({"lo": ends[:, 0].copy().view(np.float32), "hi": ends[:, 1].copy().view(np.float32),
                                   "n": cnt[:, 0].astype(np.int64), "n_pos": cnt[:, 1].astype(np.int64)}, device=self.device)

    def isotonic(self, group=None, stage_on_cpu: bool = False) -> IsotonicCalibrator:
        """The exact isotonic fit of the samples held (they stay; compute() and calibration() are not
        affected) as an IsotonicCalibrator: pool-adjacent-violators pooling on >=, computed as the lower
        convex hull of the cumulative (samples, positives) diagram with 64-bit integers (§25).  One sort of
        the keys, one read; independent of the samples' order, the update sizes and the rank split.
        Raises the ValueError compute() raises for the same status word, and ValueError with no sample.
        group / stage_on_cpu: as in compute() (the same all-gather)."""
        keys, n, rec, _ = self._gather(group, stage_on_cpu)
        return self._isotonic(keys, n, rec)

    # ------------------------------------------------------------------ DeLong
    def _place_into(self, keys: torch.Tensor, n: int, rec: torch.Tensor) -> torch.Tensor:
        """fbn_auc_place over keys[:n] into this instance's placement buffer (the uint32 words as int32)."""
        need = int(call("fbn_auc_place_workspace_size", n))
        if self._pws is None or self._pws.numel() < need:
            self._pws = None
            self._pws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self._place is None or self._place.numel() < n:
            self._place = None
            self._place = torch.empty(max(1, n), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            call("fbn_auc_place", keys.data_ptr(), n, self._pws.data_ptr(), self._pws.numel(), self._place.data_ptr(),
                 rec.data_ptr() + 32, _lib.stream_handle(self.device))
        return self._place

    def placements(self) -> torch.Tensor:
        """The DeLong placement of every sample held, in the samples' own order (int64 device tensor of
        length ``count``): for a positive 2 * #negatives with a smaller score + #negatives with an equal
        score, for a negative 2 * #positives with a larger score + #positives with an equal score.  Their
        sum over either class is compute()'s U2.  The samples stay; bad values surface in compute() /
        auc_ci(), not here (no host read)."""
        place = self._place_into(self.keys, self.count, self.rec)
        return place[:self.count].to(torch.int64) & 0xFFFFFFFF

    def _delong_record(self, keys: torch.Tensor, n: int, rec: torch.Tensor):
        place = self._place_into(keys, n, rec)
        out = torch.empty(_lib.FBN_DELONG_REC_WORDS + 1, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            call("fbn_delong_reduce", keys.data_ptr(), place.data_ptr(), keys.data_ptr(), place.data_ptr(), n,
                 out.data_ptr(), rec.data_ptr() + 32, _lib.stream_handle(self.device))
        return out

    def _auc_ci(self, keys: torch.Tensor, n: int, rec: torch.Tensor, level: float) -> Dict:
        host = self._delong_record(keys, n, rec).cpu().numpy()      # the one device-to-host read: record + status
        self._check_status(int(host[-1]))
        record = [int(v) for v in host[:-1]]
        out = delong_from_record(record, level=level)
        out["record"] = record
        return out

    def auc_ci(self, level: float = 0.95, group=None, stage_on_cpu: bool = False) -> Dict:
        """DeLong's standard error and confidence interval of the AUC of the samples held (they stay):
        delong_from_record()'s {"auc", "auc_var", "auc_se", "ci_lo", "ci_hi", "level", "n", "n_pos"} plus
        "record", the 8 exact integers behind them.  One sort, one 72-byte read; independent of the
        samples' order, the update sizes and the rank split.  NaN (not an error) with fewer than 2
        samples of a class.  Raises the ValueError compute() raises for the same status word.
        group / stage_on_cpu: as in compute() (the same all-gather)."""
        level = _check_level(level)
        keys, n, rec, _ = self._gather(group, stage_on_cpu)
        return self._auc_ci(keys, n, rec, level)


def compare_auc(a: DeviceMetrics, b: DeviceMetrics, level: float = 0.95, group=None, stage_on_cpu: bool = False) -> Dict:
    """DeLong's paired test of two AUCs: ``a`` and ``b`` were fed the SAME samples in the same order (two
    checkpoints, compute modes or epochs over one validation split).  Returns delong_from_record()'s
    three-record dict -- a's interval plus {"auc_a", "auc_b", "delta", "cov", "delta_var", "delta_se",
    "z", "p_value"} -- and "records": {"aa", "bb", "ab"}, the exact integers.  Two sorts, three
    reduces, one read.  Unequal counts raise ValueError before any launch; labels that differ at any
    sample raise it after the read, as do the status bits compute() reports.  group: collective; both
    instances' keys are all-gathered in rank-major order, which keeps the pairs aligned."""
    level = _check_level(level)
    if a.count != b.count:
        raise ValueError(f"compare_auc needs the same samples in both: a holds {a.count}, b holds {b.count}")
    if a.device != b.device:
        raise ValueError(f"compare_auc: a is on {a.device}, b on {b.device}")
    ka, n, rec_a, _ = a._gather(group, stage_on_cpu)
    kb, nb, rec_b, _ = b._gather(group, stage_on_cpu)
    if n != nb:
        raise ValueError(f"compare_auc needs the same samples in both: a holds {n} over the group, b holds {nb}")
    W = _lib.FBN_DELONG_REC_WORDS + 1
    pa, pb = a._place_into(ka, n, rec_a), b._place_into(kb, n, rec_b)
    out = torch.empty(3 * W, dtype=torch.int64, device=a.device)
    pair = torch.zeros(2, dtype=torch.int32, device=a.device)      # the pair's own status word: the label mismatch
    with torch.cuda.device(a.device):
        st = _lib.stream_handle(a.device)
        call("fbn_delong_reduce", ka.data_ptr(), pa.data_ptr(), ka.data_ptr(), pa.data_ptr(), n,
             out.data_ptr(), rec_a.data_ptr() + 32, st)
        call("fbn_delong_reduce", kb.data_ptr(), pb.data_ptr(), kb.data_ptr(), pb.data_ptr(), n,
             out.data_ptr() + 8 * W, rec_b.data_ptr() + 32, st)
        call("fbn_delong_reduce", ka.data_ptr(), pa.data_ptr(), kb.data_ptr(), pb.data_ptr(), n,
             out.data_ptr() + 16 * W, pair.data_ptr(), st)
    host = out.cpu().numpy().reshape(3, W)       # the one device-to-host read: three records + status words
    a._check_status(int(host[0, -1]))
    b._check_status(int(host[1, -1]))
    if int(host[2, -1]) & _PAIR_STATUS:
        raise ValueError("compare_auc: the labels of a and b differ at some sample (label mismatch): the two "
                         "were not fed the same samples in the same order")
    recs = {k: [int(v) for v in host[r, :-1]] for r, k in enumerate(("aa", "bb", "ab"))}
    res = delong_from_record(recs["aa"], recs["bb"], recs["ab"], level=level)
    res["records"] = recs
    return res
