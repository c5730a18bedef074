"""The weighted training loss of the head (include/fibinet.h, fbn_head_fwd_w) in float64 torch.

With o the logit, p = sigmoid(o), t the label, w the sample weight (1 if absent), pi = pos_weight,
eps = label_smoothing and n the step's global sample count:

    t~     = t (1 - eps) + eps / 2
    term_i = w_i * -(pi t~_i max(log p_i, -100) + (1 - t~_i) max(log(1 - p_i), -100))
    loss   = sum_i term_i / n            (a mean over samples, not divided by sum w: BCELoss(weight=))
    num_i  = (1 - t~_i) p_i - pi t~_i (1 - p_i)
    gout_i = (w_i num_i / max(p_i (1 - p_i), 1e-12) / n) * p_i (1 - p_i)

The -100 clamp of the logs and the 1e-12 clamp of ATen's BCELoss backward are written out: dL/dp is the
clamped formula, and gout = dL/do comes from autograd through p = sigmoid(o).
"""
import torch


def smooth(t: torch.Tensor, eps: float) -> torch.Tensor:
    return t * (1.0 - eps) + eps / 2.0


def weighted_bce(o: torch.Tensor, t: torch.Tensor, w=None, pos_weight: float = 1.0, label_smoothing: float = 0.0,
                 n=None):
    """(terms [B], gout [B], p [B]) in float64 from logits o, labels t, weights w (None: ones)."""
    o = o.detach().double().clone().requires_grad_(True)
    t = t.detach().double()
    w = torch.ones_like(t) if w is None else w.detach().double()
    n = float(o.numel() if n is None else n)
    p = torch.sigmoid(o)
    ts = smooth(t, float(label_smoothing))
    a, b = float(pos_weight) * ts, 1.0 - ts
    lp = torch.log(p).clamp(min=-100.0)
    l1p = torch.log(1.0 - p).clamp(min=-100.0)
    terms = w * -(a * lp + b * l1p)
    pd = p.detach()
    num = b * pd - a * (1.0 - pd)
    dl_dp = w * num / (pd * (1.0 - pd)).clamp(min=1e-12) / n
    p.backward(dl_dp)                       # sigmoid backward: gout = dL/dp * p (1 - p)
    return terms.detach(), o.grad.detach(), pd
