"""tests/_loss_ref.py (the float64 definition of the weighted head loss) against torch's own losses on
unsaturated logits, where neither clamp engages: BCELoss(weight=), BCEWithLogitsLoss(pos_weight=), both
with smoothed targets, their autograd gradients, and the neutral-options identity num == p - t."""
import torch
import torch.nn.functional as F

from tests._loss_ref import smooth, weighted_bce


def _data(B=300, seed=3):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(B, generator=g, dtype=torch.float64) * 2 - 1) * 12      # |o| <= 12: log p > -100, p(1-p) > 1e-12
    t = (torch.rand(B, generator=g) < 0.3).double()
    w = torch.rand(B, generator=g, dtype=torch.float64) * 5
    w[::7] = 0.0
    return o, t, w


def _close(a, b, tol=1e-12):
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


def test_equals_bce_with_sample_weights():
    o, t, w = _data()
    n = o.numel()
    terms, gout, p = weighted_bce(o, t, w)
    _close(terms, F.binary_cross_entropy(torch.sigmoid(o), t, weight=w, reduction="none"))
    oo = o.clone().requires_grad_(True)
    loss = F.binary_cross_entropy(torch.sigmoid(oo), t, weight=w)            # a mean over samples, not / sum(w)
    loss.backward()
    _close(terms.sum() / n, loss.detach())
    _close(gout, oo.grad)


def test_equals_bce_with_logits_pos_weight():
    o, t, w = _data()
    for pi in (0.25, 1.0, 7.5):
        terms, gout, _ = weighted_bce(o, t, None, pos_weight=pi)
        oo = o.clone().requires_grad_(True)
        ref = F.binary_cross_entropy_with_logits(oo, t, pos_weight=torch.tensor(pi, dtype=torch.float64),
                                                 reduction="none")
        _close(terms, ref.detach(), 1e-10)      # (log-sum-exp form against log(sigmoid): 1e-10 of the largest term)
        (ref.sum() / o.numel()).backward()
        _close(gout, oo.grad, 1e-10)


def test_label_smoothing_and_all_options():
    o, t, w = _data()
    n = 2 * o.numel()                                                        # a global count above the local one
    for eps in (0.1, 0.5):
        ts = smooth(t, eps)
        assert ts.min().item() == eps / 2 and abs(ts.max().item() - (1 - eps / 2)) < 1e-15
        terms, gout, _ = weighted_bce(o, t, w, label_smoothing=eps, n=n)
        oo = o.clone().requires_grad_(True)
        ref = F.binary_cross_entropy(torch.sigmoid(oo), ts, weight=w, reduction="none")
        _close(terms, ref.detach())
        (ref.sum() / n).backward()
        _close(gout, oo.grad)
        for pi in (0.25, 7.5):
            terms, gout, _ = weighted_bce(o, t, w, pos_weight=pi, label_smoothing=eps, n=n)
            oo = o.clone().requires_grad_(True)
            ref = w * F.binary_cross_entropy_with_logits(oo, ts, pos_weight=torch.tensor(pi, dtype=torch.float64),
                                                         reduction="none")
            _close(terms, ref.detach(), 1e-10)
            (ref.sum() / n).backward()
            _close(gout, oo.grad, 1e-10)


def test_clamps_at_saturation():
    o = torch.tensor([120.0, -120.0, 120.0, -120.0], dtype=torch.float64)
    t = torch.tensor([1.0, 0.0, 0.0, 1.0], dtype=torch.float64)
    terms, gout, p = weighted_bce(o, t, None, pos_weight=3.0)
    assert terms.tolist() == [0.0, 0.0, 100.0, 300.0]                        # max(log, -100), the positive term x pi
    assert gout.abs().max().item() < 1e-30                                  # p (1 - p) underflows: no gradient


def test_neutral_options_numerator_is_p_minus_t():
    """pi = 1, eps = 0, t in {0, 1}: (1 - t~) p - pi t~ (1 - p) == p - t bit for bit, in both formats
    (at t = 1 it is -(1 - p), the exact negation of p - 1)."""
    g = torch.Generator().manual_seed(5)
    for dt in (torch.float32, torch.float64):
        p = torch.sigmoid(torch.randn(4096, generator=g, dtype=dt) * 6)
        p[:4] = torch.tensor([0.0, 1.0, 0.5, 1.0 - 2.0 ** -24 if dt == torch.float32 else 1.0 - 2.0 ** -53], dtype=dt)
        for tv in (0.0, 1.0):
            t = torch.full_like(p, tv)
            ts = smooth(t, 0.0)
            assert torch.equal(ts, t)
            num = (1.0 - ts) * p - 1.0 * ts * (1.0 - p)
            assert torch.equal(num, p - t)
