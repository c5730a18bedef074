"""Host side of the device metrics (no GPU): the workspace query, the argument guards that return
before any launch, and the integer AUC formulation the kernels implement, against utils.compute_auc."""
import ctypes

import numpy as np
import pytest

from ctr_recommendation_amd.utils import compute_auc


def test_workspace_query_is_host_only_and_grows_with_n():
    from ctr_recommendation_amd import _lib
    h = _lib.lib()
    base = h.fbn_eval_workspace_size(0)
    assert base > 0 and base % 256 == 0
    assert h.fbn_eval_workspace_size(1) == base + 256            # 2 B per sample, 256-B granules
    assert h.fbn_eval_workspace_size(1 << 20) == base + (2 << 20)
    assert h.fbn_eval_workspace_size(-5) == base


def test_reduce_and_pack_refuse_bad_arguments_before_launching():
    from ctr_recommendation_amd import _lib
    h = _lib.lib()
    rec = (ctypes.c_ulonglong * 5)()
    out = ctypes.addressof(rec)
    assert h.fbn_eval_reduce(None, 1 << 31, None, 0, out, None, None) == 1      # n must stay below 2^31
    assert b"2^31" in h.fbn_last_error()
    assert h.fbn_eval_reduce(None, -1, None, 0, out, None, None) == 1
    assert h.fbn_eval_reduce(None, 8, None, 0, None, None, None) == 1          # no record
    assert h.fbn_eval_reduce(None, 8, None, 0, out, None, None) == 1           # no keys / workspace
    assert h.fbn_eval_pack(None, None, 8, None, None, None) == 1
    assert h.fbn_eval_pack(None, None, 1 << 31, out, out, None) == 1
    assert h.fbn_eval_pack(None, None, 0, None, None, None) == 0               # nothing to pack


def test_device_metrics_needs_a_hip_device():
    from ctr_recommendation_amd.metrics import DeviceMetrics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceMetrics(8, "cpu")


def _auc_from_keys(y, p):
    """The kernels' formulation on the host: keys, integer U2, Python int / int."""
    p = np.asarray(p, dtype=np.float32)
    bits = np.where(p == 0, 0, p.view(np.uint32)).astype(np.uint64)
    yb = (np.asarray(y) == 1).astype(np.uint64)
    score = np.sort(bits[yb == 0])
    pos = bits[yb == 1]
    n_pos, n_neg = int(len(pos)), int(len(score))
    if n_pos == 0 or n_neg == 0:
        return 0.5
    less = np.searchsorted(score, pos, side="left")
    leq = np.searchsorted(score, pos, side="right")
    u2 = int((2 * less + (leq - less)).sum())
    return u2 / (2 * n_pos * n_neg)


@pytest.mark.parametrize("n", (1, 2, 65, 4099, 70001))
def test_integer_formulation_is_bitwise_compute_auc(n):
    rng = np.random.default_rng(n)
    y = (rng.random(n) < 0.17).astype(np.float32)
    with np.errstate(over="ignore"):
        fams = [rng.random(n, dtype=np.float32), (rng.integers(0, 7, n) / 6.0).astype(np.float32),
                np.full(n, 0.5, np.float32), (0.5 + rng.integers(0, 4096, n) * 2.0 ** -24).astype(np.float32),
                (1.0 / (1.0 + np.exp(-rng.normal(0, 30, n)))).astype(np.float32)]
    for p in fams:
        assert _auc_from_keys(y, p) == compute_auc(y, p)
