"""Host side of the grouped AUC and the device sort (no GPU): the workspace queries, the argument
guards that return before any launch, and metrics.gauc_from_table over the integer group table
against compute_auc run per group."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from ctr_recommendation_amd.utils import compute_auc
from tests import _gauc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_mirror_the_header():
    from ctr_recommendation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fibinet.h")).read()
    assert int(re.search(r"#define FBN_SORT_TILE (\d+)", hdr).group(1)) == _lib.FBN_SORT_TILE
    assert int(re.search(r"#define FBN_GAUC_REC_WORDS (\d+)", hdr).group(1)) == _lib.FBN_GAUC_REC_WORDS
    scan = open(os.path.join(ROOT, "ctr_recommendation_amd", "csrc", "scan.h")).read()
    # the kernels take the tile from the header (common.h includes it): no second definition to drift
    assert not re.search(r"#\s*define\s+FBN_SORT_TILE\b", scan)


@pytest.mark.parametrize("query", ("fbn_sort_u64_workspace_size", "fbn_gauc_workspace_size"))
def test_workspace_queries_are_host_only_granular_and_monotone(query):
    from ctr_recommendation_amd import _lib
    f = getattr(_lib.lib(), query)
    T = _lib.FBN_SORT_TILE
    sizes = [f(n) for n in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 70001, 1 << 20, (1 << 31) - 1)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[0] < sizes[-3] < sizes[-2] < sizes[-1]
    assert f(-5) == f(0)
    assert f(1 << 20) >= 8 << 20                                   # at least one buffer of the keys


def test_gauc_workspace_holds_the_sort_workspace():
    from ctr_recommendation_amd import _lib
    h = _lib.lib()
    for n in (0, 1, 4099, 70001, 1 << 20):
        assert h.fbn_gauc_workspace_size(n) >= h.fbn_sort_u64_workspace_size(n) + 16 * n


def test_entry_points_refuse_bad_arguments_before_launching():
    from ctr_recommendation_amd import _lib
    h = _lib.lib()
    buf = (ctypes.c_ulonglong * 64)()
    a = ctypes.addressof(buf)                                      # a host address: the guards never touch it
    err = lambda: h.fbn_last_error()                               # noqa: E731
    # fbn_sort_u64
    assert h.fbn_sort_u64(a, 1 << 31, 63, a + 256, 1 << 40, a + 128, None) == 1 and b"fbn_sort_u64" in err() and b"2^31" in err()
    assert h.fbn_sort_u64(a, -1, 63, a + 256, 1 << 40, a + 128, None) == 1
    assert h.fbn_sort_u64(a, 8, 0, a + 256, 1 << 40, a + 128, None) == 1 and b"bits" in err()
    assert h.fbn_sort_u64(a, 8, 65, a + 256, 1 << 40, a + 128, None) == 1 and b"bits" in err()
    assert h.fbn_sort_u64(None, 8, 63, a + 256, 1 << 40, a + 128, None) == 1 and b"fbn_sort_u64" in err()
    assert h.fbn_sort_u64(a, 8, 63, a + 256, 1 << 40, None, None) == 1
    assert h.fbn_sort_u64(a, 8, 63, None, 1 << 40, a + 128, None) == 1
    assert h.fbn_sort_u64(a, 8, 63, a + 256, 1 << 40, a, None) == 1                       # out is in
    assert h.fbn_sort_u64(a, 8, 63, a + 260, 1 << 40, a + 128, None) == 1                 # misaligned workspace
    assert h.fbn_sort_u64(a, 8, 63, a + 256, h.fbn_sort_u64_workspace_size(8) - 1, a + 128, None) == 1
    assert b"fbn_sort_u64_workspace_size" in err()
    assert h.fbn_sort_u64(None, 0, 63, None, 0, None, None) == 0                          # nothing to sort
    # fbn_eval_pack_groups
    assert h.fbn_eval_pack_groups(None, 8, None, None, None) == 1 and b"fbn_eval_pack_groups" in err()
    assert h.fbn_eval_pack_groups(a, 1 << 31, a, a, None) == 1 and b"2^31" in err()
    assert h.fbn_eval_pack_groups(None, 0, None, None, None) == 0
    # fbn_gauc_reduce
    big = 1 << 40
    assert h.fbn_gauc_reduce(a, a, 1 << 31, a + 256, big, a, a, a, None) == 1 and b"fbn_gauc_reduce" in err() and b"2^31" in err()
    assert h.fbn_gauc_reduce(a, a, -1, a + 256, big, a, a, a, None) == 1
    assert h.fbn_gauc_reduce(a, a, 8, a + 256, big, a, None, a, None) == 1 and b"fbn_gauc_reduce" in err()   # no record
    assert h.fbn_gauc_reduce(a, a, 8, a + 256, big, a, a + 4, a, None) == 1               # misaligned record
    assert h.fbn_gauc_reduce(None, a, 8, a + 256, big, a, a, a, None) == 1
    assert h.fbn_gauc_reduce(a, None, 8, a + 256, big, a, a, a, None) == 1
    assert h.fbn_gauc_reduce(a, a, 8, None, big, a, a, a, None) == 1
    assert h.fbn_gauc_reduce(a, a, 8, a + 256, big, None, a, a, None) == 1
    assert h.fbn_gauc_reduce(a, a, 8, a + 256, big, a, a, None, None) == 1
    assert h.fbn_gauc_reduce(a, a, 8, a + 260, big, a, a, a, None) == 1                   # misaligned workspace
    assert h.fbn_gauc_reduce(a, a, 8, a + 256, h.fbn_gauc_workspace_size(8) - 1, a, a, a, None) == 1
    assert b"fbn_gauc_workspace_size" in err()


def test_grouped_device_metrics_needs_a_hip_device():
    from ctr_recommendation_amd.metrics import DeviceMetrics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceMetrics(8, "cpu", grouped=True)


@pytest.mark.parametrize("n", (1, 2, 65, 4099, 70001))
@pytest.mark.parametrize("gfam", R.GROUPS)
@pytest.mark.parametrize("sfam", R.SCORES)
def test_gauc_from_table_against_per_group_compute_auc(sfam, gfam, n):
    from ctr_recommendation_amd.metrics import gauc_from_table
    y, p, ids, table = R.case(sfam, gfam, n)
    out = gauc_from_table(table)
    gid, auc = R.direct_auc(y, p, ids)
    # the same groups, and on every mixed one the integer AUC is the double compute_auc's arithmetic gives
    assert np.array_equal(gid, table["group"]) and np.all(np.diff(gid) > 0)
    assert int(table["n_pos"].sum()) == int(y.sum()) and int((table["n_pos"] + table["n_neg"]).sum()) == n
    mixed = (table["n_pos"] > 0) & (table["n_neg"] > 0)
    assert np.array_equal(mixed, ~np.isnan(auc))
    for k in np.flatnonzero(mixed):
        a_int = int(table["u2"][k]) / (2 * int(table["n_pos"][k]) * int(table["n_neg"][k]))
        assert a_int == auc[k]
    # compute_auc itself on a few groups (the largest, the first and the last mixed ones): direct_auc is its arithmetic
    if mixed.any():
        big = int(np.argmax(np.where(mixed, table["n_pos"] + table["n_neg"], 0)))
        for k in {big, int(np.flatnonzero(mixed)[0]), int(np.flatnonzero(mixed)[-1])}:
            sel = ids == gid[k]
            assert compute_auc(y[sel], p[sel]) == auc[k]
    # the averages
    assert out["n_groups"] == len(gid) and out["n_groups_mixed"] == int(mixed.sum())
    npos, nneg, a = table["n_pos"][mixed], table["n_neg"][mixed], auc[mixed]
    assert out["n_mixed"] == int((npos + nneg).sum())
    if not mixed.any():
        assert all(math.isnan(out[k]) for k in ("gauc", "gauc_macro", "gauc_clicks"))
        return
    assert out["gauc"] == math.fsum((npos + nneg).astype(np.float64) * a) / int((npos + nneg).sum())
    assert out["gauc_macro"] == math.fsum(a) / len(a)
    assert out["gauc_clicks"] == math.fsum(npos.astype(np.float64) * a) / int(npos.sum())
    if gfam == "one":
        whole = compute_auc(y, p)
        assert out["gauc_macro"] == whole and out["gauc_clicks"] == float(np.float64(npos[0]) * whole) / int(npos[0])
        assert out["gauc"] == float(np.float64(n) * whole) / n


def test_group_families_have_the_shapes_the_gpu_tests_rely_on():
    _, _, ids, table = R.case("uniform", "small", 70001)
    mixed = (table["n_pos"] > 0) & (table["n_neg"] > 0)
    assert 8000 < len(table["group"]) <= 70001 // 8 and 0.6 < mixed.mean() < 0.9
    _, _, ids, table = R.case("uniform", "wide", 70001)
    assert {0, 1 << 31, (1 << 32) - 1} <= set(table["group"].tolist()) and len(table["group"]) > 4000
    b = table["group"].astype(np.uint64).view(np.uint8).reshape(-1, 8)[:, :4]
    assert all(len(np.unique(b[:, k])) > 200 for k in range(4))    # every digit pass of the id moves keys
    _, _, ids, table = R.case("uniform", "skewed", 70001)
    mixed = (table["n_pos"] > 0) & (table["n_neg"] > 0)
    assert int((table["n_pos"] + table["n_neg"]).max()) > 65535 and int(mixed.sum()) > 100
    _, _, ids, table = R.case("uniform", "singletons", 70001)
    assert len(table["group"]) == 70001
