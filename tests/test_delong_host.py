"""DeLong's variance and paired test from the integer record (metrics.delong_from_record), on the host:
against the O(m n) float64 definition (tests/_delong_ref.brute), and at the corners -- identical sets,
degenerate class counts, sums past 2^64, bad levels.  No GPU.

Tolerance of the comparison with brute(): relative 1e-10.  brute()'s two-pass sums over N <= 2000 terms
are accurate to about N 2^-53 = 2e-13 relative, the record's numbers are correctly rounded: three orders
of margin, and any wrong term (a tie counted once, a missing m - 1) is off by far more.
"""
import math
import statistics

import numpy as np
import pytest

from tests import _delong_ref as R
from tests._calib_ref import scores

# (family, N) -> seed: the first seed that gives at least 2 samples of each class and placements that
# are not all equal ("ctr" has 4 % positives: at N = 7 most seeds have none).  "hundredths" is the
# heavily tied family: scores rounded to 2 decimals.
SEEDS = {("ctr", 7): 27, ("sevenths", 7): 4, ("edges", 7): 2, ("uniform", 7): 4, ("hundredths", 7): 2}
FAMILIES = ("ctr", "sevenths", "edges", "uniform", "hundredths")
REL = 1e-10


def _case(family, n):
    seed = SEEDS.get((family, n), 0)
    y, p = scores(family, n, seed)
    return y, p, R.noisy(p, 1000 * seed + n, sigma=0.3 if n == 7 else 0.02)         # 7 samples: enough noise to reorder them


def _from(y, pa, pb, level=0.95):
    from ctr_recommendation_amd.metrics import delong_from_record
    return delong_from_record(R.record(y, pa), R.record(y, pb), R.record(y, pa, pb), level=level)


@pytest.mark.parametrize("n", (7, 400, 2000))
@pytest.mark.parametrize("family", FAMILIES)
def test_record_numbers_equal_the_definition(family, n):
    from ctr_recommendation_amd.metrics import delong_from_record
    y, pa, pb = _case(family, n)
    m = int(y.sum())
    assert m >= 2 and n - m >= 2
    want = R.brute(y, pa, pb)
    assert want["auc_var"] > 0.0 and want["var_b"] > 0.0 and want["delta_var"] > 0.0
    got = _from(y, pa, pb)
    for k in ("auc_var", "cov", "delta_var"):
        assert abs(got[k] - want[k]) <= REL * abs(want[k]), (k, got[k], want[k])
    assert abs(got["auc_a"] - want["auc_a"]) <= 1e-14 and abs(got["auc_b"] - want["auc_b"]) <= 1e-14
    assert got["auc"] == got["auc_a"] and got["delta"] == pytest.approx(want["auc_a"] - want["auc_b"], abs=1e-14)
    one = delong_from_record(R.record(y, pb))                  # B alone: its variance is the pair's var_b
    assert abs(one["auc_var"] - want["var_b"]) <= REL * want["var_b"]
    assert one["auc_se"] == math.sqrt(one["auc_var"]) and got["delta_se"] == math.sqrt(got["delta_var"])
    assert got["z"] == got["delta"] / got["delta_se"]
    assert got["p_value"] == math.erfc(abs(got["z"]) / math.sqrt(2.0)) and 0.0 <= got["p_value"] <= 1.0
    assert set(one) == {"auc", "auc_var", "auc_se", "ci_lo", "ci_hi", "level", "n", "n_pos"}
    assert set(got) == set(one) | {"auc_a", "auc_b", "delta", "cov", "delta_var", "delta_se", "z", "p_value"}


@pytest.mark.parametrize("level", (0.5, 0.9, 0.95, 0.999))
def test_interval_is_auc_plus_minus_z_se_clipped(level):
    from ctr_recommendation_amd.metrics import delong_from_record
    y, p, _ = _case("uniform", 400)
    out = delong_from_record(R.record(y, p), level=level)
    z = statistics.NormalDist().inv_cdf((1.0 + level) / 2.0)
    assert out["level"] == level and out["n"] == 400 and out["n_pos"] == int(y.sum())
    assert out["ci_lo"] == max(0.0, out["auc"] - z * out["auc_se"]) and out["ci_hi"] == min(1.0, out["auc"] + z * out["auc_se"])
    assert 0.0 <= out["ci_lo"] < out["auc"] < out["ci_hi"] <= 1.0
    # a near-perfect ranking: the upper bound is clipped at 1
    yy = np.array([0, 0, 0, 1, 1, 1, 0, 1], dtype=np.float32)
    pp = np.array([.1, .2, .3, .6, .7, .8, .65, .9], dtype=np.float32)
    out = delong_from_record(R.record(yy, pp), level=level)
    assert out["auc"] == 15 / 16 and out["ci_hi"] == min(1.0, out["auc"] + z * out["auc_se"]) and out["ci_hi"] <= 1.0


@pytest.mark.parametrize("family", FAMILIES)
def test_placements_sum_to_u2_in_both_classes(family):
    from ctr_recommendation_amd.utils import compute_auc
    y, p, _ = _case(family, 400)
    pl = R.placements(y, p)
    m = int(y.sum())
    n = len(y) - m
    u2 = int(pl[y == 1].sum())
    assert u2 == int(pl[y != 1].sum()) == R.record(y, p)[2]
    assert 0 <= pl.min() and pl[y == 1].max() <= 2 * n and pl[y != 1].max() <= 2 * m
    assert u2 / (2 * m * n) == pytest.approx(compute_auc(y, p), abs=1e-15)


def test_a_set_against_itself_has_no_difference():
    y, p, _ = _case("hundredths", 400)
    out = _from(y, p, p)
    assert out["delta"] == 0.0 and out["delta_var"] == 0.0 and out["delta_se"] == 0.0
    assert math.isnan(out["z"]) and out["p_value"] == 1.0
    assert out["cov"] == out["auc_var"] > 0.0


@pytest.mark.parametrize("m,n", ((0, 5), (5, 0), (1, 5), (5, 1), (0, 0), (1, 1)))
def test_degenerate_class_counts_give_nan(m, n):
    y = np.array([1] * m + [0] * n, dtype=np.float32)
    p = np.linspace(0.9, 0.1, m + n).astype(np.float32)
    out = _from(y, p, p[::-1].copy())
    for k in ("auc_var", "auc_se", "ci_lo", "ci_hi", "cov", "delta_var", "delta_se", "z", "p_value"):
        assert math.isnan(out[k]), (k, out[k])
    assert out["n"] == m + n and out["n_pos"] == m
    if m == 0 or n == 0:
        assert out["auc"] == out["auc_a"] == out["auc_b"] == 0.5 and out["delta"] == 0.0
    else:
        assert out["auc_a"] == 1.0 and out["auc_b"] == 0.0 and out["delta"] == 1.0


def test_sums_past_2_to_64_reassemble():
    """m = n = 2^21, every positive at 1.0 and every negative at 0.0: the record built arithmetically."""
    from ctr_recommendation_amd.metrics import delong_from_record
    m = n = 1 << 21
    rec = R.closed_form(m, n)
    assert rec[4] + (rec[5] << 32) == m * 4 * n * n > 1 << 64
    assert rec[6] + (rec[7] << 32) == n * 4 * m * m
    assert all(0 <= w < 1 << 63 for w in rec)
    out = delong_from_record(rec)
    assert out["auc"] == 1.0 and out["auc_var"] == 0.0 and out["auc_se"] == 0.0
    assert out["ci_lo"] == out["ci_hi"] == 1.0 and out["n"] == 2 * m and out["n_pos"] == m
    pair = delong_from_record(rec, rec, rec)
    assert pair["delta"] == 0.0 and pair["delta_var"] == 0.0 and pair["p_value"] == 1.0 and math.isnan(pair["z"])


@pytest.mark.parametrize("level", (0, 1, 1.5, "x", -0.1, None, True))
def test_invalid_level_raises(level):
    from ctr_recommendation_amd.metrics import delong_from_record
    y, p, _ = _case("uniform", 7)
    with pytest.raises(ValueError, match="level"):
        delong_from_record(R.record(y, p), level=level)


def test_records_of_different_samples_are_refused():
    from ctr_recommendation_amd.metrics import delong_from_record
    y, pa, pb = _case("uniform", 400)
    y2, p2, _ = _case("ctr", 400)
    with pytest.raises(ValueError, match="same samples"):
        delong_from_record(R.record(y, pa), R.record(y2, p2), R.record(y, pa, pb))
    with pytest.raises(ValueError, match="three"):
        delong_from_record(R.record(y, pa), R.record(y, pb))
