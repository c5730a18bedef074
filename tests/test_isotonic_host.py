"""Host tests of the isotonic calibrator: the reference against the integer-hull definition,
the block-count bound, the apply rule's properties, the C ABI's guards and queries (no device work: every
refusal precedes it), and the calibrator's JSON form.  No GPU."""
import json

import numpy as np
import pytest

from tests import _isotonic_ref as R

SMALL = ("farey:8", "farey:40", "farey_repeat:16,40", "distinct_convex:24", "distinct_blocks:24",
         "separable:1", "separable:2", "separable:1025", "reversed:1", "reversed:1025", "all_pos:300", "all_neg:300")
CASES = [(f, n) for f in R.CALIB_FAMILIES for n in (1, 2, 65, 2049)] + [(f, None) for f in SMALL]


def _lib():
    from ctr_recommendation_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("family,n", CASES)
def test_reference_equals_the_integer_hull(family, n):
    y, p, ref = R.case(family, n)
    assert R.same_blocks(R.hull_ref(y, p), ref) is None
    K = len(ref["n"])
    assert int(ref["n"].sum()) == len(y) and int(ref["n_pos"].sum()) == int(y.sum())
    assert all(R.rate(ref, j) < R.rate(ref, j + 1) for j in range(K - 1))          # strictly increasing values
    assert np.all(ref["lo"] <= ref["hi"]) and np.all(ref["hi"][:-1] < ref["lo"][1:])
    assert K <= R.max_blocks(len(y))


def test_named_families_have_the_blocks_they_are_built_for():
    assert len(R.case("farey:8")[2]["n"]) == len(R.farey_sequence(8)) == 23       # every group is a block
    assert len(R.case("farey:40")[2]["n"]) == 491 and len(R.case("farey:40")[0]) == 13112
    assert len(R.case("distinct_blocks:24")[2]["n"]) == len(R.farey_sequence(24))  # every piece of distinct scores is a block
    assert len(R.case("separable:1025")[2]["n"]) == 2 and len(R.case("reversed:1025")[2]["n"]) == 1
    assert len(R.case("all_pos:300")[2]["n"]) == 1 and len(R.case("all_neg:300")[2]["n"]) == 1
    y, p, ref = R.case("distinct_convex:24")                                       # all scores distinct: G = n
    assert len(np.unique(p)) == len(p) and len(ref["n"]) == len(R.hull_ref(y, p)["n"]) == 61


def test_block_bound_query():
    h = _lib()
    for n in list(range(0, 300)) + [13112, 54068, 70001, 10 ** 6, 2 ** 31 - 1]:
        assert h.fbn_isotonic_max_blocks(n) == R.max_blocks(n), n
    assert h.fbn_isotonic_max_blocks(-5) == R.max_blocks(0) == 2
    assert [R.max_blocks(n) for n in (13112, 54068, 70001)] == [580, 1489, 1768]
    # the count argument behind the bound: denominators in ascending order, phi(b) rates of b samples each
    for n in list(range(0, 3000)) + [13112, 54068, 70001, 10 ** 6]:
        assert R.max_blocks_exact(n) <= R.max_blocks(n), n
    y, _, ref = R.case("farey:64")                                                 # and it is nearly attained
    K, bound = len(ref["n"]), R.max_blocks(len(y))
    assert (len(y), K, bound) == (54068, 1261, 1489) and K == R.max_blocks_exact(len(y)) and K >= 0.8 * bound


def test_workspace_query():
    h = _lib()
    sizes = [h.fbn_isotonic_workspace_size(n) for n in (0, 1, 1024, 1025, 70001, 10 ** 6)]
    assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    assert h.fbn_isotonic_workspace_size(-3) == sizes[0]
    assert sizes[-1] >= 10 ** 6 * 32                       # widened + sorted keys + two point buffers
    assert sizes[-1] <= 10 ** 6 * 40 + h.fbn_sort_u64_workspace_size(10 ** 6)


def test_fit_guards_precede_device_work():
    """Every refusal names the function and returns FBN_ERR_ARG with nothing launched: the pointers are
    made-up addresses and there is no device here."""
    h = _lib()
    n = 1000
    ws = h.fbn_isotonic_workspace_size(n)
    words = 2 * h.fbn_isotonic_max_blocks(n) + 2
    A = 1 << 20                                            # an aligned, never dereferenced address
    good = dict(keys=A, n=n, ws=A, ws_bytes=ws, table=A, words=words, status=A)

    def fit(**kw):
        a = dict(good, **kw)
        rc = h.fbn_isotonic_fit(a["keys"], a["n"], a["ws"], a["ws_bytes"], a["table"], a["words"], a["status"], None)
        return rc, h.fbn_last_error()

    for bad in (dict(keys=None), dict(ws=None), dict(table=None), dict(status=None), dict(ws=A + 8), dict(table=A + 4),
                dict(ws_bytes=ws - 1), dict(words=words - 1), dict(n=-1), dict(n=1 << 31),
                dict(n=0, table=None), dict(n=0, status=None), dict(n=0, words=1)):
        rc, msg = fit(**bad)
        assert rc == 1 and msg.startswith(b"fbn_isotonic_fit:"), (bad, rc, msg)
    assert b"fbn_isotonic_workspace_size" in fit(ws_bytes=0)[1]
    assert b"fbn_isotonic_max_blocks" in fit(words=0)[1]


def test_apply_guards_precede_device_work():
    h = _lib()
    A = 1 << 20
    for args in ((None, 10, A, 0, A), (A, 10, None, 0, A), (A, 10, A, 0, None), (A, 10, A + 4, 0, A), (A, 10, A, 2, A),
                 (A, 10, A, -1, A), (A, -1, A, 0, A), (A, 1 << 31, A, 0, A), (None, 0, None, 0, None)):
        rc = h.fbn_isotonic_apply(*args, None)
        assert rc == 1 and h.fbn_last_error().startswith(b"fbn_isotonic_apply:"), args
    assert h.fbn_isotonic_apply(None, 0, A, 0, None, None) == 0                   # nothing to do, nothing launched


@pytest.mark.parametrize("family,n", [(f, 2049) for f in R.CALIB_FAMILIES] + [("farey:40", None), ("separable:2", None),
                                                                              ("reversed:1025", None)])
@pytest.mark.parametrize("mode", ("interp", "step"))
def test_apply_rule_is_monotone_and_keeps_the_clicks(family, n, mode):
    y, p, ref = R.case(family, n)
    x = R.probes(ref, extra=p)
    out = R.apply_ref(ref, x, mode)
    assert out.dtype == np.float32 and np.all(np.diff(out) >= 0)                   # non-decreasing on sorted probes
    v = R.values(ref)
    assert out.min() >= np.float32(v[0]) and out.max() <= np.float32(v[-1])
    # a fit score lies inside its block, so the corrected scores of the fit set sum to the positives
    fitted = R.apply_ref(ref, p, mode).astype(np.float64)
    assert abs(float(fitted.sum()) - float(y.sum())) <= len(y) * 2.0 ** -24
    # inside a block and outside every block both modes agree; in a gap step gives the upper block's value
    assert np.array_equal(R.apply_ref(ref, p, "interp"), R.apply_ref(ref, p, "step"))
    nan = np.array([np.nan, 0.5], dtype=np.float32)
    assert np.isnan(R.apply_ref(ref, nan, mode)[0]) and not np.isnan(R.apply_ref(ref, nan, mode)[1])


@pytest.mark.parametrize("family", [f for f in R.CALIB_FAMILIES if f != "edges"])   # sklearn merges scores closer than 1e-15
@pytest.mark.parametrize("n", (65, 2049))
def test_default_rule_is_sklearn_clip(family, n):
    iso = pytest.importorskip("sklearn.isotonic")
    y, p, ref = R.case(family, n)
    sk = iso.IsotonicRegression(out_of_bounds="clip").fit(p.astype(np.float64), y.astype(np.float64))
    x = np.random.default_rng(n).random(2000).astype(np.float32)
    x = np.concatenate((x, R.probes(ref)))
    got = R.apply_ref(ref, x).astype(np.float64)
    assert np.abs(got - sk.predict(x.astype(np.float64))).max() <= 2.0 ** -24


def test_calibrator_json_round_trip_and_refusals(tmp_path):
    from ctr_recommendation_amd.metrics import IsotonicCalibrator
    _, _, ref = R.case("ctr", 2049)
    cal = IsotonicCalibrator(ref)
    assert len(cal) == len(ref["n"]) and R.same_blocks(cal.blocks, ref) is None and cal.table is None
    assert np.array_equal(cal.values, R.values(ref))
    assert np.array_equal(cal._words.view(np.uint64), R.table_of(ref)[:-1])        # the device table, less the status word
    path = str(tmp_path / "cal.isotonic.json")
    cal.save(path)
    d = json.load(open(path))
    assert set(d) == {"format", "lo_bits", "hi_bits", "n", "n_pos"}                # integers only
    assert all(isinstance(v, int) for k in ("lo_bits", "hi_bits", "n", "n_pos") for v in d[k])
    assert R.same_blocks(IsotonicCalibrator.load(path).blocks, ref) is None
    assert IsotonicCalibrator.from_dict(cal.to_dict()).to_dict() == d

    def broken(**kw):
        e = json.loads(json.dumps(d))
        for k, f in kw.items():
            e[k] = f(e[k])
        return e
    swap = lambda v: [v[1], v[0]] + v[2:]                                          # noqa: E731
    for bad, match in ((broken(n=lambda v: [], n_pos=lambda v: [], lo_bits=lambda v: [], hi_bits=lambda v: []), "no blocks"),
                       (broken(lo_bits=swap, hi_bits=swap), "unsorted or overlap"),
                       (broken(lo_bits=lambda v: [v[0], v[0]] + v[2:]), "unsorted or overlap"),
                       (broken(lo_bits=lambda v: [d["hi_bits"][0] + 1] + v[1:]), "unsorted or overlap"),
                       (broken(n=swap, n_pos=swap), "increase strictly"),
                       (broken(n_pos=lambda v: [v[0], v[0]] + v[2:], n=lambda v: [v[0], v[0]] + v[2:]), "increase strictly"),
                       (broken(n=lambda v: [0] + v[1:]), "1 <= n_j"),
                       (broken(n_pos=lambda v: v[:-1] + [d["n"][-1] + 1]), "n_pos_j <= n_j"),
                       (broken(n=lambda v: v[:-1]), "differ in length"),
                       (broken(hi_bits=lambda v: v[:-1] + [0x3F800001]), r"outside \[0, 1\]"),
                       (broken(n=lambda v: [1.5] + v[1:]), "list of integers"),
                       (broken(n=lambda v: [-1] + v[1:]), "list of integers"),
                       (broken(format=lambda v: "other"), "format")):
        with pytest.raises(ValueError, match=match):
            IsotonicCalibrator.from_dict(bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        cal.to("cpu")
    with pytest.raises(ValueError, match="mode"):
        cal.apply(None, mode="linear")
