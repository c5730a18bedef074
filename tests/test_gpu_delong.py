"""DeLong on the device (metrics.DeviceMetrics.placements / auc_ci and metrics.compare_auc over fbn_auc_place
and fbn_delong_reduce): the placements and the integer records must equal the host reference
(tests/_delong_ref.py) exactly, every float must be delong_from_record() of that reference bit for bit, and
nothing may depend on the samples' order, the update sizes or the rank split.  Every comparison is == or
bitwise; nothing takes a tolerance.

The sizes are the smallest that cross the kernels' boundaries (a wave of 64 within a scan block of 256, a
sort tile of 2048, one top-level chunk of the two-level scan = 65 536 samples) -- not workload sizes; the
one large case (2^22 samples) is there because a sum of products passes 2^64 only at that size.
"""
import math
import os
import re
import shutil

import numpy as np
import pytest
import torch

from tests import _delong_ref as R
from tests._calib_ref import case
from tests.test_gpu_calibration import _feed, _metrics, _same, _same_dict

pytestmark = pytest.mark.gpu

SINGLE = ("auc", "auc_var", "auc_se", "ci_lo", "ci_hi", "level", "n", "n_pos")
PAIR = ("auc_a", "auc_b", "delta", "cov", "delta_var", "delta_se", "z", "p_value")
SIZES = (1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 70001)


def _assert_single(out, rec, level=0.95):
    from ctr_recommendation_amd.metrics import delong_from_record
    assert set(out) == set(SINGLE) | {"record"}
    assert out["record"] == list(rec), (out["record"], list(rec))
    want = delong_from_record(list(rec), level=level)
    for k in SINGLE:
        assert _same(out[k], want[k]), (k, out[k], want[k])


def _assert_pair(out, y, pa, pb):
    from ctr_recommendation_amd.metrics import delong_from_record
    recs = {"aa": R.record(y, pa), "bb": R.record(y, pb), "ab": R.record(y, pa, pb)}
    assert set(out) == set(SINGLE) | set(PAIR) | {"records"}
    assert out["records"] == recs
    want = delong_from_record(recs["aa"], recs["bb"], recs["ab"])
    for k in SINGLE + PAIR:
        assert _same(out[k], want[k]), (k, out[k], want[k])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", ("ctr", "sevenths", "edges"))
def test_placements_and_record_equal_the_reference(hip_device, family, n):
    y, p = case(family, n)
    m = _metrics(hip_device, y, p)
    got = m.placements()
    assert got.dtype == torch.int64 and got.device.type == "cuda" and got.shape == (n,)
    assert np.array_equal(got.cpu().numpy(), R.case_placements(family, n))
    _assert_single(m.auc_ci(), R.case_record(family, n))
    if n == 2049:
        _assert_single(m.auc_ci(level=0.5), R.case_record(family, n), level=0.5)
        plain = m.compute()                                        # U2 of the count-based reduce is the placements' sum
        rec = R.case_record(family, n)
        assert plain["n_pos"] == rec[0] and _same(plain["auc"], rec[2] / (2 * rec[0] * rec[1]))


def test_all_equal_scores_and_single_class(hip_device):
    y, _ = case("uniform", 2049)
    n_pos = int(y.sum())
    m = _metrics(hip_device, y, np.full(2049, 0.25, dtype=np.float32))
    pl = m.placements().cpu().numpy()
    assert np.all(pl[y == 1] == 2049 - n_pos) and np.all(pl[y != 1] == n_pos)
    out = m.auc_ci()
    assert out["auc"] == 0.5 and out["auc_var"] == 0.0 and out["ci_lo"] == out["ci_hi"] == 0.5
    for label in (0.0, 1.0):
        _, p = case("uniform", 257)
        m = _metrics(hip_device, np.full(257, label, dtype=np.float32), p)
        assert not m.placements().any()
        out = m.auc_ci()
        assert out["auc"] == 0.5 and out["n"] == 257 and out["n_pos"] == int(label) * 257
        assert all(math.isnan(out[k]) for k in ("auc_var", "auc_se", "ci_lo", "ci_hi"))
        assert out["record"] == [int(label) * 257, int(1 - label) * 257, 0, 0, 0, 0, 0, 0]
    from ctr_recommendation_amd.metrics import DeviceMetrics
    empty = DeviceMetrics(0, hip_device)
    assert empty.placements().shape == (0,) and empty.auc_ci()["record"] == [0] * 8


@pytest.mark.parametrize("family", ("ctr", "sevenths", "edges"))
def test_order_and_update_sizes_do_not_enter(hip_device, family):
    y, p = case(family, 70001)
    one = _metrics(hip_device, y, p)
    perm = np.random.default_rng(9).permutation(len(y))
    two = _metrics(hip_device, y[perm], p[perm], chunks=(1, 63, 64, 65, 8192))
    a, b, again = one.auc_ci(), two.auc_ci(), two.auc_ci()
    assert a["record"] == b["record"] == again["record"] == list(R.case_record(family, 70001))
    assert all(_same(a[k], b[k]) and _same(a[k], again[k]) for k in SINGLE)
    pl = one.placements().cpu().numpy()
    assert np.array_equal(two.placements().cpu().numpy(), pl[perm])
    assert np.array_equal(two.placements().cpu().numpy(), pl[perm])           # a second call: the same bytes
    # a different, shorter stream after reset(): no trace of the old one
    two.reset()
    y2, p2 = case("uniform", 2049)
    _feed(two, hip_device, y2, p2)
    assert np.array_equal(two.placements().cpu().numpy(), R.case_placements("uniform", 2049))
    _assert_single(two.auc_ci(), R.case_record("uniform", 2049))


def test_compute_and_calibration_are_unchanged(hip_device):
    from ctr_recommendation_amd.metrics import compare_auc
    y, p = case("ctr", 2049)
    m, other = _metrics(hip_device, y, p), _metrics(hip_device, y, R.second_scores("ctr", 2049))
    first = m.auc_ci()                                             # before any compute()
    before, cal = m.compute(), m.calibration(10)
    m.placements()
    m.auc_ci()
    compare_auc(m, other)
    compare_auc(other, m)
    after, cal2 = m.compute(), m.calibration(10)
    assert _same_dict(after, before)
    assert set(cal) == set(cal2)
    for k in cal:
        if isinstance(cal[k], dict):
            assert all(np.asarray(cal[k][c]).tobytes() == np.asarray(cal2[k][c]).tobytes() for c in cal[k])
        else:
            assert _same(cal[k], cal2[k])
    assert _same_dict(m.auc_ci(), first)
    assert _same_dict(_metrics(hip_device, y, p).compute(), before)            # ... and what an instance never asked gives


@pytest.mark.parametrize("n", (2049, 70001))
def test_compare_auc_equals_the_reference(hip_device, n):
    from ctr_recommendation_amd.metrics import compare_auc
    y, pa = case("ctr", n)
    pb = R.second_scores("ctr", n)
    a, b = _metrics(hip_device, y, pa), _metrics(hip_device, y, pb, chunks=(1, 63, 64, 65))
    out = compare_auc(a, b)
    _assert_pair(out, y, pa, pb)
    assert out["delta_var"] > 0.0 and 0.0 < out["p_value"] <= 1.0
    back = compare_auc(b, a)                                       # antisymmetric
    assert back["delta"] == -out["delta"] and _same(back["delta_var"], out["delta_var"]) and _same(back["cov"], out["cov"])
    assert back["z"] == -out["z"] and _same(back["p_value"], out["p_value"])
    assert back["records"]["aa"] == out["records"]["bb"] and back["records"]["bb"] == out["records"]["aa"]
    for same in (compare_auc(a, a), compare_auc(a, _metrics(hip_device, y, pa))):
        assert same["delta"] == 0.0 and same["delta_var"] == 0.0 and same["p_value"] == 1.0 and math.isnan(same["z"])
    _assert_single(a.auc_ci(), R.record(y, pa))


def test_errors(hip_device):
    from ctr_recommendation_amd.metrics import compare_auc
    y, p = (v.copy() for v in case("uniform", 300))
    a = _metrics(hip_device, y, p)
    short = _metrics(hip_device, y[:299], p[:299])
    with pytest.raises(ValueError, match="a holds 300, b holds 299"):
        compare_auc(a, short)
    assert a._pws is None and short._pws is None                   # nothing was allocated, nothing ran
    y2 = y.copy()
    y2[137] = 1.0 - y2[137]
    with pytest.raises(ValueError, match="label mismatch"):
        compare_auc(a, _metrics(hip_device, y2, p))
    _assert_single(a.auc_ci(), R.case_record("uniform", 300))      # the mismatch belongs to the pair: a is untouched
    assert a.compute()["n"] == 300
    with pytest.raises(ValueError, match="level"):
        a.auc_ci(level=1.0)
    with pytest.raises(ValueError, match="level"):
        compare_auc(a, a, level="x")
    p[137] = np.nan
    bad = _metrics(hip_device, y, p)
    with pytest.raises(ValueError, match="NaN") as e:
        bad.auc_ci()
    with pytest.raises(ValueError) as e2:                          # the ValueError compute() raises for the same word
        bad.compute()
    assert str(e.value) == str(e2.value)
    with pytest.raises(ValueError, match="NaN"):
        compare_auc(a, bad)
    key = _metrics(hip_device, *case("uniform", 300))
    key.keys[137] = 0x7FFFFFFF                                     # score bits above bits(1.0)
    with pytest.raises(ValueError, match="not written by fbn_eval_pack"):
        key.auc_ci()


def test_sums_past_2_to_64_on_the_device(hip_device):
    """m = n = 2^21, positives at 1.0 and negatives at 0.0 (16 MB of keys): sum of a_i^2 = m 4 n^2 > 2^64."""
    from ctr_recommendation_amd.metrics import DeviceMetrics
    half = 1 << 21
    y = (torch.arange(2 * half, device=hip_device) % 2).to(torch.float32)     # interleaved classes
    m = DeviceMetrics(2 * half, hip_device)
    m.update(y, y)                                                 # the score is the label
    out = m.auc_ci()
    rec = R.closed_form(half, half)
    assert rec[4] + (rec[5] << 32) > 1 << 64
    assert out["record"] == rec
    assert out["auc"] == 1.0 and out["auc_var"] == 0.0 and out["ci_lo"] == out["ci_hi"] == 1.0
    pl = m.placements()
    assert int(pl.min()) == int(pl.max()) == 2 * half


def test_trainer_evaluate_auc_ci(hip_device):
    from ctr_recommendation_amd.data import make_batch
    from ctr_recommendation_amd.metrics import DeviceMetrics
    from ctr_recommendation_amd.trainer import FiBiNETTrainer
    V, B, d = 2000, 64, 16
    cfg = {"embedding_dim": d, "vocab_size": V, "honour_config": True, "net_dropout": 0.0}
    tr = FiBiNETTrainer(cfg, total_steps=10, batch_size=B, device=hip_device, seed=3)
    for s in range(3):
        b, y = make_batch(40 + s, B, V)
        tr.step({k: v.to(hip_device) for k, v in b.items()}, y.to(hip_device))
    batches = []
    for s in range(5):
        nb = B if s < 4 else 37                                    # the last batch is short
        b, y = make_batch(90 + s, nb, V)
        batches.append(({k: v.to(hip_device) for k, v in b.items()}, y.to(hip_device)))
    plain = tr.evaluate(batches)
    assert set(plain) == {"auc", "logloss", "n", "n_pos"}          # without the argument: today's dict
    out = tr.evaluate(batches, auc_ci=True)
    assert set(out) == set(plain) | {"auc_se", "auc_ci_lo", "auc_ci_hi", "auc_ci_level"}
    assert {k: out[k] for k in plain} == plain and out["auc_ci_level"] == 0.95
    m = DeviceMetrics(plain["n"], hip_device)
    for b, y in batches:
        m.update(tr.predict(b), y)
    for level, got in ((0.95, out), (0.8, tr.evaluate(batches, auc_ci=0.8))):
        want = m.auc_ci(level)
        assert _same(got["auc"], want["auc"]) and _same(got["auc_se"], want["auc_se"]) and want["auc_se"] > 0.0
        assert _same(got["auc_ci_lo"], want["ci_lo"]) and _same(got["auc_ci_hi"], want["ci_hi"])
        assert got["auc_ci_level"] == level
    yy = np.concatenate([y.cpu().numpy() for _, y in batches])
    pp = np.concatenate([tr.predict(b).cpu().numpy() for b, _ in batches])
    _assert_single(m.auc_ci(), R.record(yy, pp))
    both = tr.evaluate(batches, calibration_bins=10, auc_ci=True)  # with the calibration: one gather, both reduces
    assert _same(both["auc_se"], out["auc_se"]) and "ece" in both
    assert tr.evaluate(batches) == plain
    with pytest.raises(ValueError, match="level"):
        tr.evaluate(batches, auc_ci=1.5)


LINE = re.compile(r"^Epoch \d+ \| Train Loss: [\d.]+ \| Valid AUC: [\d.]+ \| \d+ samples/s \| Valid LogLoss: [\d.]+$")
FIELD = re.compile(r" \| AUC SE: (\d\.\d{4})$")


@pytest.fixture(scope="module")
def tiny_run(hip_device, tmp_path_factory):
    """One 2-epoch launcher run with valid_auc_ci, its log lines, and the weights after epoch 1 and epoch 2."""
    from ctr_recommendation_amd.data import write_microlens_parquet
    from ctr_recommendation_amd.train import run
    from tests.test_gpu_gauc import CONFIG
    tmp = tmp_path_factory.mktemp("delong")
    p = write_microlens_parquet(str(tmp), n_train=4096, n_valid=2048, n_test=1024, n_items=600, seq_width=20,
                                item_id_stride=3, seed=21)

    def write(name, extra):
        path = str(tmp / name)
        with open(path, "w") as f:
            f.write(CONFIG.format(train=p["train_data"], valid=p["valid_data"], test=p["test_data"],
                                  info=p["item_info"], extra=extra))
        return path

    path, best, first = write("ci.yaml", "  valid_auc_ci: true\n"), str(tmp / "ck" / "best.pth"), str(tmp / "epoch1.pth")
    logs = []

    def log(line):
        logs.append(line)
        if "New best" in line and not os.path.exists(first):      # epoch 1 always is (the best AUC starts at 0)
            shutil.copyfile(best, first)

    out = run(path, epochs=2, checkpoint=best, log=log)
    last = str(tmp / "epoch2.pth")
    torch.save(out["trainer"].state_dict(), last)
    return {"config": path, "plain": write("plain.yaml", ""), "logs": logs, "out": out, "a": first, "b": last, "tmp": tmp}


def test_launcher_reports_auc_se(hip_device, tiny_run):
    from ctr_recommendation_amd.train import run
    out = tiny_run["out"]
    epoch_lines = [line for line in tiny_run["logs"] if "Valid AUC" in line]
    assert len(epoch_lines) == 2
    for k, line in enumerate(epoch_lines):
        f = FIELD.search(line)
        assert f is not None and LINE.match(line[:f.start()]), line
        assert f.group(1) == f"{out['valid_auc_se'][k]:.4f}"
    se = out["valid_auc_se"]
    assert len(se) == 2 and all(isinstance(v, float) and np.isfinite(v) and v > 0.0 for v in se)
    assert set(out) == {"best_auc", "history", "valid_logloss", "trainer", "valid_auc_se"}
    # without the key: the lines and the result are what they were
    logs = []
    plain = run(tiny_run["plain"], epochs=1, checkpoint=str(tiny_run["tmp"] / "ck2" / "best.pth"), log=logs.append)
    epoch_lines = [line for line in logs if "Valid AUC" in line]
    assert len(epoch_lines) == 1 and all(LINE.match(line) for line in epoch_lines), epoch_lines
    assert not any("AUC SE" in line for line in logs)
    assert set(plain) == {"best_auc", "history", "valid_logloss", "trainer"}


def test_compare_command(hip_device, tiny_run):
    from ctr_recommendation_amd import compare
    from ctr_recommendation_amd.loader import make_loaders
    from ctr_recommendation_amd.metrics import DeviceMetrics, compare_auc
    from ctr_recommendation_amd.predict import load_checkpoint
    from ctr_recommendation_amd.train import load_config
    got = compare.run(tiny_run["config"], tiny_run["a"], tiny_run["b"], level=0.9)
    _, dcfg, mcfg = load_config(tiny_run["config"])
    _, valid_loader, _ = make_loaders(dcfg, mcfg, hip_device)
    tr = tiny_run["out"]["trainer"]
    fed = []
    for ck in (tiny_run["a"], tiny_run["b"]):
        tr.load_state_dict(load_checkpoint(ck))
        m = DeviceMetrics(2048, hip_device)
        for batch, labels in valid_loader:
            m.update(tr.predict(batch), labels)
        fed.append(m)
    want = compare_auc(fed[0], fed[1], level=0.9)
    assert got["records"] == want["records"] and got["n"] == 2048 and got["level"] == 0.9
    assert all(_same(got[k], want[k]) for k in SINGLE + PAIR)
    assert got["auc_a"] != got["auc_b"] and got["delta_var"] > 0.0             # one more epoch moved the scores
    assert _same(got["auc_b"], tiny_run["out"]["history"][-1][2])              # epoch 2's validation AUC
    twice = compare.run(tiny_run["config"], tiny_run["b"], tiny_run["b"])
    assert twice["delta"] == 0.0 and twice["delta_var"] == 0.0 and twice["p_value"] == 1.0


def _rank_worker(rank, port, q):
    import torch.distributed as dist
    from ctr_recommendation_amd.metrics import compare_auc
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        dev = torch.device("cuda:0")
        y, pa = case("ctr", 2049)
        pb = R.second_scores("ctr", 2049)
        lo, hi = (0, 700) if rank == 0 else (700, 2049)            # unequal slices of one stream
        a, b = _metrics(dev, y[lo:hi], pa[lo:hi]), _metrics(dev, y[lo:hi], pb[lo:hi])
        one = a.auc_ci(group=dist.group.WORLD, stage_on_cpu=True)
        two = compare_auc(a, b, group=dist.group.WORLD, stage_on_cpu=True)
        q.put((rank, "ok", one, two))
    except Exception as e:
        q.put((rank, repr(e), None, None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_gather_keys(hip_device):
    """2 ranks sharing one device (gloo, host-staged gather): both return the single-process records."""
    from ctr_recommendation_amd.metrics import compare_auc
    from tests._spawn import spawn_and_wait
    from tests.test_gpu_gauc import _port
    y, pa = case("ctr", 2049)
    pb = R.second_scores("ctr", 2049)
    res = sorted(spawn_and_wait(_rank_worker, args=(_port(),), timeout=240.0, nprocs=2, rank_args=True),
                 key=lambda r: r[0])
    assert all(r[1] == "ok" for r in res), res
    a, b = _metrics(hip_device, y, pa), _metrics(hip_device, y, pb)
    one, two = a.auc_ci(), compare_auc(a, b)
    _assert_single(one, R.case_record("ctr", 2049))
    for _, _, got1, got2 in res:
        assert got1["record"] == one["record"] and all(_same(got1[k], one[k]) for k in SINGLE)
        assert got2["records"] == two["records"] and all(_same(got2[k], two[k]) for k in SINGLE + PAIR)
