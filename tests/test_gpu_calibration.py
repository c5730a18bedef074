"""Calibration on the device (metrics.DeviceMetrics.calibration over fbn_calib_reduce): both planes of
the reliability table must equal the host reference (tests/_calib_ref.py) exactly, the scalars must be
calibration_from_table() of that reference, and every byte must be independent of the samples' order, the
update sizes and the rank split.  Every comparison is == or bitwise; nothing takes a tolerance.

The sizes are the smallest that cross the kernels' boundaries (a wave of 64, a prefix block of 256, a
sort tile of 2048, one top-level chunk of the two-level prefix = 65 536 samples) -- not workload sizes.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import _calib_ref as C

pytestmark = pytest.mark.gpu

SCALARS = ("bins", "n", "n_pos", "ece", "mce", "ece_mass", "pcoc", "brier", "entropy")


def _feed(m, dev, y, p, chunks=None, ids=None):
    yt, pt = torch.from_numpy(np.array(y)).to(dev), torch.from_numpy(np.array(p)).to(dev)      # copies: the cases are read-only
    it = None if ids is None else torch.from_numpy(np.array(ids)).to(dev)
    lo = 0
    for c in list(chunks or ()) + [len(y)]:
        hi = min(len(y), lo + c)
        if it is None:
            m.update(pt[lo:hi], yt[lo:hi])
        else:
            m.update(pt[lo:hi], yt[lo:hi], group_ids=it[lo:hi])
        lo = hi
    assert m.count == len(y)
    return m


def _metrics(dev, y, p, chunks=None, ids=None):
    from ctr_recommendation_amd.metrics import DeviceMetrics
    return _feed(DeviceMetrics(len(y), dev, grouped=ids is not None), dev, y, p, chunks, ids)


def _same(a, b):
    """bitwise equality of two result values (NaN equals NaN)"""
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes() or (math.isnan(a) and math.isnan(b))
    return a == b


def _same_dict(a, b):
    return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)


def _table_bytes(out):
    return b"".join(np.ascontiguousarray(out[pl][c]).tobytes() for pl in ("width", "mass")
                    for c in C.COLS + ("p_lo", "p_hi"))


def _assert_result(out, ref):
    from ctr_recommendation_amd.metrics import calibration_from_table
    assert set(out) == set(SCALARS) | {"width", "mass"}
    assert C.same_table(out, ref) is None, C.same_table(out, ref)
    want = calibration_from_table(ref)
    for k in SCALARS:
        assert _same(out[k], want[k]), (k, out[k], want[k])


@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("family", C.FAMILIES)
def test_both_planes_and_scalars_equal_the_reference(hip_device, family, n):
    y, p = C.case(family, n)
    m = _metrics(hip_device, y, p)
    plain = m.compute()
    for bins in C.BINS:                                            # repeated on the one fed instance
        out = m.calibration(bins)
        _assert_result(out, C.table(family, n, bins))
        for c in C.COLS:                                           # both planes partition the same samples
            assert int(out["width"][c].sum()) == int(out["mass"][c].sum()), (bins, c)
        assert out["n"] == plain["n"] == n and out["n_pos"] == plain["n_pos"] == int(y.sum())
    assert m.calibration()["bins"] == 10


def test_empty_instance_gives_zeros_and_nan(hip_device):
    from ctr_recommendation_amd.metrics import DeviceMetrics
    m = DeviceMetrics(0, hip_device)
    out = m.calibration(7)
    assert out["bins"] == 7 and out["n"] == 0 and out["n_pos"] == 0
    assert all(math.isnan(out[k]) for k in ("ece", "mce", "ece_mass", "pcoc", "brier", "entropy"))
    for plane in ("width", "mass"):
        assert all(not out[plane][c].any() and len(out[plane][c]) == 7 for c in C.COLS)
        assert np.isnan(out[plane]["p_lo"]).all() and np.isnan(out[plane]["p_hi"]).all()


@pytest.mark.parametrize("family", ("ctr", "sevenths", "edges"))
def test_order_and_update_sizes_do_not_enter(hip_device, family):
    y, p = C.case(family, 70001)
    one = _metrics(hip_device, y, p)
    perm = np.random.default_rng(9).permutation(len(y))
    two = _metrics(hip_device, y[perm], p[perm], chunks=(1, 63, 64, 65, 8192))
    for bins in (10, 1024):
        a, b, again = one.calibration(bins), two.calibration(bins), two.calibration(bins)
        assert _table_bytes(a) == _table_bytes(b) == _table_bytes(again)
        assert all(_same(a[k], b[k]) and _same(a[k], again[k]) for k in SCALARS)
        _assert_result(b, C.table(family, 70001, bins))
    # a different, shorter stream after reset(): no trace of the old one
    y2, p2 = C.case("uniform", 4099)
    two.reset()
    _feed(two, hip_device, y2, p2)
    _assert_result(two.calibration(16), C.table("uniform", 4099, 16))


def test_compute_is_unchanged_by_calibration(hip_device):
    from tests import _gauc_ref as R
    y, p = C.case("ctr", 4099)
    m = _metrics(hip_device, y, p)
    before = m.compute()
    m.calibration(10)
    m.calibration(1024)
    assert _same_dict(m.compute(), before)
    assert _same_dict(_metrics(hip_device, y, p).compute(), before)           # ... and what an instance never asked gives
    # a grouped instance: the grouped numbers and the group table too
    yg, pg, ids, ref = R.case("uniform", "small", 4099)
    g = _metrics(hip_device, yg, pg, ids=ids)
    cal_first = g.calibration(10)                                             # before any compute()
    before = g.compute()
    table = {k: v.cpu().numpy() for k, v in g.group_table().items()}
    cal = g.calibration(10)
    assert _table_bytes(cal) == _table_bytes(cal_first)
    _assert_result(cal, C.ref_table(yg, pg, 10))
    assert _same_dict(g.compute(), before)
    assert all(np.array_equal(v.cpu().numpy(), table[k]) and np.array_equal(table[k], ref[k]) for k, v in g.group_table().items())


@pytest.mark.parametrize("what,match", (("nan", "NaN"), ("above", r"outside \[0, 1\]"), ("below", r"outside \[0, 1\]"),
                                        ("label", "label"), ("key", "not written by fbn_eval_pack")))
def test_bad_inputs_raise_from_calibration(hip_device, what, match):
    y, p = (a.copy() for a in C.case("uniform", 300))
    if what == "nan":
        p[137] = np.nan
    elif what == "above":
        p[137] = 1.5
    elif what == "below":
        p[137] = -0.25
    elif what == "label":
        y[137] = 0.5
    m = _metrics(hip_device, y, p)
    if what == "key":
        m.keys[137] = 0x7FFFFFFF                                   # score bits above bits(1.0)
    with pytest.raises(ValueError, match=match) as e:
        m.calibration(10)
    with pytest.raises(ValueError) as e2:                          # the ValueError compute() raises for the same word
        m.compute()
    assert str(e.value) == str(e2.value)
    m.reset()                                                      # the status word is cleared with the stream
    y, p = C.case("uniform", 300)
    _assert_result(_feed(m, hip_device, y, p).calibration(10), C.table("uniform", 300, 10))


@pytest.mark.parametrize("bins", (0, 1025, -1, 2.5))
def test_bins_out_of_range_raise_before_launching(hip_device, bins):
    y, p = C.case("uniform", 65)
    m = _metrics(hip_device, y, p)
    with pytest.raises(ValueError, match="bins"):
        m.calibration(bins)
    assert m._cws is None and m._ctab is None                      # nothing was allocated, nothing ran
    _assert_result(m.calibration(1024), C.table("uniform", 65, 1024))


def test_trainer_evaluate_calibration(hip_device):
    from ctr_recommendation_amd.data import make_batch
    from ctr_recommendation_amd.metrics import normalized_entropy
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
        b["user_id"] = b["user_id"] % 16
        batches.append(({k: v.to(hip_device) for k, v in b.items()}, y.to(hip_device)))
    err0 = int(tr.err.item())
    plain = tr.evaluate(batches)
    assert set(plain) == {"auc", "logloss", "n", "n_pos"}          # without the argument: today's dict
    out = tr.evaluate(batches, calibration_bins=10)
    assert int(tr.err.item()) == err0
    assert set(out) == set(plain) | {"ece", "mce", "ece_mass", "pcoc", "brier", "ne", "calibration"}
    assert {k: out[k] for k in plain} == plain
    yy = np.concatenate([y.cpu().numpy() for _, y in batches])
    pp = np.concatenate([tr.predict(b).cpu().numpy() for b, _ in batches])
    _assert_result(out["calibration"], C.ref_table(yy, pp, 10))
    cal = out["calibration"]
    assert all(_same(out[k], cal[k]) for k in ("ece", "mce", "ece_mass", "pcoc", "brier"))
    assert cal["entropy"] > 0 and _same(out["ne"], out["logloss"] / cal["entropy"])
    assert _same(out["ne"], normalized_entropy(out["logloss"], out["n"], out["n_pos"]))
    both = tr.evaluate(batches, group_by="user_id", calibration_bins=10)      # with the grouped metrics
    assert both["n_groups"] == 16 and _table_bytes(both["calibration"]) == _table_bytes(cal)
    assert tr.evaluate(batches) == plain
    with pytest.raises(ValueError, match="bins"):
        tr.evaluate(batches, calibration_bins=0)


LINE = re.compile(r"^Epoch \d+ \| Train Loss: [\d.]+ \| Valid AUC: [\d.]+ \| \d+ samples/s \| Valid LogLoss: [\d.]+$")
FIELDS = re.compile(r" \| Valid ECE: (\d\.\d{4}) \| PCOC: (\d+\.\d{4}) \| NE: (\d+\.\d{4})$")


def test_launcher_reports_calibration(hip_device, tmp_path):
    from ctr_recommendation_amd.data import write_microlens_parquet
    from ctr_recommendation_amd.loader import make_loaders
    from ctr_recommendation_amd.metrics import calibration_from_table, normalized_entropy
    from ctr_recommendation_amd.train import load_config, run
    from tests.test_gpu_gauc import CONFIG
    p = write_microlens_parquet(str(tmp_path), n_train=4096, n_valid=2048, n_test=1024, n_items=600, seq_width=20,
                                item_id_stride=3, seed=21)

    def write(name, extra):
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write(CONFIG.format(train=p["train_data"], valid=p["valid_data"], test=p["test_data"],
                                  info=p["item_info"], extra=extra))
        return path

    path = write("calib.yaml", "  valid_calibration_bins: 10\n")
    logs = []
    out = run(path, epochs=2, checkpoint=str(tmp_path / "ck" / "best.pth"), log=logs.append)
    epoch_lines = [line for line in logs if "Valid AUC" in line]
    assert len(epoch_lines) == 2
    for k, line in enumerate(epoch_lines):                         # the three fields close every epoch line
        f = FIELDS.search(line)
        assert f is not None and LINE.match(line[:f.start()]), line
        assert f.group(1) == f"{out['valid_ece'][k]:.4f}" and f.group(2) == f"{out['valid_pcoc'][k]:.4f}"
        assert f.group(3) == f"{out['valid_ne'][k]:.4f}"
    assert all(len(out[k]) == 2 and all(np.isfinite(v) for v in out[k]) for k in ("valid_ece", "valid_pcoc", "valid_ne"))
    _, dcfg, mcfg = load_config(path)
    _, valid_loader, _ = make_loaders(dcfg, mcfg, hip_device)
    tr = out["trainer"]
    ys, ps = [], []
    for batch, labels in valid_loader:
        ps.append(tr.predict(batch).cpu().numpy())
        ys.append(labels.cpu().numpy())
    ref = calibration_from_table(C.ref_table(np.concatenate(ys), np.concatenate(ps), 10))
    assert out["valid_ece"][-1] == ref["ece"] and out["valid_pcoc"][-1] == ref["pcoc"]
    assert out["valid_ne"][-1] == normalized_entropy(out["valid_logloss"][-1], ref["n"], ref["n_pos"])
    # without the key: the lines and the result are what they were
    path = write("plain.yaml", "")
    logs = []
    out = run(path, epochs=1, checkpoint=str(tmp_path / "ck2" / "best.pth"), log=logs.append)
    epoch_lines = [line for line in logs if "Valid AUC" in line]
    assert len(epoch_lines) == 1 and all(LINE.match(line) for line in epoch_lines), epoch_lines
    assert not any("ECE" in line or "PCOC" in line or "NE:" in line for line in logs)
    assert set(out) == {"best_auc", "history", "valid_logloss", "trainer"}


def _rank_worker(rank, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        dev = torch.device("cuda:0")
        y, p = C.case("ctr", 4099)
        lo, hi = (0, 1500) if rank == 0 else (1500, 4099)          # unequal slices of one stream
        m = _metrics(dev, y[lo:hi], p[lo:hi])
        out = m.calibration(10, group=dist.group.WORLD, stage_on_cpu=True)
        plain, cal = m.compute_and_calibrate(16, group=dist.group.WORLD, stage_on_cpu=True)
        q.put((rank, "ok", out, plain, cal))
    except Exception as e:
        q.put((rank, repr(e), None, None, None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_gather_keys(hip_device):
    """2 ranks sharing one device (gloo, host-staged gather): both return the single-process result bit
    for bit -- the table follows the sorted keys, not the gather order."""
    from tests._spawn import spawn_and_wait
    from tests.test_gpu_gauc import _port
    y, p = C.case("ctr", 4099)
    res = sorted(spawn_and_wait(_rank_worker, args=(_port(),), timeout=240.0, nprocs=2, rank_args=True),
                 key=lambda r: r[0])
    assert all(r[1] == "ok" for r in res), res
    single = _metrics(hip_device, y, p)
    one10, one16, plain1 = single.calibration(10), single.calibration(16), single.compute()
    _assert_result(one10, C.table("ctr", 4099, 10))
    for _, _, out, plain, cal in res:
        assert _table_bytes(out) == _table_bytes(one10) and all(_same(out[k], one10[k]) for k in SCALARS)
        assert _table_bytes(cal) == _table_bytes(one16) and all(_same(cal[k], one16[k]) for k in SCALARS)
        assert _same_dict(plain, plain1)
