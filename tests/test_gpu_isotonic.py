"""The isotonic calibrator on an MI355X (csrc/isotonic.hip): pytest -m gpu.

Fit: the device table equals the host reference (tests/_isotonic_ref.py) exactly.  A hull tile is 1024
sorted samples and every merge level halves the tiles, so the sizes sit around one tile (1023 .. 1025),
two (2047 .. 2049: one level, then an odd third tile), five (4099: three levels) and 65 / 69 tiles (seven
levels); the Farey families make every group a hull vertex, the degenerate ones leave one or two.
Apply: both modes bitwise equal to the numpy rule, through the LDS path (K <= 1024) and the global one.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import _calib_ref as C
from tests import _isotonic_ref as R

pytestmark = pytest.mark.gpu

TILE_SIZES = (1023, 1024, 1025)
NAMED = ("farey:8", "farey:40", "farey:64", "farey_repeat:16,40", "distinct_convex:24", "distinct_blocks:24",
         "distinct_blocks:40", "separable:1", "separable:2", "separable:1024", "separable:2049", "reversed:1",
         "reversed:1025", "reversed:4099", "all_pos:1024", "all_pos:2049", "all_neg:1025", "all_neg:4099")


def _feed(m, dev, y, p, chunks=None):
    yt, pt = torch.from_numpy(np.array(y)).to(dev), torch.from_numpy(np.array(p)).to(dev)      # copies: the cases are read-only
    lo = 0
    for c in list(chunks or ()) + [len(y)]:
        hi = min(len(y), lo + c)
        m.update(pt[lo:hi], yt[lo:hi])
        lo = hi
    assert m.count == len(y)
    return m


def _metrics(dev, y, p, chunks=None):
    from ctr_recommendation_amd.metrics import DeviceMetrics
    return _feed(DeviceMetrics(len(y), dev), dev, y, p, chunks)


@pytest.fixture(scope="module")
def fed(hip_device):
    """One DeviceMetrics for every fit case (reset and fed again): its workspace and table grow once."""
    from ctr_recommendation_amd.metrics import DeviceMetrics
    return DeviceMetrics(70001, hip_device)


def _table_words(m):
    """The words fbn_isotonic_fit left in the instance's table, up to and including the status word."""
    host = m._itab.cpu().numpy().view(np.uint64)
    return host[:2 * int(host[0]) + 2]


def _assert_fit(m, ref):
    cal = m.isotonic()
    assert R.same_blocks(cal.blocks, ref) is None, (R.same_blocks(cal.blocks, ref), len(cal), len(ref["n"]))
    assert np.array_equal(_table_words(m), R.table_of(ref))                       # K, every block word, status 0
    assert np.array_equal(cal.table.cpu().numpy().view(np.uint64), R.table_of(ref)[:-1])
    return cal


@pytest.mark.parametrize("n", C.SIZES + TILE_SIZES)
@pytest.mark.parametrize("family", R.CALIB_FAMILIES)
def test_fit_equals_the_reference(hip_device, fed, family, n):
    y, p, ref = R.case(family, n)
    fed.reset()
    _assert_fit(_feed(fed, hip_device, y, p), ref)


@pytest.mark.parametrize("family", NAMED)
def test_fit_of_the_named_families(hip_device, fed, family):
    y, p, ref = R.case(family)
    fed.reset()
    _assert_fit(_feed(fed, hip_device, y, p), ref)


def test_fit_of_nothing_is_refused(hip_device):
    from ctr_recommendation_amd import _lib
    from ctr_recommendation_amd.metrics import DeviceMetrics
    m = DeviceMetrics(16, hip_device)
    with pytest.raises(ValueError, match="no samples"):
        m.isotonic()
    assert int(m._itab[0].item()) == 0 and int(m._itab[1].item()) == 0            # n = 0 writes K = 0 and the status word
    y, p, ref = R.case("sevenths", 2)
    _assert_fit(_feed(m, hip_device, y, p), ref)
    assert _lib.lib().fbn_isotonic_max_blocks(2) == 3


@pytest.mark.parametrize("family,n", (("ctr", 4099), ("sevenths", 4099), ("edges", 2049), ("farey:40", None)))
def test_order_and_update_sizes_do_not_enter(hip_device, family, n):
    y, p, ref = R.case(family, n)
    a = _metrics(hip_device, y, p)
    _assert_fit(a, ref)
    want = _table_words(a).tobytes()
    perm = np.random.default_rng(3).permutation(len(y))
    b = _metrics(hip_device, y[perm], p[perm], chunks=(1, 63, 1000, 7))
    _assert_fit(b, ref)
    assert _table_words(b).tobytes() == want


def test_compute_and_calibration_are_unchanged_by_isotonic(hip_device):
    y, p, ref = R.case("ctr", 4099)
    m = _metrics(hip_device, y, p)
    before, cal_before = m.compute(), m.calibration(10)
    _assert_fit(m, ref)
    after, cal_after = m.compute(), m.calibration(10)
    assert before == after and C.same_table(cal_after, cal_before) is None
    assert all(cal_after[k] == cal_before[k] for k in ("ece", "pcoc", "brier", "n", "n_pos"))
    _assert_fit(m, ref)                                                            # and it can be repeated


@pytest.mark.parametrize("what,match", (("nan", "NaN"), ("above", r"outside \[0, 1\]"), ("label", "label"),
                                        ("key", "not written by fbn_eval_pack")))
def test_bad_inputs_raise_computes_error(hip_device, what, match):
    y, p = (a.copy() for a in C.case("uniform", 300))
    if what == "nan":
        p[137] = np.nan
    elif what == "above":
        p[137] = 1.5
    elif what == "label":
        y[137] = 0.5
    m = _metrics(hip_device, y, p)
    if what == "key":
        m.keys[137] = 0x7FFFFFFF                                   # score bits above bits(1.0)
    with pytest.raises(ValueError, match=match) as e:
        m.isotonic()
    with pytest.raises(ValueError) as e2:                          # the ValueError compute() raises for the same word
        m.compute()
    assert str(e.value) == str(e2.value)
    m.reset()
    y, p, ref = R.case("uniform", 300)
    _assert_fit(_feed(m, hip_device, y, p), ref)


# ---------------------------------------------------------------------------------------- apply
def _probe_scores(y, p, ref):
    x = np.concatenate((R.probes(ref, extra=p), np.array([np.nan, -0.0, 1.0, 0.0, 2.0 ** -149, -0.5, 1.5], dtype=np.float32)))
    nan2 = np.array([0x7FC00001, 0xFFC00000], dtype=np.uint32).view(np.float32)  # NaNs keep their bits
    return np.concatenate((x, nan2)).astype(np.float32)


@pytest.mark.parametrize("family,n,K", (("reversed:1025", None, 1), ("separable:2049", None, 2), ("ctr", 70001, 48),
                                        ("farey:40", None, 491), ("farey:64", None, 1261)))
def test_apply_equals_the_numpy_rule_bitwise(hip_device, family, n, K):
    from ctr_recommendation_amd.metrics import IsotonicCalibrator
    y, p, ref = R.case(family, n)
    assert len(ref["n"]) == K                                      # K <= 1024: staged in LDS; 1261: the global table
    cal = IsotonicCalibrator(ref, device=hip_device)
    x = _probe_scores(y, p, ref)
    xt = torch.from_numpy(x).to(hip_device)
    for mode in ("interp", "step"):
        want = R.apply_ref(ref, x, mode)
        got = cal.apply(xt, mode=mode)
        assert got.dtype == torch.float32 and got.shape == xt.shape
        assert got.cpu().numpy().tobytes() == want.tobytes(), mode
        buf = xt.clone()
        assert cal.apply(buf, mode=mode, out=buf) is buf           # in place equals out of place
        assert buf.cpu().numpy().tobytes() == want.tobytes(), mode
    assert cal(xt).cpu().numpy().tobytes() == R.apply_ref(ref, x).tobytes()       # __call__: the default rule
    two = xt[:6].reshape(2, 3).to(torch.float64)                   # another dtype and shape: converted, shape kept
    assert cal(two).shape == (2, 3) and cal(two).reshape(-1).cpu().numpy().tobytes() == R.apply_ref(ref, x[:6]).tobytes()
    with pytest.raises(ValueError, match="mode"):
        cal.apply(xt, mode="linear")
    with pytest.raises(ValueError, match="out must be"):
        cal.apply(xt, out=torch.empty(3, dtype=torch.float32, device=hip_device))
    with pytest.raises(RuntimeError):
        cal.apply(torch.from_numpy(x))                             # a host tensor: no CPU fallback


def test_fitted_calibrator_applies_and_corrects_pcoc(hip_device):
    """Fit on the device, apply on the device, measure on the device: the corrected scores of the fit set
    have PCOC 1 up to the one fp32 rounding per sample."""
    y, p, ref = R.case("ctr", 70001)
    m = _metrics(hip_device, y, p)
    raw = m.calibration(10)
    assert raw["pcoc"] < 0.9                                       # the family under-predicts
    cal = _assert_fit(m, ref)
    pt = torch.from_numpy(np.array(p)).to(hip_device)
    fixed = cal(pt)
    assert fixed.cpu().numpy().tobytes() == R.apply_ref(ref, p).tobytes()
    m2 = _metrics(hip_device, y, fixed.cpu().numpy())
    out = m2.calibration(10)
    assert abs(out["pcoc"] - 1.0) <= 2.0 ** -24 * len(y) / float(y.sum())
    assert m2.compute()["auc"] >= m.compute()["auc"]               # monotone map: only new ties, and PAV's ties do not lose


# ---------------------------------------------------------------------------------------- end to end
def _trainer_and_batches(dev):
    from ctr_recommendation_amd.data import make_batch
    from ctr_recommendation_amd.trainer import FiBiNETTrainer
    V, B, d = 2000, 64, 16
    cfg = {"embedding_dim": d, "vocab_size": V, "honour_config": True, "net_dropout": 0.0}
    tr = FiBiNETTrainer(cfg, total_steps=10, batch_size=B, device=dev, seed=3)
    for s in range(3):
        b, y = make_batch(40 + s, B, V)
        tr.step({k: v.to(dev) for k, v in b.items()}, y.to(dev))
    batches = []
    for s in range(5):
        nb = B if s < 4 else 37                                    # the last batch is short
        b, y = make_batch(90 + s, nb, V)
        batches.append(({k: v.to(dev) for k, v in b.items()}, y.to(dev)))
    return tr, batches


def test_trainer_evaluate_and_predict_with_a_calibrator(hip_device):
    tr, batches = _trainer_and_batches(hip_device)
    plain = tr.evaluate(batches)
    assert set(plain) == {"auc", "logloss", "n", "n_pos"}          # the defaults leave the dict as it is
    out = tr.evaluate(batches, fit_isotonic=True)
    assert set(out) == set(plain) | {"calibrator"} and {k: out[k] for k in plain} == plain
    cal = out["calibrator"]
    yy = np.concatenate([y.cpu().numpy() for _, y in batches])
    pp = np.concatenate([tr.predict(b).cpu().numpy() for b, _ in batches])
    ref = R.fit_ref(yy, pp)
    assert R.same_blocks(cal.blocks, ref) is None                  # fitted on the raw scores
    fixed = tr.evaluate(batches, calibrator=cal, calibration_bins=10)
    n, n_pos = fixed["n"], fixed["n_pos"]
    assert (n, n_pos) == (plain["n"], plain["n_pos"]) and n_pos > 0
    assert abs(fixed["pcoc"] - 1.0) <= 2.0 ** -24 * n / n_pos
    assert fixed["auc"] >= plain["auc"]
    for b, _ in batches[:2] + batches[-1:]:
        raw = tr.predict(b)
        got = tr.predict(b, calibrator=cal)
        assert got.shape == raw.shape and torch.equal(got, cal(raw))
        assert got.cpu().numpy().tobytes() == R.apply_ref(ref, raw.cpu().numpy()).tobytes()
    with pytest.raises(ValueError, match="logits"):
        tr.predict(batches[0][0], logits=True, calibrator=cal)
    with pytest.raises(ValueError, match="fit_isotonic"):
        tr.evaluate(batches, fit_isotonic=True, calibrator=cal)
    assert tr.evaluate(batches) == plain


def test_recommender_scores_with_a_calibrator(hip_device):
    from ctr_recommendation_amd.metrics import IsotonicCalibrator
    from tests.test_gpu_recommend import CHUNKED, _catalogue, _histories, _rec
    _, _, ref = R.case("ctr", 2049)
    cal = IsotonicCalibrator(ref, device=hip_device)
    rec = _rec(16, hip_device, CHUNKED)
    seq = _histories().to(hip_device)
    raw = rec.score(seq)
    got = rec.score(seq, calibrator=cal)
    assert got.shape == raw.shape and torch.equal(got, cal(raw))
    assert got.cpu().numpy().tobytes() == R.apply_ref(ref, raw.cpu().numpy().reshape(-1)).tobytes()
    ids = _catalogue()["item_id"]
    cands = torch.stack([ids[:7], ids[100:107], ids[500:507]]).clone()
    cands[1, 3] = -1                                               # an empty slot still reads 0
    cands = cands.to(hip_device)
    raw_l = rec.score_lists(seq, cands)
    got_l = rec.score_lists(seq, cands, calibrator=cal)
    live = cands >= 0
    assert torch.equal(got_l[live], cal(raw_l)[live]) and float(got_l[1, 3]) == 0.0 and float(raw_l[1, 3]) == 0.0
    for fn, args in ((rec.score, (seq,)), (rec.score_lists, (seq, cands))):
        with pytest.raises(ValueError, match="logits"):
            fn(*args, logits=True, calibrator=cal)
    import inspect
    assert "calibrator" not in inspect.signature(rec.topk).parameters      # untouched: it ranks on logits, the map is monotone


LINE = re.compile(r"^Epoch \d+ \| Train Loss: [\d.]+ \| Valid AUC: [\d.]+ \| \d+ samples/s \| Valid LogLoss: [\d.]+$")
FIELD = re.compile(r" \| iso blocks: (\d+)$")


def test_launchers_fit_save_and_apply(hip_device, tmp_path, capsys):
    from ctr_recommendation_amd import predict as predict_cli
    from ctr_recommendation_amd.data import write_microlens_parquet
    from ctr_recommendation_amd.loader import make_loaders
    from ctr_recommendation_amd.metrics import IsotonicCalibrator
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

    path = write("iso.yaml", "  valid_isotonic: true\n")
    ck = str(tmp_path / "ck" / "best.pth")
    logs = []
    out = run(path, epochs=2, checkpoint=ck, log=logs.append)
    epoch_lines = [line for line in logs if "Valid AUC" in line]
    assert len(epoch_lines) == 2 and len(out["valid_iso_blocks"]) == 2
    for k, line in enumerate(epoch_lines):                         # the field closes every epoch line
        f = FIELD.search(line)
        assert f is not None and LINE.match(line[:f.start()]), line
        assert int(f.group(1)) == out["valid_iso_blocks"][k] >= 1
    iso_path = str(tmp_path / "ck" / "best.isotonic.json")
    assert os.path.exists(ck) and os.path.exists(iso_path)
    saved = IsotonicCalibrator.load(iso_path, hip_device)
    aucs = [h[2] for h in out["history"]]
    best = aucs.index(max(aucs))                                   # saved at each new best AUC: the first maximum's
    assert len(saved) == out["valid_iso_blocks"][best]
    _, dcfg, mcfg = load_config(path)
    _, valid_loader, _ = make_loaders(dcfg, mcfg, hip_device)
    tr = out["trainer"]
    ys, ps = [], []
    for batch, labels in valid_loader:
        ps.append(tr.predict(batch).cpu().numpy())
        ys.append(labels.cpu().numpy())
    ref = R.fit_ref(np.concatenate(ys), np.concatenate(ps))        # the last epoch's validation scores
    assert len(ref["n"]) == out["valid_iso_blocks"][-1]
    if best == 1:
        assert R.same_blocks(saved.blocks, ref) is None
    # predict.py: --calibrator applies the saved map to the export; without it nothing changes
    args = ["--config", path, "--checkpoint", ck]
    plain = predict_cli.main(args + ["--out", str(tmp_path / "a.csv"), "--zip", str(tmp_path / "a.zip")])
    again = predict_cli.main(args + ["--out", str(tmp_path / "b.csv"), "--zip", str(tmp_path / "b.zip")])
    fixed = predict_cli.main(args + ["--out", str(tmp_path / "c.csv"), "--zip", str(tmp_path / "c.zip"), "--calibrator", iso_path])
    assert open(tmp_path / "a.csv", "rb").read() == open(tmp_path / "b.csv", "rb").read()
    assert plain.tobytes() == again.tobytes() and len(fixed) == len(plain) == 1024
    assert fixed.tobytes() == R.apply_ref(saved.blocks, plain).tobytes()
    assert open(tmp_path / "c.csv", "rb").read() != open(tmp_path / "a.csv", "rb").read()
    # without the key: the lines, the files and the result are what they were
    path = write("plain.yaml", "")
    logs = []
    out = run(path, epochs=1, checkpoint=str(tmp_path / "ck2" / "best.pth"), log=logs.append)
    epoch_lines = [line for line in logs if "Valid AUC" in line]
    assert len(epoch_lines) == 1 and all(LINE.match(line) for line in epoch_lines), epoch_lines
    assert not any("iso" in line for line in logs)
    assert sorted(os.listdir(tmp_path / "ck2")) == ["best.pth"]
    assert set(out) == {"best_auc", "history", "valid_logloss", "trainer"}


# ---------------------------------------------------------------------------------------- two ranks
def _rank_worker(rank, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        dev = torch.device("cuda:0")
        y, p, _ = R.case("ctr", 4099)
        lo, hi = (0, 1500) if rank == 0 else (1500, 4099)          # unequal slices of one stream
        m = _metrics(dev, y[lo:hi], p[lo:hi])
        cal = m.isotonic(group=dist.group.WORLD, stage_on_cpu=True)
        q.put((rank, "ok", {k: np.array(v) for k, v in cal.blocks.items()}))
    except Exception as e:
        q.put((rank, repr(e), None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_give_the_single_process_table(hip_device):
    """2 ranks sharing one device (gloo, host-staged gather): both return the single-process blocks."""
    from tests._spawn import spawn_and_wait
    from tests.test_gpu_gauc import _port
    _, _, ref = R.case("ctr", 4099)
    res = sorted(spawn_and_wait(_rank_worker, args=(_port(),), timeout=240.0, nprocs=2, rank_args=True),
                 key=lambda r: r[0])
    assert all(r[1] == "ok" for r in res), res
    for _, _, blocks in res:
        assert R.same_blocks(blocks, ref) is None
