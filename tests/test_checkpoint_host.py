"""Full-state checkpoints, the parts that need no GPU (ctr_recommendation_amd/checkpoint.py, DESIGN.md
§22): the host form of the state digest (the reference fbn_digest_u64 is tested against), the file
layer (atomic writes, ``latest`` last, fallback, pruning, the offline verifier) over a stub trainer,
and the loader's shuffle position.  Every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

from ctr_recommendation_amd import checkpoint as ck
from ctr_recommendation_amd.checkpoint import digest_host

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def _mix64(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def _formula(words, base=0):
    """The digest's definition in Python integers."""
    return sum(_mix64((base + i + 1) * G + int(w)) for i, w in enumerate(words)) & M64


def _fake_state(step=0, V=64, d=16, seed=0):
    """A training state of numpy-backed CPU tensors in FiBiNETTrainer.training_state()'s layout."""
    rng = np.random.default_rng(seed + step)
    t = {"E": rng.standard_normal((V, d)).astype(np.float32), "Em": rng.standard_normal((V, d)).astype(np.float32),
         "Ev": rng.random((V, d)).astype(np.float32), "flat_p": rng.standard_normal(203).astype(np.float32),
         "flat_m": rng.standard_normal(203).astype(np.float32), "flat_v": rng.random(203).astype(np.float32),
         "mlp.1.num_batches_tracked": np.array(step, dtype=np.int64), "step_dev": np.array([step], dtype=np.int32),
         "rng": np.array([12345, 4 * step], dtype=np.int64)}
    state = {k: torch.from_numpy(v) for k, v in t.items()}
    state["digests"] = {k: digest_host(v) for k, v in t.items()}
    state["meta"] = {"host_step": step, "rank": 0, "world": 1, "d": d, "V": V, "sync_bn": True}
    return state


class _Stub:
    """What the file layer needs of a trainer."""
    rank, world, group = 0, 1, None

    def __init__(self):
        self.step, self.loaded = 0, None

    def training_state(self):
        return _fake_state(self.step)

    def load_training_state(self, state):
        self.loaded = state


def test_digest_host_properties():
    st = _fake_state(3)
    assert digest_host(np.zeros(0, dtype=np.float32)) == 0
    assert digest_host(np.zeros(0, dtype=np.int64), base=77) == 0
    w = st["E"].numpy().reshape(-1).view(np.uint32)
    assert digest_host(w) == _formula(w)
    # chunks compose through `base`, at a split that is no multiple of 4
    for k in (1, 2, 3, 5, 1001 % w.size):
        assert (digest_host(w[:k]) + digest_host(w[k:], base=k)) & M64 == digest_host(w)
    # 64-bit index arithmetic: a base just below 2^32, the indices crossing it
    five = np.array([7, 0, 0xFFFFFFFF, 3, 0x80000000], dtype=np.uint32)
    base = 2 ** 32 - 2
    assert digest_host(five, base=base) == _formula(five, base)
    assert digest_host(five, base=base) != digest_host(five, base=base - 2 ** 32)     # no 32-bit wrap of the index
    # position matters: two swapped words change the digest (a plain sum of the words would not)
    sw = w.copy()
    assert sw[10] != sw[11]
    sw[[10, 11]] = sw[[11, 10]]
    assert digest_host(sw) != digest_host(w) and int(sw.sum()) == int(w.sum())
    # float32, int32 and int64 buffers: the same words give the same digest
    i32 = np.arange(-50, 50, dtype=np.int32)
    assert digest_host(i32) == _formula(i32.view(np.uint32))
    assert digest_host(i32.view(np.float32)) == digest_host(i32)
    i64 = np.array([-1, 2 ** 40 + 5, 0, 9], dtype=np.int64)
    assert digest_host(i64) == _formula(i64.view(np.uint32)) == digest_host(i64.view(np.float64))
    assert digest_host(st["mlp.1.num_batches_tracked"].numpy()) == _formula([3, 0])
    # the chunked evaluation (4 M words per chunk) composes too
    big = np.random.default_rng(1).integers(0, 2 ** 32, size=(1 << 22) + 13, dtype=np.uint32)
    assert digest_host(big) == (digest_host(big[:99]) + digest_host(big[99:], base=99)) & M64
    with pytest.raises(ValueError):
        digest_host(np.zeros(3, dtype=np.float16))


def test_file_layer_roundtrip_fallback_keep_and_verify(tmp_path):
    root = str(tmp_path / "state")
    tr = _Stub()
    for step in (4, 8, 12):
        tr.step = step
        sdir = ck.save(root, tr, extra={"epoch": 1, "steps": step, "history": [[1, 0.5, None]], "bits": -(2 ** 62),
                                        "loader": {"epoch": 1, "gen_state": torch.arange(5, dtype=torch.uint8)}},
                       keep=2)
        assert os.path.basename(sdir) == f"step-{step:08d}"
        assert open(os.path.join(root, "latest")).read().strip() == f"step-{step:08d}"
    # keep = 2: the two newest step directories stay
    assert sorted(n for n in os.listdir(root) if n.startswith("step-")) == ["step-00000008", "step-00000012"]
    assert not [n for n in os.listdir(os.path.join(root, "step-00000012")) if ".tmp" in n]
    # the files load under weights_only=True and round-trip state and extra
    blob = torch.load(os.path.join(root, "step-00000012", "rank0.pt"), weights_only=True)
    assert set(blob) == {"state", "extra"}
    got = _Stub()
    extra = ck.load(root, got)
    assert extra["steps"] == 12 and extra["history"] == [[1, 0.5, None]] and extra["bits"] == -(2 ** 62)
    assert torch.equal(extra["loader"]["gen_state"], torch.arange(5, dtype=torch.uint8))
    want = _fake_state(12)
    assert got.loaded["meta"] == want["meta"] and got.loaded["digests"] == want["digests"]
    for k, v in want.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(got.loaded[k], v) and got.loaded[k].dtype == v.dtype, k
    man = json.load(open(os.path.join(root, "step-00000012", "manifest.json")))
    assert man["step"] == 12 and man["world"] == 1 and man["files"] == ["rank0.pt"]
    assert man["digests"]["0"]["Em"] == f"{want['digests']['Em']:016x}"
    assert ck.verify(root, out=lambda s: None) == 0
    # ``latest`` is written last: a save that died before its manifest is passed over
    os.remove(os.path.join(root, "step-00000012", "manifest.json"))
    got = _Stub()
    assert ck.load(root, got)["steps"] == 8 and got.loaded["meta"]["host_step"] == 8
    os.remove(os.path.join(root, "step-00000008", "rank0.pt"))
    with pytest.raises(FileNotFoundError):
        ck.load(root, _Stub())


def test_verify_names_the_corrupt_tensor(tmp_path, capsys):
    root = str(tmp_path / "state")
    tr = _Stub()
    tr.step = 5
    ck.save(root, tr)
    assert ck.main(["verify", root]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == len(_fake_state(5)["digests"]) and all(ln.endswith("OK") for ln in lines)
    # one byte of one saved tensor flipped
    path = os.path.join(root, "step-00000005", "rank0.pt")
    blob = torch.load(path, weights_only=True)
    blob["state"]["Em"].view(torch.uint8).reshape(-1)[37] ^= 0x10
    torch.save(blob, path)
    assert ck.main(["verify", root]) != 0
    bad = [ln for ln in capsys.readouterr().out.splitlines() if "MISMATCH" in ln]
    assert len(bad) == 1 and " Em " in bad[0]
    assert ck.main(["frobnicate"]) == 2


class _DS:
    """A dataset stand-in on the CPU: the loader's batches are then its row indices."""
    has_label = True
    device = torch.device("cpu")

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def _cpu_loader(shuffle=True, seed=5):
    from ctr_recommendation_amd.loader import DeviceLoader
    dl = DeviceLoader(_DS(1000), None, 128, shuffle=shuffle, seed=seed)
    dl.collate = lambda rows, flag=None: (rows.clone(), None)     # no device: a batch is its rows
    return dl


def test_loader_state_resumes_the_epoch_permutation():
    ref = _cpu_loader()
    epochs = [[b for b, _ in ref] for _ in range(3)]             # the uninterrupted run's batches
    assert len(epochs[0]) == 8 and not torch.equal(epochs[0][0], epochs[1][0])
    a = _cpu_loader()
    for _ in a:
        pass
    it = iter(a)                                                  # epoch 2, stopped mid-way, one batch ahead
    used = [next(it)[0] for _ in range(4)]
    sd = a.state_dict()
    assert sd["epoch"] == 1 and sd["gen_state"].dtype == torch.uint8
    r = _cpu_loader(seed=99)                                      # a fresh loader, seeded differently
    r.load_state_dict(sd, skip=3)
    rest = [b for b, _ in r]
    assert len(rest) == 5 and all(torch.equal(x, y) for x, y in zip(rest, epochs[1][3:]))
    assert torch.equal(used[3], rest[0]) and r.epoch == 2
    nxt = [b for b, _ in r]                                       # and the following epoch, whole
    assert len(nxt) == 8 and all(torch.equal(x, y) for x, y in zip(nxt, epochs[2]))
    # between epochs: the next epoch's permutation
    b = _cpu_loader()
    for _ in b:
        pass
    sd = b.state_dict()
    assert sd["epoch"] == 1
    r = _cpu_loader(seed=98)
    r.load_state_dict(sd)
    assert all(torch.equal(x[0], y) for x, y in zip(r, epochs[1]))
    # unshuffled loaders carry only the epoch
    u = _cpu_loader(shuffle=False)
    for _ in u:
        pass
    assert u.state_dict() == {"epoch": 1}
    v = _cpu_loader(shuffle=False)
    v.load_state_dict({"epoch": 1}, skip=6)
    assert [int(x[0][0]) for x in v] == [768, 896] and v.epoch == 2
    with pytest.raises(ValueError):
        v.load_state_dict({"epoch": 1}, skip=9)
