"""CPU tests of the per-user list entry points (csrc/recommend.hip: fbn_rec_fields_list,
fbn_rec_topk_list, fbn_rec_rank_list): the argument checks that precede any device call (null pointers,
no GPU here), and the shape checks of Recommender's ``*_lists`` methods."""
import pytest
import torch

FBN_ERR_ARG = 1


def _h():
    from ctr_recommendation_amd import _lib
    return _lib.lib()


def _fields(h, D=16, R=3, ldc=240, U=3, ldp=152, c0=0, Cc=100, M=1037):
    return h.fbn_rec_fields_list(None, None, None, None, None, None, 11, None, 5000, None, None, None, None, R, None,
                                 None, None, ldc, 0, None, None, U, None, ldp, c0, Cc, M, D, None)


def _topk(h, K=10, L=20, U=5, c0=0, Cc=400, ldp=1103, M=1037, ws_bytes=1 << 20):
    return h.fbn_rec_topk_list(None, U, c0, Cc, None, ldp, M, None, None, L, 1, K, None, None, ws_bytes, None, None,
                               None, None, None, None, None)


def _rank(h, L=20, U=5, C=1100, ld=1103, ldp=1103, M=1037):
    return h.fbn_rec_rank_list(None, ld, U, C, None, ldp, M, None, None, L, 1, None, None, None, None, None)


def _refused(h, rc, who):
    assert rc == FBN_ERR_ARG
    assert who in h.fbn_last_error(), h.fbn_last_error()


@pytest.mark.parametrize("D", [0, 8, 48, 512])
def test_fields_list_refuses_unsupported_dim(D):
    h = _h()
    _refused(h, _fields(h, D=D), b"fbn_rec_fields_list")
    assert b"16,32,64,128,256" in h.fbn_last_error()


def test_fields_list_refuses_bad_senet_width_stride_and_list_geometry():
    h = _h()
    for kw in ({"R": 0}, {"R": 9}, {"ldc": 242}, {"c0": -1}, {"ldp": 99}, {"c0": 100, "Cc": 53},
               {"M": -1}):
        _refused(h, _fields(h, **kw), b"fbn_rec_fields_list")
    _refused(h, _fields(h, U=1 << 16, Cc=1 << 15, ldp=1 << 15), b"fbn_rec_fields_list")      # 2^31 pair rows
    assert b"31 bits" in h.fbn_last_error()


@pytest.mark.parametrize("K", [0, 257])
def test_topk_list_refuses_k_outside_1_256(K):
    h = _h()
    _refused(h, _topk(h, K=K), b"fbn_rec_topk_list")
    assert b"K must be in 1..256" in h.fbn_last_error()


def test_topk_list_refuses_long_history_list_geometry_and_small_workspace():
    h = _h()
    _refused(h, _topk(h, L=33), b"fbn_rec_topk_list")
    assert b"L must be in 0..32" in h.fbn_last_error()
    _refused(h, _topk(h, c0=-1), b"fbn_rec_topk_list")
    _refused(h, _topk(h, c0=800, Cc=400, ldp=1103), b"fbn_rec_topk_list")       # ldp < c0 + Cc
    assert b"ldp >= c0 + Cc" in h.fbn_last_error()
    _refused(h, _topk(h, M=-1), b"fbn_rec_topk_list")
    need = h.fbn_rec_topk_workspace_size(5, 400, 10)
    assert need == 5 * 1 * 10 * 8
    _refused(h, _topk(h, ws_bytes=need - 1), b"fbn_rec_topk_list")
    assert b"workspace" in h.fbn_last_error()


def test_rank_list_refuses_long_history_and_short_strides():
    h = _h()
    _refused(h, _rank(h, L=33), b"fbn_rec_rank_list")
    assert b"L must be in 0..32" in h.fbn_last_error()
    _refused(h, _rank(h, ld=1099), b"fbn_rec_rank_list")                         # ld < C
    assert b"ld >= C" in h.fbn_last_error()
    _refused(h, _rank(h, ldp=1099), b"fbn_rec_rank_list")                        # ldp < C
    _refused(h, _rank(h, C=-1), b"fbn_rec_rank_list")
    _refused(h, _rank(h, M=-1), b"fbn_rec_rank_list")
    _refused(h, _rank(h, U=65536), b"fbn_rec_rank_list")


def test_empty_list_problems_launch_nothing():
    """U = 0 (and for the fields Cc = 0) return before any device call (this process has no GPU)."""
    h = _h()
    assert _fields(h, U=0) == 0
    assert _fields(h, Cc=0) == 0
    assert _topk(h, U=0, ws_bytes=0) == 0
    assert _rank(h, U=0) == 0


def test_the_catalogue_entry_points_keep_their_messages():
    """The list entry points share the catalogue ones' checks; each names itself."""
    h = _h()
    assert h.fbn_rec_topk(None, 3, 0, 1037, None, None, 20, 1, 0, None, None, 1 << 20, None, None, None, None, None,
                          None) == FBN_ERR_ARG
    assert b"fbn_rec_topk: K must be in 1..256" in h.fbn_last_error()
    assert h.fbn_rec_fields(None, None, None, None, None, None, 11, None, 5000, None, None, None, None, 3, None, None,
                            None, 242, 0, None, None, 3, 0, 1037, 16, None) == FBN_ERR_ARG
    assert b"fbn_rec_fields:" in h.fbn_last_error()


def test_list_methods_validate_shapes_before_touching_a_device():
    from ctr_recommendation_amd import recommend
    seq = torch.zeros((3, 20), dtype=torch.int64)
    cand = torch.zeros((3, 7), dtype=torch.int64)
    assert recommend._check_lists(seq, cand, "item_id") == (3, 7)
    assert recommend._check_lists(None, cand[:1], "index", target_slot=torch.zeros(1), k=256) == (1, 7)
    bad = [dict(by="name"), dict(k=0), dict(k=257), dict(candidates=cand[:2]), dict(candidates=cand[0]),
           dict(candidates=cand[:, :0]), dict(candidates=cand.float()), dict(target_slot=torch.zeros(2)),
           dict(item_seq=seq[0]), dict(item_seq=None)]
    for kw in bad:
        args = {"item_seq": seq, "candidates": cand, "by": "item_id", **kw}
        with pytest.raises(ValueError):
            recommend._check_lists(**args)
    for name in ("score_lists", "topk_lists", "rank_lists", "evaluate_sampled"):
        assert callable(getattr(recommend.Recommender, name))
