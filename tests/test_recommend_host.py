"""CPU tests of the serving entry points (csrc/recommend.hip): argument checks that precede any
device call (null pointers, no GPU here) and the host-only workspace query."""
import pytest

FBN_ERR_ARG = 1


def _h():
    from ctr_recommendation_amd import _lib
    return _lib.lib()


def _topk(h, K, L=20, ws_bytes=1 << 20):
    return h.fbn_rec_topk(None, 3, 0, 1037, None, None, L, 1, K, None, None, ws_bytes, None, None, None, None, None,
                          None)


@pytest.mark.parametrize("K", [0, 257, -1])
def test_topk_refuses_k_outside_1_256(K):
    h = _h()
    assert _topk(h, K) == FBN_ERR_ARG
    assert b"K must be in 1..256" in h.fbn_last_error()


def test_topk_refuses_long_history_and_small_workspace():
    h = _h()
    assert _topk(h, 10, L=33) == FBN_ERR_ARG
    assert b"L must be in 0..32" in h.fbn_last_error()
    need = h.fbn_rec_topk_workspace_size(3, 1037, 10)
    assert _topk(h, 10, ws_bytes=need - 1) == FBN_ERR_ARG
    assert b"workspace" in h.fbn_last_error()


def test_hist_pool_refuses_long_history_and_bad_dim():
    h = _h()
    assert h.fbn_rec_hist_pool(None, None, 5000, None, None, 3, 33, 128, None) == FBN_ERR_ARG
    assert b"L must be in 0..32" in h.fbn_last_error()
    assert h.fbn_rec_hist_pool(None, None, 5000, None, None, 3, 20, 48, None) == FBN_ERR_ARG
    assert b"16,32,64,128,256" in h.fbn_last_error()


@pytest.mark.parametrize("D", [0, 8, 48, 512])
def test_item_cache_and_fields_refuse_unsupported_dim(D):
    h = _h()
    assert h.fbn_rec_item_cache(None, None, None, None, None, None, 1e-5, 11, 5000, None, None, 1037, D,
                                None) == FBN_ERR_ARG
    assert b"fbn_rec_item_cache" in h.fbn_last_error() and b"16,32,64,128,256" in h.fbn_last_error()
    assert h.fbn_rec_fields(None, None, None, None, None, None, 11, None, 5000, None, None, None, None, 3, None, None,
                            None, 15 * 16, 0, None, None, 3, 0, 1037, D, None) == FBN_ERR_ARG
    assert b"fbn_rec_fields" in h.fbn_last_error() and b"16,32,64,128,256" in h.fbn_last_error()


def test_fields_refuses_bad_senet_width_and_stride():
    h = _h()
    for R, ldc in ((0, 240), (9, 240), (3, 242)):
        assert h.fbn_rec_fields(None, None, None, None, None, None, 11, None, 5000, None, None, None, None, R, None,
                                None, None, ldc, 0, None, None, 3, 0, 1037, 16, None) == FBN_ERR_ARG
        assert b"fbn_rec_fields" in h.fbn_last_error()


def test_empty_problems_launch_nothing():
    """M = 0 / U = 0 return before any device call (this process has no GPU)."""
    h = _h()
    assert h.fbn_rec_item_cache(None, None, None, None, None, None, 1e-5, 11, 5000, None, None, 0, 128, None) == 0
    assert h.fbn_rec_hist_pool(None, None, 5000, None, None, 0, 20, 128, None) == 0
    assert h.fbn_rec_fields(None, None, None, None, None, None, 11, None, 5000, None, None, None, None, 3, None, None,
                            None, 240, 0, None, None, 0, 0, 1037, 16, None) == 0
    assert h.fbn_rec_topk(None, 0, 0, 1037, None, None, 20, 1, 10, None, None, 0, None, None, None, None, None,
                          None) == 0


def test_topk_workspace_query_is_host_only_and_monotone():
    h = _h()
    size = h.fbn_rec_topk_workspace_size
    assert size(3, 1037, 10) == 3 * 2 * 10 * 8          # two 1024-candidate segments per user
    assert size(1, 1, 1) == 8
    assert size(3, 1037, 0) == 0 and size(3, 1037, 257) == 0
    prev = 0
    for U, Mc, K in [(1, 1, 1), (1, 1024, 1), (1, 1025, 1), (2, 1025, 1), (2, 1025, 10), (64, 91718, 10),
                     (64, 91718, 256)]:
        s = size(U, Mc, K)
        assert s >= prev and s > 0
        prev = s
    for K in range(1, 256):
        assert size(5, 3000, K) <= size(5, 3000, K + 1)
    for Mc in (1, 1023, 1024, 1025, 4096, 91718):
        assert size(5, Mc, 10) <= size(5, Mc + 1, 10) and size(5, Mc, 10) <= size(6, Mc, 10)


def test_recommender_module_validates_before_touching_a_device():
    from ctr_recommendation_amd import recommend
    assert recommend.K_MAX == 256 and recommend.L_MAX == 32
    with pytest.raises(RuntimeError, match="HIP device"):
        recommend.Recommender({}, {"embedding_dim": 16}, {}, device="cpu")
