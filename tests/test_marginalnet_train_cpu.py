"""CPU tests of MarginalNet's training tail: argument validation of the backward entry points (no GPU needed: they
return before any launch) and the float64 restatements of the two backwards (tests/marginalnet_train_ref.py) against
torch's float64 CPU autograd of the reference formulas (MN/model.py:8-14, 80-88)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from marginalnet_train_ref import film_axis_means_backward, safe_softmax_backward

E_ARG, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    from attwarp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_training_tail_abi_validation_without_gpu(lib):
    p = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    F32, F16, BF16, U8 = 0, 1, 2, 3
    # film_axis_means_t (v, v_dtype, gamma_beta, gb_dtype, B, Ch, H, W, vx, vy, stream)
    assert lib.attwarp_film_axis_means_t(None, F32, p, F32, 1, 2, 4, 4, p, p, None) == E_ARG
    assert lib.attwarp_film_axis_means_t(p, F32, p, F32, 1, 2, 4, 4, p, None, None) == E_ARG
    assert lib.attwarp_film_axis_means_t(p, U8, p, F32, 1, 2, 4, 4, p, p, None) == E_ARG
    assert lib.attwarp_film_axis_means_t(p, F16, p, 7, 1, 2, 4, 4, p, p, None) == E_ARG
    assert lib.attwarp_film_axis_means_t(p, BF16, p, F16, 1, 0, 4, 4, p, p, None) == E_ARG
    assert lib.attwarp_film_axis_means_t(p, F16, p, F16, 1, 2, 64, 64, p, p, None) == E_UNSUPPORTED
    # film_axis_means_backward (v, v_dtype, gb, gb_dtype, gx, gy, B, Ch, H, W, dv, dgb, stream)
    assert lib.attwarp_film_axis_means_backward(p, F32, p, F32, None, p, 1, 2, 4, 4, p, p, None) == E_ARG
    assert lib.attwarp_film_axis_means_backward(p, F32, p, F32, p, p, 1, 2, 4, 4, p, None, None) == E_ARG
    assert lib.attwarp_film_axis_means_backward(p, 4, p, F32, p, p, 1, 2, 4, 4, p, p, None) == E_ARG    # float64
    assert lib.attwarp_film_axis_means_backward(p, F32, p, -1, p, p, 1, 2, 4, 4, p, p, None) == E_ARG
    assert lib.attwarp_film_axis_means_backward(p, F32, p, F32, p, p, 1, 2, -3, 4, p, p, None) == E_ARG
    assert lib.attwarp_film_axis_means_backward(p, F16, p, F16, p, p, 1, 2, 63, 65, p, p, None) == E_UNSUPPORTED
    # safe_softmax_backward (logits, g, B, N, eps, dlogits, stream)
    assert lib.attwarp_safe_softmax_backward(None, p, 1, 4, 1e-6, p, None) == E_ARG
    assert lib.attwarp_safe_softmax_backward(p, None, 1, 4, 1e-6, p, None) == E_ARG
    assert lib.attwarp_safe_softmax_backward(p, p, 1, 4, 1e-6, None, None) == E_ARG
    assert lib.attwarp_safe_softmax_backward(p, p, 0, 4, 1e-6, p, None) == E_ARG
    assert lib.attwarp_safe_softmax_backward(p, p, 1, 4097, 1e-6, p, None) == E_UNSUPPORTED
    from attwarp_amd import model
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.film_axis_means(torch.rand(2, 4, 6, 6, requires_grad=True), torch.rand(2, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.safe_softmax(torch.rand(2, 6, requires_grad=True))


def _torch_film(v, gb, gx, gy):
    v = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    gb = torch.tensor(gb, dtype=torch.float64, requires_grad=True)
    gamma, beta = gb.chunk(2, dim=1)                      # MN/model.py:80-88
    w = gamma[:, :, None, None] * v + beta[:, :, None, None]
    torch.autograd.backward([w.mean(dim=2), w.mean(dim=3)], [torch.from_numpy(gx), torch.from_numpy(gy)])
    return v.grad.numpy(), gb.grad.numpy()


@pytest.mark.parametrize("shape", [(2, 3, 24, 24), (1, 4, 7, 13), (3, 1, 1, 5)])
def test_film_backward_restatement_matches_torch_autograd(shape):
    B, Ch, H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    v = rng.standard_normal(shape)
    gb = rng.standard_normal((B, 2 * Ch))
    gx, gy = rng.standard_normal((B, Ch, W)), rng.standard_normal((B, Ch, H))
    dv, dgb, _ = film_axis_means_backward(v, gb, gx, gy)
    tv, tgb = _torch_film(v, gb, gx, gy)
    np.testing.assert_allclose(dv, tv, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(dgb, tgb, rtol=1e-12, atol=1e-13)


def _softmax_cases():
    rng = np.random.default_rng(31)
    rows = [rng.standard_normal(24) * 3 for _ in range(4)]
    rows[1][[3, 9]] = rows[1].max() + 1.0                 # two tied maxima
    rows[2][[0, 5, 17]] = [np.nan, np.inf, -np.inf]       # non-finite logits (nan_to_num -> 0)
    rows[3][:] = 0.5                                      # all tied
    rows.append(np.full(24, np.nan))                      # all NaN: every position is a tied max at 0
    rows.append(np.r_[np.full(12, -np.inf), rng.standard_normal(12) - 5])   # the zeros of -inf are the maxima
    return np.stack(rows)


@pytest.mark.parametrize("N", [1, 24, 336])
def test_safe_softmax_backward_restatement_matches_torch_autograd(N):
    from attwarp_amd.model import safe_softmax_stock
    rng = np.random.default_rng(N)
    x = _softmax_cases() if N == 24 else rng.standard_normal((5, N)) * 4
    g = rng.standard_normal(x.shape)
    g[0, 0] = 0.0
    for eps in (1e-6, 2.0):                               # eps = 2 > S2: the clamp branch (dd does not pass)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        out = safe_softmax_stock(xt, dim=1, eps=eps)
        out.backward(torch.from_numpy(g))
        want = xt.grad.numpy()
        got, _ = safe_softmax_backward(x, g, eps)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
        assert (got[~np.isfinite(x)] == 0).all()
