"""The Stable-Diffusion warp ablation without a GPU: the numpy restatement (tests/sdwarp_ref.py) against the fixture recorded
from the reference (tests/golden/sd_warp.npz), and the library's HOST tables against the restatement, bit for bit."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import sdwarp_ref as R  # noqa: E402
import grounding_ref as G  # noqa: E402
from oracle import warp_oracle as O  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "sd_warp.npz"))
STEPS = (981, 801, 621)
LAYERS = (0, 1, 2)
TOP_K = 5
F32, F64 = np.float32, np.float64


def inputs(dtype):
    """The fixture's tensors [B,heads,HW,tokens] per (step, layer) in float32 or float16, and their [H,W]."""
    out, shapes = {}, {}
    for s in STEPS:
        for k in LAYERS:
            a = GOLD[f"in_{s}_{k}"]
            shapes[(s, k)] = a.shape[2:4]
            a = a.reshape(a.shape[0], a.shape[1], -1, a.shape[-1])
            out[(s, k)] = a.astype(np.float16) if dtype == "f16" else a
    return out, shapes


def sum_bound(a, dtype):
    """|any float32-or-better summation of a over (B, heads, HW) - another| per token: n * 2^-24 * sum|v| (n terms), the
    bound for any float32 summation order; plus one float16 ulp of the result when the result is stored in float16."""
    v = np.abs(a.astype(F64))
    n = a.shape[0] * a.shape[1] * a.shape[2]
    b = n * 2.0 ** -24 * v.sum(axis=(0, 1, 2))
    if dtype == "f16":
        b = b + np.spacing(np.abs(a.astype(F64).sum(axis=(0, 1, 2))).astype(np.float16)).astype(F64)
    return b


def restated_importance(dtype, mode):
    x, _ = inputs(dtype)
    sums = {k: R.xattn_reduce(a, dtype)[0] for k, a in x.items()}
    bounds = {k: sum_bound(a, dtype) for k, a in x.items()}
    if mode == "last":
        key = (max(STEPS), max(LAYERS))
        return sums[key], bounds[key]
    steps = STEPS if mode == "all" else [s for s in STEPS if s in (801, 621)]
    layers = LAYERS if mode == "all" else sorted(LAYERS)[-2:]
    keys = [(s, k) for s in steps for k in layers]
    got = np.mean([sums[k] for k in keys], axis=0)
    # np.mean of m vectors: the mean of the per-tensor bounds, plus the (m + 1) roundings of its own arithmetic
    ulp = 2.0 ** -24 if dtype == "f32" else 2.0 ** -11
    bound = np.mean([bounds[k] for k in keys], axis=0) + (len(keys) + 1) * ulp * np.abs(got.astype(F64))
    return got, bound


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("mode", ["all", "sel", "last"])
def test_restated_importance_matches_reference(dtype, mode):
    got, bound = restated_importance(dtype, mode)
    want = GOLD[f"imp_{mode}_{dtype}"]
    assert got.dtype == want.dtype
    err = np.abs(got.astype(F64) - want.astype(F64))
    print(f"importance {mode} {dtype}: max err {err.max():.3e}, smallest bound {bound.min():.3e}")
    assert np.all(err <= bound)
    if mode == "all":
        assert list(np.argsort(got)[-TOP_K:][::-1]) == list(GOLD[f"top_{dtype}"])
        imp = np.sort(want.astype(F64))[::-1]
        assert imp[TOP_K - 1] - imp[TOP_K] > 0.01 * imp[TOP_K - 1]      # the planted gap: no test depends on a tie


def aggregated(dtype, hw_toks=None):
    """The restatement's aggregated map, and a bound on its distance from any evaluation whose sums are float32-or-better:
    every un-normalised pixel is a sum of n = B * heads * k terms with the bound above (plus, float16, one ulp), the mean
    over maps keeps it, and (m - min) / (max - min + 1e-9) turns an absolute error d of every pixel into at most
    4 d / range, plus the four float32 roundings of the mean and the normalisation."""
    x, shapes = inputs(dtype)
    top = list(GOLD[f"top_{dtype}"])
    keys = [(s, max(LAYERS)) for s in sorted(STEPS)]
    if hw_toks is None:
        hw_toks = [R.xattn_reduce(x[k], dtype)[1].reshape(*shapes[k], -1) for k in keys]
    got = R.aggregate_from_hw_tok(hw_toks, top, dtype)
    raw, d = [], []
    for k in keys:
        a = x[k][..., top].astype(F64)
        raw.append(a.sum(axis=(0, 1, 3)).reshape(shapes[k]))
        b = a.shape[0] * a.shape[1] * len(top) * 2.0 ** -24 * np.abs(a).sum(axis=(0, 1, 3)).reshape(shapes[k])
        if dtype == "f16":
            b = b + np.spacing(raw[-1].astype(np.float16)).astype(F64)
        d.append(b)
    m = np.mean(raw, axis=0)
    bound = 4 * np.mean(d, axis=0).max() / (m.max() - m.min()) + 4 * 2.0 ** -24
    return got, bound


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_restated_aggregate_matches_reference(dtype):
    got, bound = aggregated(dtype)
    want = GOLD[f"agg_{dtype}"]
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(F64) - want.astype(F64)).max()
    print(f"aggregate {dtype}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("transform", ["identity", "square", "sqrt", "exp", "log"])
@pytest.mark.parametrize("inverse", [False, True])
def test_axis_maps_of_the_ablation(transform, inverse):
    """The (tx, ty) the ablation's warp_image_by_attention hands to cv2.remap: new_method's grid construction (the oracle's
    maps_from_attention, the code reused unchanged) except in the near-zero fallback, which the ablation resolves with
    uniform profiles of total w / h (here: log without the inverse, whose profiles are negative)."""
    mx, my = R.maps_from_attention(GOLD["warp_att"], 17, 13, transform, 1.5, 2.0, inverse)
    assert np.array_equal(mx, GOLD[f"warp_tx_{transform}_{int(inverse)}"])
    assert np.array_equal(my, GOLD[f"warp_ty_{transform}_{int(inverse)}"])
    ox, oy = O.maps_from_attention(GOLD["warp_att"], 17, 13, transform, 1.5, 2.0, inverse)
    fallback = transform == "log" and not inverse
    assert np.array_equal(mx, ox) != fallback and np.array_equal(my, oy) != fallback
    if fallback:
        assert np.array_equal(mx, R.uniform_axis_map(10, 17)) and np.array_equal(my, R.uniform_axis_map(12, 13))


def test_step_scale_sequence():
    for it in (1, 3):
        want = GOLD[f"step_scale_{it}"]
        assert want.shape == (it,)
        assert np.array_equal(want, np.full(it, 2.0 / max(1, it)))


def test_versions_recorded():
    assert len(GOLD["versions"]) == 2


# ---- the library's HOST helpers ------------------------------------------------------------------------------------------
OUT_SIDES = (1, 2, 3, 5, 7, 16, 24, 31, 64, 65, 100, 255, 256, 257, 513)


def lib_cubic(n_in, n_out):
    from attwarp_amd import _tables
    return _tables.cubic_tables_host(n_in, n_out)


def test_cubic_coeffs_bit_for_bit():
    cache = {}

    def coeff(f):
        key = F32(f).tobytes()
        if key not in cache:
            cache[key] = R.interpolate_cubic(f)
        return cache[key]
    cases = [(n_in, n_out) for n_in in range(1, 65) for n_out in OUT_SIDES] + [(4096, 500)]
    assert len(OUT_SIDES) == 15
    for n_in, n_out in cases:
        ofs, co = lib_cubic(n_in, n_out)
        scale = 1.0 / (float(n_out) / n_in)
        for d in range(n_out):
            f = F32((d + 0.5) * scale - 0.5)
            s = math.floor(f)
            assert ofs[d] == s, (n_in, n_out, d)
            want = coeff(F32(f - F32(s)))
            assert co[d].tobytes() == want.tobytes(), (n_in, n_out, d, co[d], want)
    ofs, co = R.cubic_coeffs(24, 100)
    lo, lc = lib_cubic(24, 100)
    assert np.array_equal(ofs, lo) and co.tobytes() == lc.tobytes()


def test_cubic_coeffs_refusals():
    from attwarp_amd import _lib
    ofs = np.zeros(4, np.int32)
    co = np.zeros((4, 4), np.float32)
    with pytest.raises(_lib.AttWarpError):
        _lib.call("attwarp_cubic_coeffs", 0, 4, ofs.ctypes.data, co.ctypes.data)
    with pytest.raises(_lib.AttWarpError):
        _lib.call("attwarp_cubic_coeffs", 4, 4, None, co.ctypes.data)
    _lib.call("attwarp_cubic_coeffs", 4, 4, ofs.ctypes.data, co.ctypes.data)
    assert np.array_equal(ofs, np.arange(4)) and np.array_equal(co[:, 1], np.ones(4, np.float32))


def test_gaussian_taps():
    from attwarp_amd import _lib
    t = np.zeros(5, np.float32)
    _lib.call("attwarp_gaussian5_taps", 1.0, t.ctypes.data)
    want = R.gaussian5_taps(1.0)
    assert t.tobytes() == want.tobytes()
    e = np.exp(-0.5 * (np.arange(5) - 2.0) ** 2)
    assert np.allclose(t, e / e.sum(), rtol=1e-7) and t[0] == t[4] and t[1] == t[3]
    with pytest.raises(_lib.AttWarpError):
        _lib.call("attwarp_gaussian5_taps", 0.0, t.ctypes.data)


def test_lanczos4_coeffs_unchanged():
    """attwarp_lanczos4_coeffs shares its source-coordinate code with the cubic tables now: same bits as the restatement on
    the sides its own test uses."""
    from attwarp_amd import _tables
    for n_in, n_out in [(24, 1), (24, 24), (24, 336), (24, 500), (24, 18), (24, 27), (7, 64), (64, 1000), (1, 5)]:
        ofs, co = _tables.lanczos4_tables_host(n_in, n_out)
        ro, rc = G.lanczos4_coeffs(n_in, n_out)
        assert np.array_equal(ofs, ro) and co.tobytes() == rc.tobytes(), (n_in, n_out)


def test_chunk_of_the_reduce():
    from attwarp_amd import sd_warp
    for tokens in (1, 7, 64, 77, 256):
        assert sd_warp.xattn_chunk(tokens) == R.xattn_chunk(tokens)
    with pytest.raises(ValueError):
        sd_warp.xattn_chunk(0)
    with pytest.raises(ValueError):
        sd_warp.xattn_chunk(257)


def test_restatement_edges():
    assert np.array_equal(R.reflect101(np.array([-2, -1, 0, 1, 2, 3]), 2), [0, 1, 0, 1, 0, 1])
    assert np.array_equal(R.reflect101(np.array([-2, -1, 0, 1, 2]), 1), [0, 0, 0, 0, 0])
    assert np.array_equal(R.reflect101(np.array([-2, -1, 5, 6]), 5), [2, 1, 3, 2])
    c = np.full((3, 4), 2.5, F32)
    assert np.array_equal(R.minmax_normalize(c), np.zeros((3, 4), F32))
    c[1, 1] = np.nan
    assert np.isnan(R.minmax_normalize(c)).all()
    a = np.arange(12, dtype=F32).reshape(3, 4)
    assert np.array_equal(R.resize_cubic(a, 4, 3), a)
    b = R.blur5(np.full((5, 7), 3.0, F32))
    assert np.allclose(b, 3.0, rtol=1e-6)


def test_cpu_tensors_raise():
    import torch
    from attwarp_amd import sd_warp
    t = torch.zeros(1, 1, 2, 2, 3)
    with pytest.raises(RuntimeError):
        sd_warp.reduce_captured_maps({0: {0: t}})
    with pytest.raises(RuntimeError):
        sd_warp.resize_cubic([torch.zeros(2, 2)], [(3, 3)])
    with pytest.raises(RuntimeError):
        sd_warp.minmax_normalize([torch.zeros(2, 2)])
    with pytest.raises(RuntimeError):
        sd_warp.iterative_warp([torch.zeros(2, 2, 3, dtype=torch.uint8)], [torch.zeros(2, 2)])
    assert sd_warp.ATTENTION_TRANSFORM == "identity"
    assert sd_warp.set_transform_function("nope") == "nope" and sd_warp.ATTENTION_TRANSFORM == "identity"
    with pytest.raises(FileNotFoundError):
        sd_warp.save_warped_image(os.path.join(HERE, "no_such_image.png"), np.zeros((2, 2), np.float32), "unused.png")
