"""The per-axis kernels (axis.hip) and the profile kernels (profiles.hip) at the sizes their launchers document as limits:
16384 elements per axis, 8192 for the fused kernels, a low-resolution side of 64, a grid side of 64 (26 for
attn_reduce_and_maps) and 65535 images per launch.  Every limit has a case at it, one just below it (or at an irregular
size below it) and one above it that must be refused in the launcher's own words, never with a bare HIP error string.

Results are held to oracle/warp_oracle.py bit for bit (np.array_equal on the float32 values).  Two exceptions keep the
criteria of tests/test_gpu_parity.py: safe_softmax is held to rtol=5e-7, atol=1e-12 (test_safe_softmax), and for
sqrt / exp / log the fast profile kernels are held bit for bit to the generic kernel (the device libm is in both).
Cases: tests/axis_limit_cases.py (thin arrays: a limit on one axis, a handful of elements on the other)."""
import os

import numpy as np
import pytest
import torch

from attwarp_amd import _lib
from attwarp_amd._lib import AttWarpError
from oracle import warp_oracle as O
import axis_limit_cases as C

pytestmark = pytest.mark.gpu

F32 = np.float32
TRANSFORMS = ("identity", "square", "sqrt", "exp", "log")
TORCH_DT = {"uint8": torch.uint8, "float32": torch.float32, "float64": torch.float64}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert os.path.exists(_lib.LIB_PATH), "HIP library missing -- the product has no fallback"
    _lib.load()
    return torch.device("cuda:0")


def T(x, dev):
    return torch.from_numpy(np.array(x, order="C")).to(dev)        # (a copy: the cases are read-only arrays)


def N(t):
    return t.detach().cpu().numpy()


def same(got, ref, nan=False):
    got = N(got) if isinstance(got, torch.Tensor) else got
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref, equal_nan=nan)


# ================================ refusals (run first: no kernel is launched) ================================
def test_axis_lengths_above_the_limit_are_refused(dev):
    from attwarp_amd import checkpoint_utils as cu, model
    z = torch.zeros(2, C.MAX_L + 1, device=dev)
    with pytest.raises(AttWarpError, match=r"cdf_from_density: L=16385 > 16384"):
        cu.cdf_from_density(z)
    with pytest.raises(AttWarpError, match=r"make_strictly_increasing: N=16385 > 16384"):
        cu._make_strictly_increasing(z)
    with pytest.raises(AttWarpError, match=r"resample_cdf: N\+L=32769 too large"):
        cu.resample_cdf(z[:, :C.MAX_L], C.MAX_L + 1)
    with pytest.raises(AttWarpError, match=r"resample_cdf: N\+L=32769 too large"):
        cu.resample_cdf(z, C.MAX_L)
    with pytest.raises(AttWarpError, match=r"axis_map_from_cdf: L=16385 > 16384"):
        cu.axis_maps_from_cdf(z, z[:, :8], (8, 8))
    with pytest.raises(AttWarpError, match=r"axis_map_from_cdf: L=16385 > 16384"):
        cu.axis_maps_from_cdf(z[:, :8], z, (8, 8))
    with pytest.raises(AttWarpError, match=r"safe_softmax: N=16385 > 16384"):
        model.safe_softmax(z, dim=1)


def test_profile_sizes_above_the_limit_are_refused(dev):
    from attwarp_amd import checkpoint_utils as cu, new_method as nm, pipeline
    for dt in TORCH_DT.values():
        with pytest.raises(AttWarpError, match=r"axis_maps_from_attention: max\(h,w\)=16385 > 16384"):
            nm.attention_axis_maps(torch.zeros(2, 2, C.MAX_L + 1, device=dev, dtype=dt), 8, 8)
        with pytest.raises(AttWarpError, match=r"axis_maps_from_attention: max\(h,w\)=16385 > 16384"):
            nm.attention_axis_maps(torch.zeros(2, C.MAX_L + 1, 2, device=dev, dtype=dt), 8, 8)
    for hw in ((2, C.MAX_L + 1), (C.MAX_L + 1, 2)):
        with pytest.raises(AttWarpError, match=r"gt_marginals: H, W must be <= 16384"):
            cu.gt_marginals(torch.zeros(2, 1, *hw, device=dev))
    for out in ((24, 24), (1, 1)):
        with pytest.raises(AttWarpError, match=r"adaptive_avg_pool: W=16385 > 16384"):
            pipeline.adaptive_avg_pool2d(torch.zeros(2, 1, 3, C.MAX_L + 1, device=dev), out)


def test_fused_sizes_above_the_limit_are_refused(dev):
    from attwarp_amd import pipeline
    p64, p65 = torch.full((2, 64), 1 / 64, device=dev), torch.full((2, 65), 1 / 65, device=dev)
    with pytest.raises(AttWarpError, match=r"axis_maps_from_pdf: L_out=65 > 64"):
        pipeline.axis_maps_from_pdf(p65, p65, (128, 128))
    for hw in ((C.FUSED_MAX_L + 1, 64), (64, C.FUSED_MAX_L + 1)):
        with pytest.raises(AttWarpError, match=r"axis_maps_from_pdf: max\(W,H\)=8193 > 8192"):
            pipeline.axis_maps_from_pdf(p64, p64, hw, (8, 8))
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        with pytest.raises(AttWarpError, match=r"axis_maps_from_steps: grid side 65 > 64"):
            pipeline.axis_maps_from_attention_steps(torch.zeros(2, 2, 65 * 65, device=dev, dtype=dt), (128, 128))
        for hw in ((C.FUSED_MAX_L + 1, 64), (64, C.FUSED_MAX_L + 1)):
            with pytest.raises(AttWarpError, match=r"axis_maps_from_steps: max\(W,H\)=8193 > 8192"):
                pipeline.axis_maps_from_attention_steps(torch.zeros(2, 2, 64 * 64, device=dev, dtype=dt), hw, (8, 8))


def test_batches_above_the_limit_are_refused(dev):
    from attwarp_amd import checkpoint_utils as cu, new_method as nm, pipeline
    B = C.MAX_B + 1
    for dt in TORCH_DT.values():
        with pytest.raises(AttWarpError, match=r"axis_maps_from_attention: B > 65535"):
            nm.attention_axis_maps(torch.zeros(B, 8, 8, device=dev, dtype=dt), 8, 8)
    with pytest.raises(AttWarpError, match=r"gt_marginals: B > 65535"):
        cu.gt_marginals(torch.zeros(B, 1, 8, 8, device=dev))
    with pytest.raises(AttWarpError, match=r"axis_maps_from_steps: B > 65535"):
        pipeline.axis_maps_from_attention_steps(torch.zeros(2, B, 4, device=dev), (8, 8))
    with pytest.raises(AttWarpError, match=r"adaptive_avg_pool: oh/B > 65535"):
        pipeline.adaptive_avg_pool2d(torch.zeros(B, 1, 8, 8, device=dev), (2, 2))
    with pytest.raises(AttWarpError, match=r"adaptive_avg_pool: oh/B > 65535"):
        pipeline.adaptive_avg_pool2d(torch.zeros(2, 1, 8, 8, device=dev), (C.MAX_B + 1, 2))


# ================================ 1. unfused per-axis kernels ================================
@pytest.mark.parametrize("L", C.AXIS_LENGTHS)
def test_cdf_from_density_at_limits(dev, L):
    """Random densities (parallel scan), a row that forces the sequential scan, a spike plus a denormal, an all-zero row."""
    from attwarp_amd import checkpoint_utils as cu
    p = C.densities(L)
    assert same(cu.cdf_from_density(T(p, dev)), O.cdf_from_density(p))


@pytest.mark.parametrize("n", C.AXIS_LENGTHS)
def test_make_strictly_increasing_at_limits(dev, n):
    """A monotone CDF, a flat one (every step the eps / N floor), one with NaN / +inf / -inf, a decreasing one."""
    from attwarp_amd import checkpoint_utils as cu
    F = C.cdfs(n)
    assert same(cu._make_strictly_increasing(T(F, dev)), O.make_strictly_increasing(F))


@pytest.mark.parametrize("NL", C.RESAMPLE_NL)
def test_resample_cdf_at_limits(dev, NL):
    from attwarp_amd import checkpoint_utils as cu
    n, L = NL
    F = C.cdfs(n)
    assert same(cu.resample_cdf(T(F, dev), L), O.resample_cdf(F, L))


@pytest.mark.parametrize("L", C.AXIS_LENGTHS)
def test_axis_maps_from_cdf_at_limits(dev, L):
    """CDFs with equal neighbouring knots (the tie-break ramp) on x, strictly increasing ones on y; 1, 500 and 16384
    outputs."""
    from attwarp_amd import checkpoint_utils as cu
    Ft, Fs = C.map_cdfs(L)
    dFt, dFs = T(Ft, dev), T(Fs, dev)
    for n_out in C.MAP_N_OUT:
        mx, my = cu.axis_maps_from_cdf(dFt, dFs, (n_out, n_out))
        rx, ry = O.maps_from_cdf(Ft, Fs, (n_out, n_out))
        assert same(mx, rx) and same(my, ry), n_out


@pytest.mark.parametrize("n", C.AXIS_LENGTHS)
def test_safe_softmax_at_limits(dev, n):
    """Rows of +-80 logits, a row with NaN / +-inf, a constant row, a random row: the bound of test_safe_softmax
    (rtol=5e-7, atol=1e-12), and every row sums to 1 within N * 2^-24."""
    from attwarp_amd import model
    x = C.logits(n)
    got = N(model.safe_softmax(T(x, dev), dim=1, eps=1e-6))
    ref = O.safe_softmax(x)
    worst = np.abs(got.astype(np.float64) - ref).max()
    print(f"safe_softmax N={n}: max|gpu-oracle| = {worst:.3e}, row sums - 1 = {got.astype(np.float64).sum(1) - 1}")
    np.testing.assert_allclose(got, ref, rtol=5e-7, atol=1e-12)
    assert np.isfinite(got).all()
    assert np.abs(got.astype(np.float64).sum(1) - 1).max() <= n * 2.0 ** -24


# ================================ 2. profile kernels + finalize ================================
def _check_attention_maps(dev, a_dev, a_np, variants=(-1,), label=""):
    """attention_axis_maps on every transform, both inverse settings and both output sizes: the default route (and the
    forced ones of `variants`) bit for bit the generic kernel; identity / square bit for bit the oracle."""
    from attwarp_amd import new_method as nm
    for (nw, nh) in C.ATT_OUT_WH:
        for tr in TRANSFORMS:
            for inv in (False, True):
                kw = dict(transform=tr, exp_scale=1.0, exp_divisor=50.0, apply_inverse=inv)
                with _lib.debug_override(profiles_variant=1):
                    gx, gy = nm.attention_axis_maps(a_dev, nw, nh, **kw)
                gx, gy = N(gx), N(gy)
                mx, my = nm.attention_axis_maps(a_dev, nw, nh, **kw)                  # the product library
                assert same(mx, gx, nan=True) and same(my, gy, nan=True), (label, nw, nh, tr, inv)
                for v in variants:
                    with _lib.debug_override(profiles_variant=v):
                        vx, vy = nm.attention_axis_maps(a_dev, nw, nh, **kw)
                    assert same(vx, gx, nan=True) and same(vy, gy, nan=True), (label, nw, nh, tr, inv, v)
                if tr in ("identity", "square"):
                    for b in range(a_np.shape[0]):
                        rx, ry = O.maps_from_attention(a_np[b], nw, nh, tr, 1.0, 50.0, inv)
                        assert same(gx[b], rx) and same(gy[b], ry), (label, nw, nh, tr, inv, b)


@pytest.mark.parametrize("dtype", ["uint8", "float32", "float64"])
@pytest.mark.parametrize("hw", C.ATT_HW)
def test_attention_axis_maps_at_limits(dev, hw, dtype):
    """Rows and columns of 16384 (128 leaves of 128), 16383 and 16381 (129 leaves, the most any accepted length makes, one
    of them no multiple of 4), 8200 and 12296 (leaves of 64 / 96 .. 104) against 3 .. 8 elements on the other axis."""
    h, w = hw
    a = C.attention(h, w, dtype)
    _check_attention_maps(dev, T(a, dev), a, variants=(-1, 2) if dtype == "float32" else (-1,), label=(hw, dtype))


@pytest.mark.parametrize("hw", C.ATT_HW)
def test_attention_axis_maps_unaligned_views(dev, hw):
    """A uint8 view one byte into its allocation (with w % 4 != 0 in two of the shapes: the unaligned form of the uint8
    block) and a float32 view one element in (a base that is not 16-byte aligned: the generic kernel serves it) give the
    maps of the aligned tensors."""
    from attwarp_amd import new_method as nm
    h, w = hw
    for dtype in ("uint8", "float32"):
        a = C.attention(h, w, dtype)
        buf = torch.zeros(1 + a.size, device=dev, dtype=TORCH_DT[dtype])
        view = buf[1:].view(2, h, w)
        view.copy_(T(a, dev))
        assert view.is_contiguous() and view.data_ptr() % (4 if dtype == "uint8" else 16) != 0
        for tr in ("identity", "sqrt"):
            for inv in (False, True):
                mx, my = nm.attention_axis_maps(view, 500, 400, tr, apply_inverse=inv)
                ax, ay = nm.attention_axis_maps(T(a, dev), 500, 400, tr, apply_inverse=inv)
                assert torch.equal(mx, ax) and torch.equal(my, ay), (hw, dtype, tr, inv)
                if tr == "identity":
                    for b in range(2):
                        rx, ry = O.maps_from_attention(a[b], 500, 400, tr, 1.0, 1.0, inv)
                        assert same(mx[b], rx) and same(my[b], ry), (hw, dtype, inv, b)


@pytest.mark.parametrize("hw", C.ATT_HW)
def test_gt_marginals_at_limits(dev, hw):
    """marginals_finalize_kernel with up to 128 KiB of LDS; a NaN and an inf planted; the fast float32 kernel and the generic
    one against the oracle."""
    from attwarp_amd import checkpoint_utils as cu
    A = C.marginal_maps(*hw)
    with np.errstate(invalid="ignore"):
        pxo, pyo = O.gt_marginals(A)
    px, py = cu.gt_marginals(T(A, dev))
    with _lib.debug_override(profiles_variant=1):
        qx, qy = cu.gt_marginals(T(A, dev))
    assert same(px, pxo, nan=True) and same(py, pyo, nan=True)
    assert same(qx, pxo, nan=True) and same(qy, pyo, nan=True)
    assert np.isfinite(pxo[0]).all() and np.isfinite(pyo[0]).all()


@pytest.mark.parametrize("W", C.POOL_W)
def test_adaptive_avg_pool_at_limits(dev, W):
    from attwarp_amd import pipeline
    A = C.pool_maps(W)
    for out in ((24, 24), (1, 1)):
        got = pipeline.adaptive_avg_pool2d(T(A, dev), out)
        assert same(got, O.adaptive_avg_pool24(A, out)), out


# ================================ 3. fused kernels ================================
@pytest.mark.parametrize("HW", [(8192, 8192 // 2), (8191, 8192)])
@pytest.mark.parametrize("Lo", [64, 1])
def test_axis_maps_from_pdf_at_limits(dev, Lo, HW):
    from attwarp_amd import pipeline
    H, W = HW
    px, py = C.low_res_pdfs(Lo)
    mx, my = pipeline.axis_maps_from_pdf(T(px, dev), T(py, dev), (H, W))
    rx, ry = C.pdf_chain(px, py, H, W)
    assert same(mx, rx) and same(my, ry)


def _bf16_round(x):
    """float64 / float32 -> the nearest bfloat16 (ties to even), as float32: ONE rounding, as from_f64<__hip_bfloat16>."""
    x = np.asarray(x, np.float64)
    f = x.astype(F32)
    lo = (f.view(np.uint32) & np.uint32(0xFFFF0000))
    lo = np.where(lo.view(F32).astype(np.float64) > x, lo - np.uint32(0x10000), lo).astype(np.uint32)   # f rounded up past a bfloat16
    hi = lo + np.uint32(0x10000)
    lo_f, hi_f = lo.view(F32).astype(np.float64), hi.view(F32).astype(np.float64)      # positive inputs: lo <= x < hi
    assert (x >= 0).all() and (lo_f <= x).all() and (x < hi_f).all()
    dl, dh = x - lo_f, hi_f - x
    up = (dh < dl) | ((dh == dl) & ((lo >> np.uint32(16)) & np.uint32(1)).astype(bool))
    return np.where(up, hi, lo).astype(np.uint32).view(F32)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("g,HW", [(64, (8192, 64)), (64, (64, 8191)), (1, (8192, 8191))])
def test_axis_maps_from_attention_steps_at_limits(dev, g, HW, dt):
    """A 64 x 64 grid (4096 tokens: the strided copy of the inverse matrix, 147 KB of LDS) and a 1 x 1 grid at axes of 8192
    and 8191, in every step dtype.  bfloat16 has no numpy type: the mean over steps is restated here (float64 sum, one
    rounding, a float32 division rounded once more) and checked on the attention map the kernel returns."""
    from attwarp_amd import pipeline
    H, W = HW
    s = T(C.step_maps(g), dev).to(dt)
    mx, my, att = pipeline.axis_maps_from_attention_steps(s, (H, W), return_attention=True)
    if dt == torch.bfloat16:
        sf = N(s.float())
        acc = _bf16_round(sf.astype(np.float64).sum(axis=0))
        mean = _bf16_round((acc / F32(sf.shape[0])).astype(F32))
        qx, qy = O.gt_marginals(mean.reshape(-1, 1, g, g))
        rx, ry = C.pdf_chain(qx, qy, H, W)
    else:
        sn = N(s)
        mean = O.attn_finalize([t for t in sn]).astype(F32)
        rx, ry = C.steps_chain(sn, g, H, W)
    assert same(att, mean)
    assert same(mx, rx) and same(my, ry)


@pytest.mark.parametrize("adt", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("HW", [(8192, 8191), (100, 8192)])
def test_attn_reduce_and_maps_at_limits(dev, HW, adt):
    """The largest grid attwarp_attn_reduce_and_maps takes (g = 26: 676 tokens) at max(W, H) = 8192: the reduce of one batch
    and the maps of another in one launch == attn_reduce_step + axis_maps_from_attention_steps, bit for bit; the float32
    maps also equal the oracle chain."""
    from attwarp_amd import pipeline, _tables, attention_extraction as ae
    H, W = HW
    g, ntok = C.AM_MAX_G, C.AM_MAX_G ** 2
    gen = torch.Generator(device=dev).manual_seed(26)
    Tn, B, heads, kv = 3, 2, 5, ntok + 9
    rows = torch.softmax(torch.randn((Tn, B, heads, kv), device=dev, generator=gen) * 2, dim=-1).to(adt)
    starts = torch.tensor([3, 9], device=dev, dtype=torch.int32).repeat(Tn)
    steps_in = T(C.step_maps(g), dev).to(adt)
    steps_out = torch.full((Tn, B, ntok), -1, device=dev, dtype=adt)
    mx = torch.full((B, W), -1, device=dev, dtype=torch.float32)
    my = torch.full((B, H), -1, device=dev, dtype=torch.float32)
    inv_x, inv_y = _tables.right_inverse_inv(g, W, 1e-8, dev), _tables.right_inverse_inv(g, H, 1e-8, dev)
    with torch.cuda.device(dev):
        _lib.call("attwarp_attn_reduce_and_maps", _lib.dtype_id(rows), _lib.ptr(rows), Tn * B, heads, kv, _lib.ptr(starts),
                  Tn * B, ntok, _lib.ptr(steps_out), _lib.ptr(steps_in), Tn, B, g, W, H, W, H, _lib.ptr(inv_x),
                  _lib.ptr(inv_y), _lib.ptr(mx), _lib.ptr(my), _lib.stream_ptr(dev))
    want_steps = ae.attn_reduce_step(rows.view(Tn * B, heads, 1, kv), starts, ntok).view(Tn, B, ntok)
    wx, wy = pipeline.axis_maps_from_attention_steps(steps_in, (H, W))
    assert torch.equal(steps_out, want_steps) and torch.equal(mx, wx) and torch.equal(my, wy)
    if adt == torch.float32:
        rx, ry = C.steps_chain(C.step_maps(g), g, H, W)
        assert same(mx, rx) and same(my, ry)


def test_attn_reduce_and_maps_refusals(dev):
    from attwarp_amd import _tables
    z = torch.zeros(2 * 2 * 1100, device=dev)
    zi = torch.zeros(4, device=dev, dtype=torch.int32)
    inv = _tables.right_inverse_inv(26, 128, 1e-8, dev)

    def am(ntok, g, W, H, B=2, kv=1100):
        with torch.cuda.device(dev):
            _lib.call("attwarp_attn_reduce_and_maps", _lib.dtype_id(z), _lib.ptr(z), 1, 1, kv, _lib.ptr(zi), 1, ntok,
                      _lib.ptr(z), _lib.ptr(z[2200:]), 1, B, g, W, H, 8, 8, _lib.ptr(inv), _lib.ptr(inv), _lib.ptr(z),
                      _lib.ptr(z), _lib.stream_ptr(dev))

    with pytest.raises(AttWarpError, match=r"attn_reduce_and_maps: ntok must equal g\*g, be a multiple of 4 and <= 768"):
        am(33 * 33, 33, 128, 128)
    with pytest.raises(AttWarpError, match=r"attn_reduce_and_maps: ntok must equal g\*g, be a multiple of 4 and <= 768"):
        am(772, 26, 128, 128)
    with pytest.raises(AttWarpError, match=r"attn_reduce_and_maps: ntok must equal g\*g, be a multiple of 4 and <= 768"):
        am(28 * 28, 28, 128, 128)
    for W, H in ((C.FUSED_MAX_L + 1, 128), (128, C.FUSED_MAX_L + 1)):
        with pytest.raises(AttWarpError, match=r"attn_reduce_and_maps: g > 32, max\(W,H\) > 8192 or B > 65535"):
            am(676, 26, W, H)
    with pytest.raises(AttWarpError, match=r"attn_reduce_and_maps: g > 32, max\(W,H\) > 8192 or B > 65535"):
        am(676, 26, 128, 128, B=C.MAX_B + 1)


# ================================ 4. the batch edge ================================
@pytest.fixture(scope="module")
def batch(dev):
    """65535 images of 8 x 8: five distinct ones tiled, a sixth in the last place; (index of each image's source, the six)."""
    src = C.batch_sources()
    return src, T(src, dev), C.six_maps()


def test_attention_axis_maps_full_batch(dev, batch):
    from attwarp_amd import new_method as nm
    src, dsrc, six = batch
    for name, imgs in (("uint8", (six * 255).astype(np.uint8)), ("float32", six), ("float64", six.astype(np.float64))):
        mx, my = nm.attention_axis_maps(T(imgs, dev)[dsrc], 12, 9, "square")
        ref = [O.maps_from_attention(a, 12, 9, "square") for a in imgs]
        rx, ry = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
        assert len({r.tobytes() for r in rx}) == 6
        assert same(mx, rx[src]) and same(my, ry[src]), name


def test_gt_marginals_full_batch(dev, batch):
    from attwarp_amd import checkpoint_utils as cu
    src, dsrc, six = batch
    px, py = cu.gt_marginals(T(six[:, None], dev)[dsrc])
    rx, ry = O.gt_marginals(six[:, None])
    assert same(px, rx[src]) and same(py, ry[src])


def test_axis_maps_from_attention_steps_full_batch(dev, batch):
    from attwarp_amd import pipeline
    src, dsrc, _ = batch
    s = C.six_step_maps()
    mx, my = pipeline.axis_maps_from_attention_steps(T(s, dev)[:, dsrc].contiguous(), (8, 8))
    rx, ry = C.steps_chain(s, 2, 8, 8)
    assert len({r.tobytes() for r in rx}) == 6
    assert same(mx, rx[src]) and same(my, ry[src])


def test_adaptive_avg_pool_full_batch(dev, batch):
    from attwarp_amd import pipeline
    src, dsrc, six = batch
    got = pipeline.adaptive_avg_pool2d(T(six[:, None], dev)[dsrc], (3, 2))
    assert same(got, O.adaptive_avg_pool24(six[:, None], (3, 2))[src])
