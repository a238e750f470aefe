"""Shape sweep of the training kernels (losses.hip, loss_blocks.hpp, the target builders of profiles.hip, pdf_l1 on the
right-inverse block) against tests/losses_ref.py, the float64 restatement that tests/test_losses_ref_cpu.py pins to the
reference's own values.  The expected values are computed at run time from the same float32 inputs.

Bounds, as tests/test_losses_gpu.py states them: loss scalars 1e-5 relative, target vectors 2e-6 absolute, gradients
||g - g_ref||_inf <= 1e-4 ||g_ref||_inf + 1e-9.

The cases are the structural edges of the kernels, not a random cloud: one element more or less than a wave (64), a
workgroup (256), the scan's elements per thread (N / 256 rounded up), the row limit (4096), the default LDS grant
(3 N doubles pass 64 KB at N = 2731), the in-launch reduction's 256-thread strided sum of its partials (B, or 2 B for
pdf_l1), the grid cap of the element-wise kernels (4096 x 256 threads), the 4-wide loads of the pooling kernels.

Sign margin: the L1 losses have sign discontinuities, so every L1 case is drawn again, from the next draw of its own
seeded generator, until the float64 restatement shows no compared difference within 1e-6 (in units of a uniform density)
of zero -- the fixture generator's rule (losses_ref.l1_margin_ok), at most 500 draws.  Only the restatement takes part,
so tests/test_losses_ref_cpu.py::test_every_sweep_case_finds_its_draw checks every case without a GPU.  No case skips.

What the sweep is there to catch, by example (none of these is in the code):
* finish_loss summing its partials in one pass of 256 threads and not a strided loop: test_row_losses[257-24] and
  [1000-24], test_recon_losses[300-24-24-False], test_pdf_l1_loss[129-...] and [300-...] (2 B partials) lose the partials
  past 256, a share (B - 256) / B of the loss, against a bound of 1e-5.  B = 256 and pdf_l1's B = 128 are the last that fit.
* block_inclusive_scan rounding its elements per thread down: every row length that 256 does not divide leaves its last
  n mod 256 entries unscanned (all of them below 256), so test_row_losses at n = 63, 65, 255, 257, 1023, 2730, 2731, 4095
  gets raw densities where CDF entries belong (l1_cdf and its backward, cdf_downsample at L = 24): errors of order 1.
* right_inverse_block visiting three windows only: test_pdf_l1_loss with an axis shorter than its low resolution
  ([2-64-64-8192-37]: output 1 of 37 lies in windows 1, 2, 3 of 64 and the loop would stop at 2) drops whole terms of a
  row; so do test_gpu_parity.py::test_right_inverse_shorter_than_low_resolution and, without a GPU,
  test_oracle_properties.py::test_right_inverse_window_loop_covers_every_window.
"""
import numpy as np
import pytest
import torch

import losses_ref as R

pytestmark = pytest.mark.gpu


# ---- the cases (plain data and CPU-only builders: importable without a GPU) --------------------------------------------
ROW_CASES = [(3, n) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 2730, 2731, 4095, 4096)] + \
            [(b, 24) for b in (1, 255, 256, 257, 1000)]
DOWNSAMPLE_CASES = [(4096, 4096), (4096, 1), (1, 4096), (37, 256)]
RECON_CASES = [(2, 1, 1, False), (2, 1, 4096, False), (2, 4096, 1, False), (2, 5, 63, False), (2, 5, 65, False),
               (2, 1025, 3, False), (2, 24, 24, False), (300, 24, 24, False), (3, 5, 65, True)]
PDF_LOW = [(24, 24), (1, 64), (7, 9), (63, 8), (64, 64)]
PDF_CASES = [(2, lx, ly, w, h) for lx, ly in PDF_LOW
             for w, h in ((lx, ly), (lx + 1, 2 * ly - 1), (336, 512), (8192, 37), (37, 8192))] + \
            [(b, 24, 24, 96, 96) for b in (128, 129, 300)]
# (H, W, L, base offset in floats): every H or W of 1, 3, 4, 5, 8191, 8192, 8193, 16384, L of 1, 24, 4096; the 4-wide
# loads need W % 4 == 0 and a 16-byte-aligned base, so W % 4 == 0 comes with and without an offset of one float
TARGET_CASES = [(1, 16384, 24, 0), (16384, 1, 1, 0), (3, 8191, 24, 0), (8193, 4, 24, 0), (5, 8192, 4096, 1), (8192, 5, 1, 0),
                (4, 8193, 4096, 0), (8, 16384, 24, 1), (3, 4, 24, 1), (50, 8192, 24, 0), (58, 50, 4096, 0)]
TRANSFORMS = ["sqrt", "none", "identity", "x", "sqrt"]


def rows_case(B, N):
    """(p, q) with the l1_cdf sign margin; the other row kernels take the same rows.  peak = 1.0, not the generator's
    3.0: at 3.0 most of a long row (and of some row in a large batch) sits at the grid's floor of 2^-16, where the two CDFs
    rise in lockstep and tie to 1e-8 or exactly -- of 60 draws none passed at N >= 2730 or B >= 255.  At 1.0 every case
    passes within a few draws."""
    rng = np.random.default_rng(10_000 + 17 * B + N)
    return R.redraw(lambda: (R.softmax_rows(rng, B, N, 1.0), R.softmax_rows(rng, B, N, 1.0)), R.l1_cdf_margin_ok)


def recon_case(B, H, W, hostile):
    rng = np.random.default_rng(20_000 + 4099 * B + 17 * H + W)

    def draw():
        px, py = R.softmax_rows(rng, B, W), R.softmax_rows(rng, B, H)
        A = R.unit_map(rng, (B, 1, H, W)) + np.float32(1 / 16)
        if hostile:                                           # negative cells, an all-zero map, an all-negative map
            A[0, 0, 1:4, 2:7] = -rng.random((3, 5), dtype=np.float32)
            A[1] = 0.0
            A[2] = -A[2]
        return px, py, A
    return R.redraw(draw, R.recon_margin_ok)


def pdf_eps(Lx, Ly, W, H):
    """The ridge term of a case.  1e-8, the default, where both axes have L >= Lo.  For L < Lo, A A^T has rank L and its
    float32 form loses a ridge of 1e-8, so the package refuses to build that table (LinAlgError, like the reference's own
    float32 solve); such lengths are reached with a ridge that float32 keeps, here 0.5 (well-conditioned: the kernel's
    float32 intermediate then carries no cancellation)."""
    return 1e-8 if W >= Lx and H >= Ly else 0.5


def pdf_tables(Lx, Ly, W, H):
    """The (Lo, Lo) tables the package gives its kernels, numpy float64: the restatement takes the same ones."""
    from attwarp_amd import _tables
    eps = pdf_eps(Lx, Ly, W, H)
    return _tables._right_inverse_inv_host(Lx, W, eps), _tables._right_inverse_inv_host(Ly, H, eps)


def pdf_case(B, Lx, Ly, W, H):
    rng = np.random.default_rng(30_000 + 7919 * B + 131 * Lx + 17 * Ly + W + 3 * H)
    inv_x, inv_y = pdf_tables(Lx, Ly, W, H)
    rows = lambda L: R.softmax_rows(rng, B, L, peak=1.0)
    case = R.redraw(lambda: (rows(Lx), rows(Ly), rows(Lx), rows(Ly)),
                    lambda a, b, c, d: R.pdf_l1_margin_ok(a, b, c, d, W, H, inv_x, inv_y))
    return case + (inv_x, inv_y)


def target_case(H, W):
    rng = np.random.default_rng(40_000 + 17 * H + W)
    return R.hostile_map(rng, len(TRANSFORMS), H, W)


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import os
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from attwarp_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "HIP library missing -- the product has no fallback"
    _lib.load()
    return torch.device("cuda:0")


def T(x, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(grad)


def N(t):
    return t.detach().double().cpu().numpy()


def check_loss(got, ref, what):
    assert got.dtype == torch.float32 and got.dim() == 0, what
    g, r = float(got.detach()), float(ref)
    print(f"{what}: loss {g!r} ref {r!r}")
    assert abs(g - r) <= 1e-5 * abs(r) + 1e-12, (what, g, r)


def check_grad(got, ref, what):
    g = N(got)
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    bound = 1e-4 * np.abs(ref).max() + 1e-9
    err = np.abs(g - ref).max()
    print(f"{what}: grad err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def check_target(got, ref, what):
    g = N(got)
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    err = np.abs(g - ref).max()
    print(f"{what}: target err {err:.3e}")
    assert err <= 2e-6, (what, err)


def ticket_is_zero(dev):
    from attwarp_amd import losses
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    assert key in losses._TICKETS, key
    return int(losses._TICKETS[key].item()) == 0


def run_loss(dev, fn, ref_fn, arrays, grad_of, what, upstream=1.0, **kw):
    """fn on the GPU and ref_fn in float64 on the same float32 arrays; loss, the ticket and the gradients of the inputs
    ``grad_of`` for the upstream gradient ``upstream``."""
    xs = [T(a, dev, i in grad_of) for i, a in enumerate(arrays)]
    loss = fn(*xs, **kw)
    assert ticket_is_zero(dev), what
    rs = [R.t64(a, i in grad_of) for i, a in enumerate(arrays)]
    ref = ref_fn(*rs, **kw)
    check_loss(loss, ref.detach(), what)
    if grad_of:
        (loss * upstream).backward()
        for i, g in zip(grad_of, R.grads(ref, [rs[i] for i in grad_of], upstream)):
            check_grad(xs[i].grad, g, f"{what} input {i}")
    return loss


# ---- row kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", ROW_CASES)
def test_row_losses(dev, B, n):
    from attwarp_amd import losses, model
    p, q = rows_case(B, n)
    run_loss(dev, losses.l1_cdf_loss, R.l1_cdf_loss, (p, q), (0, 1), f"l1_cdf b{B} n{n}")
    run_loss(dev, losses.sym_kl, R.sym_kl, (p, q), (0, 1), f"sym_kl b{B} n{n}")
    run_loss(dev, model.entropy, R.entropy, (p,), (0,), f"entropy b{B} n{n}")
    for L in sorted({24, n}):
        Fp = losses.cdf_from_density_downsample(T(p, dev), L)
        check_target(Fp, R.cdf_from_density_downsample(R.t64(p), L).numpy(), f"cdf_downsample b{B} n{n} L{L}")
        assert (Fp[:, -1] == 1).all()


@pytest.mark.parametrize("n,L", DOWNSAMPLE_CASES)
def test_cdf_downsample_extremes(dev, n, L):
    from attwarp_amd import losses
    p = R.softmax_rows(np.random.default_rng(50_000 + n + L), 3, n)
    p[1, n // 2] = np.nan                                     # counts as 0
    if n > 1:
        p[1, 0], p[2] = np.inf, 0.0                           # inf counts as 0; an all-zero row
    Fp = losses.cdf_from_density_downsample(T(p, dev), L)
    check_target(Fp, R.cdf_from_density_downsample(R.t64(p), L).numpy(), f"cdf_downsample n{n} L{L}")


def test_row_longer_than_the_limit_raises_and_the_stream_stays_good(dev):
    from attwarp_amd import _lib, losses, model
    p = T(R.softmax_rows(np.random.default_rng(1), 3, 4097), dev, True)
    for fn in (lambda: losses.l1_cdf_loss(p, p), lambda: losses.sym_kl(p, p), lambda: model.entropy(p),
               lambda: losses.cdf_from_density_downsample(p.detach(), 24),
               lambda: losses.cdf_from_density_downsample(p.detach()[:, :24], 4097),
               lambda: losses.recon_l1(p, p[:, :5], torch.ones(3, 1, 5, 4097, device=dev))):
        with pytest.raises(_lib.AttWarpError):
            fn()
    a, b = rows_case(3, 4096)
    run_loss(dev, losses.l1_cdf_loss, R.l1_cdf_loss, (a, b), (0, 1), "l1_cdf after a refused call")
    run_loss(dev, losses.sym_kl, R.sym_kl, (a, b), (0, 1), "sym_kl after a refused call")


# ---- element-wise kernels past their grid cap of 4096 x 256 threads -----------------------------------------------------
def test_second_grid_stride_trip(dev):
    from attwarp_amd import _lib, model
    B, n = 1025, 1024                                         # 1025 x 1024 = 4096 x 256 + 1024 elements
    rng = np.random.default_rng(60_000)
    p = R.softmax_rows(rng, B, n, peak=6.0)
    run_loss(dev, model.entropy, R.entropy, (p,), (0,), "entropy 1025x1024", upstream=-2.5)
    w = rng.standard_normal((B, n)).astype(np.float32)
    x = T(p, dev, True)
    out = model.mix_with_uniform(x, 0.3)
    r = R.t64(p, True)
    ref = R.mix_with_uniform(r, 0.3)
    check_target(out, ref.detach().numpy(), "mix_with_uniform 1025x1024")
    (out * T(w, dev)).sum().backward()
    check_grad(x.grad, R.grads((ref * R.t64(w)).sum(), (r,))[0], "mix_with_uniform 1025x1024")
    # one element past the cap, flat, through the ABI: c1 * p + c2 in float32 with one rounding per operation, bit for bit
    m = 4096 * 256 + 1
    flat = rng.random(m, dtype=np.float32)
    c1, c2 = np.float32(0.7), np.float32(0.3 / 24)
    src, dst = T(flat, dev), torch.full((m + 1,), -7.0, device=dev)
    with torch.cuda.device(dev):
        _lib.call("attwarp_scale_shift", _lib.ptr(src), m, float(c1), float(c2), _lib.ptr(dst), _lib.stream_ptr(dev))
    got = dst.cpu().numpy()
    assert np.array_equal(got[:m], (c1 * flat).astype(np.float32) + c2)
    assert got[m] == -7.0                                     # nothing written past n


# ---- recon, both kinds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,hostile", RECON_CASES)
def test_recon_losses(dev, B, H, W, hostile):
    from attwarp_amd import losses
    px, py, A = recon_case(B, H, W, hostile)
    tag = f"{'hostile ' if hostile else ''}b{B} h{H} w{W}"
    run_loss(dev, losses.separable_recon_loss, R.separable_recon_loss, (px, py, A), (0, 1), "recon_mse " + tag)
    run_loss(dev, losses.recon_l1, R.recon_l1, (px, py, A), (0, 1), "recon_l1 " + tag)


# ---- pdf_l1_loss ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Lx,Ly,W,H", PDF_CASES)
def test_pdf_l1_loss(dev, B, Lx, Ly, W, H):
    from attwarp_amd import losses
    px, py, gx, gy, inv_x, inv_y = pdf_case(B, Lx, Ly, W, H)
    eps = pdf_eps(Lx, Ly, W, H)
    what = f"pdf_l1 b{B} lx{Lx} ly{Ly} w{W} h{H} eps{eps}"
    if eps != 1e-8:                                           # never a silent row: the default ridge builds no table for L < Lo
        with pytest.raises(np.linalg.LinAlgError):
            losses.pdf_l1_loss(T(px, dev), T(py, dev), T(gx, dev), T(gy, dev), W, H)
    run_loss(dev, lambda a, b, c, d: losses.pdf_l1_loss(a, b, c, d, W, H, eps),
             lambda a, b, c, d: R.pdf_l1_loss(a, b, c, d, W, H, inv_x, inv_y), (px, py, gx, gy), (0, 1), what)


def test_pdf_l1_axis_longer_than_the_limit_raises(dev):
    from attwarp_amd import _lib, losses
    p = T(R.softmax_rows(np.random.default_rng(2), 2, 24), dev)
    for W, H in ((8193, 96), (96, 8193)):
        with pytest.raises(_lib.AttWarpError):
            losses.pdf_l1_loss(p, p, p, p, W, H)
    px, py, gx, gy, inv_x, inv_y = pdf_case(2, 24, 24, 336, 512)
    run_loss(dev, lambda a, b, c, d: losses.pdf_l1_loss(a, b, c, d, 336, 512),
             lambda a, b, c, d: R.pdf_l1_loss(a, b, c, d, 336, 512, inv_x, inv_y), (px, py, gx, gy), (0, 1),
             "pdf_l1 after a refused call")


# ---- target builders ------------------------------------------------------------------------------------------------------
def offset_tensor(A, off, dev):
    """A on the device with its first element ``off`` floats past a 16-byte boundary (contiguous: the wrappers keep it)."""
    buf = torch.empty(A.size + 4, device=dev, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + A.size].view(*A.shape)
    t.copy_(torch.from_numpy(A))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * off
    return t


@pytest.mark.parametrize("H,W,L,off", TARGET_CASES)
def test_target_builders(dev, H, W, L, off):
    from attwarp_amd import losses, pipeline
    A = target_case(H, W)
    x = offset_tensor(A, off, dev)
    tag = f"h{H} w{W} L{L} off{off}"
    Fx, Fy = losses.build_axis_cdf_targets(x, L=L)
    rFx, rFy = R.build_axis_cdf_targets(R.t64(A), L)
    check_target(Fx, rFx.numpy(), "build_axis_cdf_targets Fx " + tag)
    check_target(Fy, rFy.numpy(), "build_axis_cdf_targets Fy " + tag)
    assert (Fx[:, -1] == 1).all() and (Fy[:, -1] == 1).all()
    # every transform mode in one batch; 24 does not divide H or W evenly (and exceeds the short ones)
    Ap, pxg, pyg = pipeline.trainer_attention_targets(x, TRANSFORMS)
    rA, rpx, rpy = R.trainer_attention_targets(R.t64(A), TRANSFORMS)
    check_target(Ap, rA.numpy(), "trainer_attention_targets A " + tag)
    check_target(pxg, rpx.numpy(), "trainer_attention_targets px " + tag)
    check_target(pyg, rpy.numpy(), "trainer_attention_targets py " + tag)
    # the plain pool kernel on the stock-op transform gives the same pooled map bit for bit, and gt_marginals of a clean map
    # its float64 marginals: both keep a whole row of doubles in LDS, 128 KB at 16384
    m = torch.tensor([1.0 if t == "sqrt" else 0.0 for t in TRANSFORMS], device=dev).view(-1, 1, 1, 1)
    pos = x.clamp_min(0.0)
    assert torch.equal(Ap, pipeline.adaptive_avg_pool2d(pos.sqrt() * m + pos * (1.0 - m), (24, 24), sanitize=True)), tag
    from attwarp_amd import checkpoint_utils as cu
    clean = R.unit_map(np.random.default_rng(H + W), A.shape)
    gpx, gpy = cu.gt_marginals(offset_tensor(clean, off, dev))
    rgx, rgy = R.gt_marginals(R.t64(clean))
    check_target(gpx, rgx.numpy(), "gt_marginals px " + tag)
    check_target(gpy, rgy.numpy(), "gt_marginals py " + tag)
    if off:                                                   # the pool's dword loads and 4-wide loads add in one order
        y = offset_tensor(A, 0, dev)
        assert all(torch.equal(a, b) for a, b in zip(pipeline.trainer_attention_targets(y, TRANSFORMS), (Ap, pxg, pyg)))


def test_target_builder_sizes_past_the_limits_raise(dev):
    from attwarp_amd import _lib, losses, pipeline
    for H, W, L in ((4, 16385, 24), (16385, 4, 24), (4, 64, 4097), (4, 16384, 4096)):     # the last: 160 KB of rows + `red`
        with pytest.raises(_lib.AttWarpError):
            losses.build_axis_cdf_targets(torch.ones(1, 1, H, W, device=dev), L=L)
    with pytest.raises(_lib.AttWarpError):
        pipeline.trainer_attention_targets(torch.ones(1, 1, 4, 16385, device=dev), ["sqrt"])
    test_target_builders(dev, 3, 4, 24, 1)


# ---- upstream gradients -------------------------------------------------------------------------------------------------
def loss_table(dev):
    """name -> (GPU function, restatement, float32 arrays, indices with gradients): one small case per loss."""
    from attwarp_amd import losses, model
    p, q = rows_case(5, 37)
    px, py, A = recon_case(3, 12, 37, False)
    sx, sy, gx, gy, inv_x, inv_y = pdf_case(3, 24, 24, 336, 100)
    return {
        "l1_cdf": (losses.l1_cdf_loss, R.l1_cdf_loss, (p, q), (0, 1)),
        "sym_kl": (losses.sym_kl, R.sym_kl, (p, q), (0, 1)),
        "entropy": (model.entropy, R.entropy, (p,), (0,)),
        "recon_mse": (losses.separable_recon_loss, R.separable_recon_loss, (px, py, A), (0, 1)),
        "recon_l1": (losses.recon_l1, R.recon_l1, (px, py, A), (0, 1)),
        "pdf_l1": (lambda a, b, c, d: losses.pdf_l1_loss(a, b, c, d, 336, 100),
                   lambda a, b, c, d: R.pdf_l1_loss(a, b, c, d, 336, 100, inv_x, inv_y), (sx, sy, gx, gy), (0, 1)),
    }


LOSS_NAMES = ["l1_cdf", "sym_kl", "entropy", "recon_mse", "recon_l1", "pdf_l1"]


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_upstream_gradients(dev, name):
    fn, ref_fn, arrays, grad_of = loss_table(dev)[name]
    run_loss(dev, fn, ref_fn, arrays, grad_of, name + " x -2.5", upstream=-2.5)
    # x 0.0: every gradient is exactly zero (also where the reference's is -0.0)
    xs = [T(a, dev, i in grad_of) for i, a in enumerate(arrays)]
    (fn(*xs) * 0.0).backward()
    for i in grad_of:
        assert xs[i].grad is not None and not xs[i].grad.any(), (name, i)
    # a 0-d upstream gradient that is a view into a larger buffer (storage offset, not the loss's own dtype)
    rs = [R.t64(a, i in grad_of) for i, a in enumerate(arrays)]
    want = R.grads(ref_fn(*rs), [rs[i] for i in grad_of], 0.375)
    for g in (torch.tensor([9.0, 0.375, 9.0], device=dev)[1], torch.tensor([9.0, 0.375], device=dev, dtype=torch.float16)[1],
              torch.tensor([[9.0, 0.375]], device=dev).t()[1, 0]):
        xs = [T(a, dev, i in grad_of) for i, a in enumerate(arrays)]
        fn(*xs).backward(gradient=g)
        for i, w in zip(grad_of, want):
            check_grad(xs[i].grad, w, f"{name} upstream view {g.dtype} input {i}")


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_upstream_gradient_under_autocast(dev, name):
    """Inside torch.autocast(float16) the loss stays float32 and is scaled by a half-precision 0-d tensor before backward."""
    fn, ref_fn, arrays, grad_of = loss_table(dev)[name]
    scale = torch.tensor(-2.5, device=dev, dtype=torch.float16)
    xs = [T(a, dev, i in grad_of) for i, a in enumerate(arrays)]
    with torch.autocast("cuda", dtype=torch.float16):
        loss = fn(*xs)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        (loss * scale).backward()
    rs = [R.t64(a, i in grad_of) for i, a in enumerate(arrays)]
    ref = ref_fn(*rs)
    check_loss(loss, ref.detach(), name + " autocast")
    for i, w in zip(grad_of, R.grads(ref, [rs[i] for i in grad_of], -2.5)):
        assert xs[i].grad.dtype == torch.float32
        check_grad(xs[i].grad, w, f"{name} autocast input {i}")


# ---- input layout: the wrappers make every input contiguous float32 ---------------------------------------------------
@pytest.mark.parametrize("name", LOSS_NAMES)
def test_strided_inputs_equal_contiguous_copies(dev, name):
    fn, _, arrays, grad_of = loss_table(dev)[name]

    def run(xs):
        xs = [x.requires_grad_(i in grad_of) for i, x in enumerate(xs)]
        loss = fn(*xs)
        loss.backward()
        return [loss.detach()] + [xs[i].grad for i in grad_of]
    base = run([T(a, dev) for a in arrays])
    variants = []
    for a in arrays:
        t = T(a, dev)
        if a.ndim == 2:                                       # a transposed view and every second column of a wider tensor
            wide = torch.zeros(a.shape[0], 2 * a.shape[1], device=dev)
            wide[:, ::2] = t
            variants.append((t.t().contiguous().t(), wide[:, ::2]))
        else:                                                 # a (B,H,W) map and channel 1 of a (B,3,H,W) tensor
            three = torch.rand(a.shape[0], 3, *a.shape[2:], device=dev)
            three[:, 1] = t[:, 0]
            variants.append((t[:, 0], three[:, 1:2]))
    for k in range(2):
        xs = [v[k].detach() for v in variants]
        assert any(not x.is_contiguous() or x.dim() == 3 for x in xs)
        got = run(xs)
        for a, b in zip(base, got):
            assert a.shape == b.shape and torch.equal(a, b), (name, k)


def test_strided_inputs_of_the_builders(dev):
    from attwarp_amd import losses, model, pipeline
    A = target_case(50, 58)
    t = T(A, dev)
    three = torch.rand(A.shape[0], 3, 50, 58, device=dev)
    three[:, 1] = t[:, 0]
    for x in (t[:, 0], three[:, 1:2]):
        for a, b in zip(losses.build_axis_cdf_targets(x, L=24), losses.build_axis_cdf_targets(t, L=24)):
            assert torch.equal(a, b)
    for a, b in zip(pipeline.trainer_attention_targets(three[:, 1:2], TRANSFORMS), pipeline.trainer_attention_targets(t, TRANSFORMS)):
        assert torch.equal(a, b)
    p = T(rows_case(5, 37)[0], dev)
    wide = torch.zeros(5, 74, device=dev)
    wide[:, ::2] = p
    for x in (p.t().contiguous().t(), wide[:, ::2]):
        assert not x.is_contiguous()
        assert torch.equal(losses.cdf_from_density_downsample(x, 24), losses.cdf_from_density_downsample(p, 24))
        assert torch.equal(model.mix_with_uniform(x, 0.3), model.mix_with_uniform(p, 0.3))


# ---- the ticket ---------------------------------------------------------------------------------------------------------
def test_ticket_across_batch_sizes_and_streams(dev):
    """One partial, then more partials than the 256 threads that sum them, then one again, on one ticket: each call is
    right and repeats bit for bit; the same on a second stream, which has a ticket of its own."""
    from attwarp_amd import losses, model
    cases = {B: rows_case(B, 24) for B in (1, 1000)}
    pdf = {B: pdf_case(B, 24, 24, 96, 96) for B in (1, 300)}
    want = {}

    def sequence(tag):
        for rep in range(2):
            for B in (1, 1000, 1):
                p, q = cases[B]
                for name, fn, ref_fn, arrs in (("l1_cdf", losses.l1_cdf_loss, R.l1_cdf_loss, (p, q)),
                                               ("sym_kl", losses.sym_kl, R.sym_kl, (p, q)),
                                               ("entropy", model.entropy, R.entropy, (p,))):
                    loss = run_loss(dev, fn, ref_fn, arrs, (), f"{tag} {name} b{B}")
                    assert torch.equal(want.setdefault((name, B), loss.clone()), loss), (tag, name, B, rep)
            for B in (1, 300, 1):
                px, py, gx, gy, inv_x, inv_y = pdf[B]
                loss = run_loss(dev, lambda a, b, c, d: losses.pdf_l1_loss(a, b, c, d, 96, 96),
                                lambda a, b, c, d: R.pdf_l1_loss(a, b, c, d, 96, 96, inv_x, inv_y), (px, py, gx, gy), (),
                                f"{tag} pdf_l1 b{B}")
                assert torch.equal(want.setdefault(("pdf_l1", B), loss.clone()), loss), (tag, B, rep)
    sequence("default stream")
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        sequence("second stream")
        side.synchronize()
    assert len({k for k in losses._TICKETS if k[0] == dev.index}) >= 2
    assert all(int(t.item()) == 0 for t in losses._TICKETS.values())
