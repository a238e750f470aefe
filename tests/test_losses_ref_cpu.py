"""Pins tests/losses_ref.py, the float64 restatement the GPU sweep and the fuzzers take their expected values from, to
EVERY case of tests/golden/losses.npz (the reference's own float64 values and CPU-autograd gradients).

Bounds: the stored float64 loss scalars within 1e-12 relative; the stored targets and gradients, which were rounded once
to float32 (at most 6e-8 relative), within 1e-7 of the array's maximum.  No GPU."""
import json

import numpy as np
import pytest
import torch

import losses_ref as R

FUNCTIONS = ["l1_cdf_loss", "sym_kl", "separable_recon_loss", "recon_l1", "build_axis_cdf_targets",
             "cdf_from_density_downsample", "mix_with_uniform", "entropy", "trainer_block"]


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("losses")
    cases = json.loads(str(z["cases"]))
    assert sorted(cases) == sorted(FUNCTIONS), sorted(cases)        # a function added to the fixture must be pinned here

    def get(fn):
        out = [(c, {k.split("__", 2)[2]: z[k] for k in z.files if k.startswith(f"{fn}__{c}__")}) for c in cases[fn]]
        assert out, fn
        return out
    return get


def scalar(got, ref, what):
    g, r = float(got.detach()), float(np.asarray(ref).item())
    assert np.asarray(ref).dtype == np.float64, what
    print(f"{what}: loss {g!r} stored {r!r} rel {abs(g - r) / max(abs(r), 1e-300):.2e}")
    assert abs(g - r) <= 1e-12 * abs(r), (what, g, r)


def array(got, ref, what):
    g = got.detach().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref, np.float64)
    assert g.shape == ref.shape and g.dtype == np.float64, (what, g.shape, ref.shape)
    same_nan = np.isnan(g) == np.isnan(ref)
    assert same_nan.all(), what
    err = np.abs(np.nan_to_num(g - ref)).max()
    bound = 1e-7 * np.abs(np.nan_to_num(ref)).max()
    print(f"{what}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def test_l1_cdf_loss(fx):
    for case, d in fx("l1_cdf_loss"):
        p, q = R.t64(d["p_pred"], True), R.t64(d["p_gt"], True)
        loss = R.l1_cdf_loss(p, q)
        scalar(loss, d["loss"], case)
        gp, gq = R.grads(loss, (p, q))
        array(gp, d["g_p_pred"], case + " g_p_pred")
        array(gq, d["g_p_gt"], case + " g_p_gt")


def test_sym_kl(fx):
    for case, d in fx("sym_kl"):
        p, q = R.t64(d["p"], True), R.t64(d["q"], True)
        loss = R.sym_kl(p, q, eps=float(d["eps"].item()))
        scalar(loss, d["loss"], case)
        gp, gq = R.grads(loss, (p, q))
        array(gp, d["g_p"], case + " g_p")
        array(gq, d["g_q"], case + " g_q")


@pytest.mark.parametrize("fn", ["separable_recon_loss", "recon_l1"])
def test_recon_losses(fx, fn):
    for case, d in fx(fn):
        px, py, A = R.t64(d["px"], True), R.t64(d["py"], True), R.t64(d["A"])
        loss = getattr(R, fn)(px, py, A)
        scalar(loss, d["loss"], case)
        gx, gy = R.grads(loss, (px, py))
        array(gx, d["g_px"], case + " g_px")
        array(gy, d["g_py"], case + " g_py")


def test_target_builders(fx):
    for case, d in fx("build_axis_cdf_targets"):
        Fx, Fy = R.build_axis_cdf_targets(R.t64(d["A"]), L=int(d["L"].item()))
        array(Fx, d["Fx"], case + " Fx")
        array(Fy, d["Fy"], case + " Fy")
    for case, d in fx("cdf_from_density_downsample"):
        array(R.cdf_from_density_downsample(R.t64(d["p"]), int(d["L"].item())), d["F"], case)


def test_mix_with_uniform_and_entropy(fx):
    for case, d in fx("mix_with_uniform"):
        p, alpha = R.t64(d["p"], True), float(d["alpha"].item())
        out = R.mix_with_uniform(p, alpha)
        array(out, d["out"], case)
        (g,) = R.grads((out * R.t64(d["w"])).sum(), (p,))
        array(g, d["g_p"], case + " g_p")
    for case, d in fx("entropy"):
        p = R.t64(d["p"], True)
        loss = R.entropy(p, eps=float(d["eps"].item()))
        scalar(loss, d["loss"], case)
        array(R.grads(loss, (p,))[0], d["g_p"], case + " g_p")


def test_trainer_block(fx):
    for case, d in fx("trainer_block"):
        tfms = [str(t) for t in d["transforms"]]
        H, W = int(d["img_h"].item()), int(d["img_w"].item())
        px, py = R.t64(d["px_s"], True), R.t64(d["py_s"], True)
        inv_x, inv_y = R.right_inverse_table(px.shape[1], W), R.right_inverse_table(py.shape[1], H)
        loss, A, pxg, pyg = R.trainer_block(R.t64(d["A_full"]), px, py, tfms, H, W, inv_x, inv_y)
        scalar(loss, d["loss"], case)
        array(A, d["A"], case + " A")
        array(pxg, d["px_gt"], case + " px_gt")
        array(pyg, d["py_gt"], case + " py_gt")
        gx, gy = R.grads(loss, (px, py))
        array(gx, d["g_px_s"], case + " g_px_s")
        array(gy, d["g_py_s"], case + " g_py_s")
        # the package's device table (Gram matrix rounded to float32) moves the loss by that rounding, far inside the GPU
        # tests' 1e-5: the sweep may use it on both sides
        from attwarp_amd import _tables
        tx, ty = (_tables._right_inverse_inv_host(24, n, 1e-8) for n in (W, H))
        with torch.no_grad():
            alt = float(R.trainer_block(R.t64(d["A_full"]), px, py, tfms, H, W, tx, ty)[0])
        assert abs(alt - float(d["loss"].item())) <= 2e-6 * abs(float(d["loss"].item())), (case, alt)


def test_right_inverse_restates_the_pooling_identity():
    """pool(right_inverse(y)) == y at L >= Lo, and the dense product the parity tests use equals the restatement."""
    g = torch.Generator().manual_seed(3)
    for Lo, L in ((1, 1), (7, 9), (24, 37), (24, 336), (64, 64), (63, 125)):
        y = torch.rand(3, Lo, generator=g, dtype=torch.float64)
        inv = R.right_inverse_table(Lo, L)
        x = R.upsample_pdf_right_inverse(y, L, inv)
        back = torch.nn.functional.adaptive_avg_pool1d(x.unsqueeze(1), Lo).squeeze(1)
        assert (back - y).abs().max() <= 1e-6, (Lo, L)


def test_margin_rule_is_the_generators(fx):
    """Every stored L1 case passes the sign-margin rule as restated here (the generator re-drew until it did)."""
    for case, d in fx("l1_cdf_loss"):
        if case.startswith("b"):
            assert R.l1_cdf_margin_ok(d["p_pred"], d["p_gt"]), case
    for case, d in fx("recon_l1"):
        assert R.recon_margin_ok(d["px"], d["py"], d["A"]), case
    for case, d in fx("trainer_block"):
        H, W = int(d["img_h"].item()), int(d["img_w"].item())
        inv_x, inv_y = R.right_inverse_table(24, W), R.right_inverse_table(24, H)
        tfms = [str(t) for t in d["transforms"]]
        _, pxg, pyg = R.trainer_attention_targets(R.t64(d["A_full"]), tfms)
        assert R.pdf_l1_margin_ok(d["px_s"], d["py_s"], pxg, pyg, W, H, inv_x, inv_y), case


def test_every_sweep_case_finds_its_draw():
    """The GPU sweep redraws every L1 case until the restatement alone shows the sign margin, and skips nothing: every
    parametrised case must find its draw within the generator's 500, here, without a GPU."""
    import test_losses_sweep_gpu as S
    for B, n in S.ROW_CASES:
        p, q = S.rows_case(B, n)
        assert p.shape == q.shape == (B, n) and p.dtype == np.float32
    for B, H, W, hostile in S.RECON_CASES:
        px, py, A = S.recon_case(B, H, W, hostile)
        assert px.shape == (B, W) and py.shape == (B, H) and A.shape == (B, 1, H, W)
    for B, Lx, Ly, W, H in S.PDF_CASES + [(3, 24, 24, 336, 100), (1, 24, 24, 96, 96), (2, 24, 24, 336, 512)]:
        case = S.pdf_case(B, Lx, Ly, W, H)
        assert case[0].shape == (B, Lx) and case[1].shape == (B, Ly)
        assert all(np.isfinite(t).all() for t in case[4:])
        assert R.pdf_l1_well_conditioned(*case[:4], W, H, *case[4:]), (B, Lx, Ly, W, H)     # 1e-5 is attainable from float32 rows
    for name in S.LOSS_NAMES:                                  # the small cases of the gradient, layout and ticket tests
        assert name in S.loss_table(None)
    assert S.rows_case(5, 37) and S.recon_case(3, 12, 37, False)
