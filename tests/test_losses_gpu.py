"""GPU tests of the MarginalNet training losses (attwarp_amd.losses, model.mix_with_uniform / entropy) and the trainer's
loss block (pipeline.trainer_attention_targets, losses.pdf_l1_loss) against tests/golden/losses.npz, the reference's own
values and float64 CPU-autograd gradients (tests/golden/make_golden_losses.py).

Bounds: loss scalars within 1e-5 relative, target vectors within 2e-6 absolute (of the float64 values), gradients
||g - g_ref||_inf <= 1e-4 ||g_ref||_inf + 1e-9."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from attwarp_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "HIP library missing -- the product has no fallback"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("losses")
    cases = json.loads(str(z["cases"]))

    def get(fn):
        return [(c, {k.split("__", 2)[2]: z[k] for k in z.files if k.startswith(f"{fn}__{c}__")}) for c in cases[fn]]
    return get


def T(x, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(grad)


def N(t):
    return t.detach().double().cpu().numpy()


def check_loss(got, ref, what):
    assert got.dtype == torch.float32 and got.dim() == 0, what
    g, r = float(got.detach()), float(np.asarray(ref).item())
    assert abs(g - r) <= 1e-5 * abs(r) + 1e-12, (what, g, r)


def check_grad(got, ref, what):
    g = N(got)
    bound = 1e-4 * np.abs(ref).max() + 1e-9
    err = np.abs(g - ref).max()
    assert err <= bound, (what, err, bound)


def check_target(got, ref, what):
    err = np.abs(N(got) - ref).max()
    assert err <= 2e-6, (what, err)


def test_l1_cdf_loss(dev, fx):
    from attwarp_amd import losses
    for case, d in fx("l1_cdf_loss"):
        p, q = T(d["p_pred"], dev, True), T(d["p_gt"], dev, True)
        loss = losses.l1_cdf_loss(p, q)
        check_loss(loss, d["loss"], case)
        loss.backward()
        check_grad(p.grad, d["g_p_pred"], case + " p_pred")
        check_grad(q.grad, d["g_p_gt"], case + " p_gt")
        if case.startswith("tie"):
            # row 0: prediction == GT -> every |dF| is 0 -> an exactly zero gradient (torch's sign(0) = 0)
            assert not p.grad[0].any() and not q.grad[0].any()


def test_sym_kl(dev, fx):
    from attwarp_amd import losses
    for case, d in fx("sym_kl"):
        p, q = T(d["p"], dev, True), T(d["q"], dev, True)
        loss = losses.sym_kl(p, q, eps=float(d["eps"].item()))
        check_loss(loss, d["loss"], case)
        loss.backward()
        check_grad(p.grad, d["g_p"], case + " p")
        check_grad(q.grad, d["g_q"], case + " q")
        if case.startswith("tie"):              # entries exactly at the clamp bound pass the gradient, those below do not
            eps = float(d["eps"].item())
            at, below = d["p"] == np.float32(eps), d["p"] < np.float32(eps)
            assert (N(p.grad)[at] != 0).all() and (N(p.grad)[below] == 0).all()


@pytest.mark.parametrize("fn", ["separable_recon_loss", "recon_l1"])
def test_recon_losses(dev, fx, fn):
    from attwarp_amd import losses
    for case, d in fx(fn):
        px, py, A = T(d["px"], dev, True), T(d["py"], dev, True), T(d["A"], dev)
        loss = getattr(losses, fn)(px, py, A)
        check_loss(loss, d["loss"], case)
        loss.backward()
        check_grad(px.grad, d["g_px"], case + " px")
        check_grad(py.grad, d["g_py"], case + " py")


def test_target_builders(dev, fx):
    from attwarp_amd import losses
    for case, d in fx("build_axis_cdf_targets"):
        Fx, Fy = losses.build_axis_cdf_targets(T(d["A"], dev), L=int(d["L"].item()))
        check_target(Fx, d["Fx"], case + " Fx")
        check_target(Fy, d["Fy"], case + " Fy")
        assert (Fx[:, -1] == 1).all() and (Fy[:, -1] == 1).all()
    for case, d in fx("cdf_from_density_downsample"):
        Fp = losses.cdf_from_density_downsample(T(d["p"], dev), int(d["L"].item()))
        check_target(Fp, d["F"], case)


def test_mix_with_uniform_and_entropy(dev, fx):
    from attwarp_amd import model
    for case, d in fx("mix_with_uniform"):
        p = T(d["p"], dev, True)
        alpha = float(d["alpha"].item())
        out = model.mix_with_uniform(p, alpha)
        if alpha <= 0:
            assert out is p
            continue
        check_target(out, d["out"], case)
        (out * T(d["w"], dev)).sum().backward()
        check_grad(p.grad, d["g_p"], case)
    for case, d in fx("entropy"):
        p = T(d["p"], dev, True)
        loss = model.entropy(p, eps=float(d["eps"].item()))
        check_loss(loss, d["loss"], case)
        loss.backward()
        check_grad(p.grad, d["g_p"], case)
        if case.startswith("tie"):
            eps = float(d["eps"].item())
            assert (N(p.grad)[d["p"] == np.float32(eps)] != 0).all() and (N(p.grad)[d["p"] < np.float32(eps)] == 0).all()


def stock_transform(A_full, tfms):
    """MN/trainer.py:187-193 on stock ops."""
    m = torch.tensor([1.0 if t == "sqrt" else 0.0 for t in tfms], device=A_full.device).view(-1, 1, 1, 1)
    pos = A_full.clamp_min(0.0)
    return pos.sqrt() * m + pos * (1.0 - m)


def test_trainer_block(dev, fx):
    from attwarp_amd import losses, pipeline
    for case, d in fx("trainer_block"):
        tfms = [str(t) for t in d["transforms"]]
        A_full = T(d["A_full"], dev)
        A, pxg, pyg = pipeline.trainer_attention_targets(A_full, tfms)
        check_target(A, d["A"], case + " A")
        check_target(pxg, d["px_gt"], case + " px_gt")
        check_target(pyg, d["py_gt"], case + " py_gt")
        # the pooled map equals the stock-op transform + the existing pool kernel with the trainer's sanitise, bit for bit
        want = pipeline.adaptive_avg_pool2d(stock_transform(A_full, tfms), (24, 24), sanitize=True)
        assert torch.equal(A, want), case
        px, py = T(d["px_s"], dev, True), T(d["py_s"], dev, True)
        loss = losses.pdf_l1_loss(px, py, pxg, pyg, int(d["img_w"].item()), int(d["img_h"].item()))
        check_loss(loss, d["loss"], case)
        loss.backward()
        check_grad(px.grad, d["g_px_s"], case + " px_s")
        check_grad(py.grad, d["g_py_s"], case + " py_s")


def test_pdf_l1_exact_tie_and_determinism(dev):
    from attwarp_amd import losses
    g = torch.Generator().manual_seed(5)
    px = torch.softmax(torch.randn(16, 24, generator=g), 1).to(dev)
    py = torch.softmax(torch.randn(16, 24, generator=g), 1).to(dev)
    gx, gy = px.clone(), torch.softmax(torch.randn(16, 24, generator=g), 1).to(dev)
    gx[3] = 0.5 * gx[3] + 0.5 / 24
    runs = []
    for _ in range(2):
        a, b = px.clone().requires_grad_(True), py.clone().requires_grad_(True)
        loss = losses.pdf_l1_loss(a, b, gx, gy, 512, 336)
        loss.backward()
        runs.append((loss.detach().clone(), a.grad.clone(), b.grad.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))            # bitwise repeatable
    gxr = runs[0][1]
    assert not gxr[torch.arange(16) != 3].any()                     # prediction == GT on x: exactly zero gradient
    assert gxr[3].abs().max() > 0
    # the other losses repeat bitwise as well
    p = torch.softmax(torch.randn(128, 24, generator=g), 1).to(dev)
    q = torch.softmax(torch.randn(128, 24, generator=g), 1).to(dev)
    A = torch.rand(128, 1, 24, 24, generator=g).to(dev)
    for fn in (lambda a: losses.recon_l1(a, q, A), lambda a: losses.separable_recon_loss(a, q, A),
               lambda a: losses.l1_cdf_loss(a, q), lambda a: losses.sym_kl(a, q)):
        outs = []
        for _ in range(2):
            a = p.clone().requires_grad_(True)
            loss = fn(a)
            loss.backward()
            outs.append((loss.detach().clone(), a.grad.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs_under_autocast_give_float32_losses(dev, dtype):
    from attwarp_amd import losses, model
    g = torch.Generator().manual_seed(7)
    p32 = torch.softmax(torch.randn(8, 24, generator=g), 1).to(dev)
    q32 = torch.softmax(torch.randn(8, 24, generator=g), 1).to(dev)
    A = torch.rand(8, 1, 24, 24, generator=g).to(dev)
    with torch.autocast("cuda", dtype=dtype):
        p = p32.to(dtype).requires_grad_(True)
        q = q32.to(dtype)
        outs = [losses.l1_cdf_loss(p, q), losses.sym_kl(p, q), losses.recon_l1(p, q, A), losses.separable_recon_loss(p, q, A),
                model.entropy(p), losses.pdf_l1_loss(model.mix_with_uniform(p, 0.3), q, q, q, 64, 48)]
    for o in outs:
        assert o.dtype == torch.float32 and o.dim() == 0
    sum(outs).backward()
    assert p.grad.dtype == dtype and torch.isfinite(p.grad.float()).all()
    # the upcast inputs give the float32 call's value
    ref = losses.l1_cdf_loss(p.detach().float(), q.float())
    assert torch.equal(outs[0], ref)


def _stock_block(px_s, py_s, pxg, pyg, W, H, A):
    from attwarp_amd import checkpoint_utils as cu
    def img(p, n):
        u = cu.upsample_pdf_right_inverse(p, n).clamp_min(0)
        return u / u.sum(dim=1, keepdim=True).clamp_min(1e-6)
    L_pdf = F.l1_loss(img(px_s, W), img(pxg, W)) + F.l1_loss(img(py_s, H), img(pyg, H))
    q = px_s.clamp_min(1e-8)
    r = py_s.clamp_min(1e-8)
    ent = -(q * q.log()).sum(1).mean() - (r * r.log()).sum(1).mean()
    Ap = A.clamp_min(0)
    Ap = Ap / Ap.sum(dim=(2, 3), keepdim=True).clamp_min(1e-6)
    P = torch.einsum("bh,bw->bhw", py_s, px_s)
    P = P / P.sum(dim=(1, 2), keepdim=True).clamp_min(1e-6)
    return L_pdf + 0.01 * ent + 0.1 * F.l1_loss(P.unsqueeze(1), Ap)


def test_one_optimiser_step_matches_stock_ops(dev):
    """MN/trainer.py:173-257 once through the new functions and once through the stock-op restatement, on a small seeded
    MarginalNet: the parameter updates of one SGD step agree within the gradient bound."""
    from attwarp_amd import losses, model, pipeline
    torch.manual_seed(0)
    B, img = 4, 96
    fmap = torch.randn(B, 32, 24, 24, device=dev)
    ttok, tmask = torch.randn(B, 5, 16, device=dev), torch.ones(B, 5, 1, device=dev)
    A_full = torch.rand(B, 1, img, img, device=dev)
    tfms = ["sqrt", "none", "identity", "sqrt"]
    updates = []
    for route in ("hip", "stock"):
        torch.manual_seed(1)
        net = model.MarginalNet(d_vis_in=32, d_txt_in=16, hidden=32).to(dev)
        before = [p.detach().clone() for p in net.parameters()]
        opt = torch.optim.SGD(net.parameters(), lr=1.0)
        A, pxg, pyg = pipeline.trainer_attention_targets(A_full, tfms)
        px, py = net(fmap, 24, 24, ttok, tmask)
        px_s, py_s = model.mix_with_uniform(px, 0.3), model.mix_with_uniform(py, 0.3)
        if route == "hip":
            loss = (losses.pdf_l1_loss(px_s, py_s, pxg, pyg, img, img)
                    + 0.01 * (model.entropy(px_s) + model.entropy(py_s)) + 0.1 * losses.recon_l1(px_s, py_s, A))
        else:
            loss = _stock_block(px_s, py_s, pxg, pyg, img, img, A)
        opt.zero_grad()
        loss.backward()
        opt.step()
        updates.append([(p.detach() - b).double().cpu().numpy() for p, b in zip(net.parameters(), before)])
    for hip, stock in zip(*updates):
        bound = 1e-4 * np.abs(stock).max() + 1e-9
        assert np.abs(hip - stock).max() <= bound, (np.abs(hip - stock).max(), bound)
