"""GPU tests of MarginalNet's training tail: film_axis_means and safe_softmax as autograd Functions with HIP backwards,
and MarginalNet.forward with grad taking the fused route (reference MN/model.py:8-14, 69-91; MN/trainer.py:173-257).
float64 restatements of the backwards: tests/marginalnet_train_ref.py."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from marginalnet_train_ref import film_axis_means_backward, safe_softmax_backward

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def _film_inputs(shape, dev, seed):
    B, Ch, H, W = shape
    g = torch.Generator(device=dev).manual_seed(seed)
    v = torch.randn(B, Ch, H, W, device=dev, generator=g)
    gb = torch.randn(B, 2 * Ch, device=dev, generator=g)
    gx = torch.randn(B, Ch, W, device=dev, generator=g)
    gy = torch.randn(B, Ch, H, device=dev, generator=g)
    return v, gb, gx, gy


def _stock_film_grads(v, gb, gx, gy):
    v, gb = v.detach().clone().requires_grad_(True), gb.detach().clone().requires_grad_(True)
    gamma, beta = gb.chunk(2, dim=1)
    w = gamma[:, :, None, None] * v + beta[:, :, None, None]
    torch.autograd.backward([w.mean(dim=2), w.mean(dim=3)], [gx, gy])
    return v.grad, gb.grad


def _fused_film_grads(v, gb, gx, gy):
    from attwarp_amd import model
    v, gb = v.detach().clone().requires_grad_(True), gb.detach().clone().requires_grad_(True)
    vx, vy = model.film_axis_means(v, gb)
    torch.autograd.backward([vx, vy], [gx, gy])
    return vx, vy, v.grad, gb.grad


@pytest.mark.parametrize("shape", [(3, 5, 24, 24), (2, 7, 17, 33), (1, 3, 63, 64), (5, 2, 1, 9), (2, 130, 24, 24)])
def test_film_backward_float32(dev, shape):
    v, gb, gx, gy = _film_inputs(shape, dev, sum(shape))
    vx, vy, dv, dgb = _fused_film_grads(v, gb, gx, gy)
    with torch.no_grad():
        from attwarp_amd import model
        ox, oy = model.film_axis_means(v, gb)
    assert torch.equal(vx, ox) and torch.equal(vy, oy)               # the forward is the inference kernel's
    sv, _ = _stock_film_grads(v, gb, gx, gy)
    assert torch.equal(dv, sv)                                        # bit for bit the stock float32 autograd
    _, ref, mag = film_axis_means_backward(N(v), N(gb), N(gx), N(gy))
    err = np.abs(N(dgb).astype(np.float64) - ref)
    assert (err <= 4 * EPS32 * mag + EPS32 * np.abs(ref)).all(), float((err / (mag + 1e-30)).max())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_film_16bit(dev, dt):
    from attwarp_amd import model
    shape = (3, 6, 24, 24)
    v, gb, gx, gy = _film_inputs(shape, dev, 77)
    v16, gb16 = v.to(dt), gb.to(dt)
    vx, vy, dv, dgb = _fused_film_grads(v16, gb16, gx, gy)
    with torch.no_grad():
        ox, oy = model.film_axis_means(v16.float(), gb16.float())
    assert vx.dtype == vy.dtype == torch.float32
    assert torch.equal(vx, ox) and torch.equal(vy, oy)
    assert dv.dtype == dt and dgb.dtype == dt
    sv, _ = _stock_film_grads(v16.float(), gb16.float(), gx, gy)
    assert torch.equal(dv, sv.to(dt))                                 # float32 dv, one rounding to the dtype
    _, ref, mag = film_axis_means_backward(N(v16.float()), N(gb16.float()), N(gx), N(gy))
    ulp = 2.0 ** (-11 if dt == torch.float16 else -8)
    err = np.abs(N(dgb.float()).astype(np.float64) - ref)
    assert (err <= 4 * EPS32 * mag + ulp * np.abs(ref)).all()
    # an inf upstream gradient reaches dv (GradScaler must see it), not sanitised to 0
    gxi = gx.clone()
    gxi[1, 2, 5] = float("inf")
    _, _, dvi, dgbi = _fused_film_grads(v16, gb16, gxi, gy)
    hit = dvi[1, 2, :, 5].float()
    assert not torch.isfinite(hit).any()
    assert not torch.isfinite(dgbi[1, [2, 6 + 2]].float()).any()
    assert torch.isfinite(dvi[0].float()).all()


def _softmax_grad(logits, g, dim, eps=1e-6):
    from attwarp_amd import model
    x = logits.detach().clone().requires_grad_(True)
    out = model.safe_softmax(x, dim=dim, eps=eps)
    out.backward(g)
    return out, x.grad


def _check_softmax_backward(got, x, g, eps=1e-6):
    ref, scale = safe_softmax_backward(x, g, eps)
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= 2e-6 * scale).all(), float((err / scale).max())
    assert (got[~np.isfinite(x)] == 0).all()


@pytest.mark.parametrize("n", [1, 24, 336, 4096])
def test_safe_softmax_backward(dev, n):
    from attwarp_amd import model
    gen = torch.Generator(device=dev).manual_seed(n)
    x = torch.randn(6, n, device=dev, generator=gen) * 3
    g = torch.randn(6, n, device=dev, generator=gen)
    out, gl = _softmax_grad(x, g, 1)
    with torch.no_grad():
        assert torch.equal(out, model.safe_softmax(x))                 # forward: the inference kernel
    _check_softmax_backward(N(gl), N(x), N(g))
    # dim = 0 on the transposed rows
    out0, gl0 = _softmax_grad(x.t().contiguous(), g.t().contiguous(), 0)
    assert torch.equal(out0.t(), out) and torch.equal(gl0.t(), gl)


def test_safe_softmax_backward_non_finite_and_ties(dev):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, 48)).astype(np.float32) * 3
    x[0, [3, 9]] = x[0].max() + 1.0                                   # tied maxima
    x[1, [0, 5, 17]] = [np.nan, np.inf, -np.inf]
    x[2] = 0.5                                                        # all tied
    x[3] = np.nan                                                     # all NaN
    x[4, :24] = -np.inf                                               # zeros of -inf are the maxima
    x[4, 24:] -= 5
    x[5, 7] = np.inf
    g = rng.standard_normal(x.shape).astype(np.float32)
    _, gl = _softmax_grad(torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev), 1)
    got = N(gl)
    _check_softmax_backward(got, x, g)
    assert (got[3] == 0).all()


def test_safe_softmax_long_rows_take_stock_route(dev):
    from attwarp_amd import model
    gen = torch.Generator(device=dev).manual_seed(50)
    x = torch.randn(3, 5000, device=dev, generator=gen)
    g = torch.randn(3, 5000, device=dev, generator=gen)
    out, gl = _softmax_grad(x, g, 1)
    xs = x.clone().requires_grad_(True)
    model.safe_softmax_stock(xs, 1, 1e-6).backward(g)
    assert torch.equal(gl, xs.grad)
    _check_softmax_backward(N(gl), N(x), N(g))


@pytest.mark.parametrize("autocast", [False, True])
def test_safe_softmax_output_dtypes_match_stock(dev, autocast):
    from attwarp_amd import model
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        x = torch.randn(4, 24, device=dev).to(dt).requires_grad_(True)
        with torch.autocast("cuda", enabled=autocast):
            a = model.safe_softmax(x, dim=1)
            b = model.safe_softmax_stock(x, dim=1)
        assert a.dtype == b.dtype, (dt, autocast, a.dtype, b.dtype)
        a.float().sum().backward()
        assert x.grad.dtype == dt


# ---- the network ---------------------------------------------------------------------------------------------------
def _small_net(golden, dev):
    from attwarp_amd import model
    g = golden("marginalnet")
    net = model.MarginalNet(32, 48, hidden=16)
    net.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd|")})
    args = (torch.from_numpy(g["fmap"]), 24, 24, torch.from_numpy(g["ttok"]), torch.from_numpy(g["tmask"]))
    return net, args


def _full_net(B=4):
    from conftest import marginalnet_full_state, marginalnet_full_inputs
    from attwarp_amd import model
    net = model.MarginalNet(1024, 4096, hidden=256)
    net.load_state_dict(marginalnet_full_state({k: tuple(v.shape) for k, v in net.state_dict().items()}))
    fmap, ttok, tmask = marginalnet_full_inputs(B)
    return net, (fmap, 24, 24, ttok, tmask)


def _to(args, dev):
    return tuple(a.to(dev) if isinstance(a, torch.Tensor) else a for a in args)


@pytest.mark.parametrize("which", ["small", "hidden256"])
def test_training_forward_tail_bits_equal_inference_kernels(dev, golden, which):
    from attwarp_amd import model
    net, args = _small_net(golden, dev) if which == "small" else _full_net()
    net = net.to(dev).train()
    args = _to(args, dev)
    cap = {}

    def keep(name):
        return lambda m, a, o: cap.__setitem__(name, (a[0].detach().clone(), o.detach().clone()))

    hs = [net.proj_v.register_forward_hook(keep("v")), net.film.register_forward_hook(keep("gb")),
          net.head_x.register_forward_hook(keep("hx")), net.head_y.register_forward_hook(keep("hy"))]
    px, py = net(*args)
    for h in hs:
        h.remove()
    assert px.requires_grad and py.requires_grad
    with torch.no_grad():
        vx, vy = model.film_axis_means(cap["v"][1], cap["gb"][1])
        assert torch.equal(vx, cap["hx"][0]) and torch.equal(vy, cap["hy"][0])
        assert torch.equal(model.safe_softmax(cap["hx"][1].squeeze(1)), px.detach())
        assert torch.equal(model.safe_softmax(cap["hy"][1].squeeze(1)), py.detach())
    gen = torch.Generator(device=dev).manual_seed(1)
    (px * torch.randn(px.shape, device=dev, generator=gen)).sum().backward(retain_graph=True)
    (py * torch.randn(py.shape, device=dev, generator=gen)).sum().backward()
    bad = [n for n, p in net.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not bad, bad


def _forward64(net, fmap, H, W, tok, mask):
    """The reference forward (MN/model.py:69-91) on the net's own modules, float64, CPU."""
    from attwarp_amd.model import safe_softmax_stock
    v = F.interpolate(net.proj_v(fmap), size=(H, W), mode="bilinear", align_corners=False)
    t = (tok * mask).sum(dim=1) / mask.sum(dim=1).clamp_min(1.0)
    gamma, beta = net.film(net.txt_pool(t)).chunk(2, dim=1)
    v = gamma[:, :, None, None] * v + beta[:, :, None, None]
    lx, ly = net.head_x(v.mean(dim=2)).squeeze(1), net.head_y(v.mean(dim=3)).squeeze(1)
    return safe_softmax_stock(lx, 1, net.eps), safe_softmax_stock(ly, 1, net.eps)


def _grads(net, px, py, wx, wy):
    net.zero_grad()
    ((px * wx).sum() + (py * wy).sum()).backward()
    return [p.grad.detach().double().cpu() for p in net.parameters()]


@pytest.mark.parametrize("which", ["small", "hidden256"])
def test_training_gradients_against_float64(dev, golden, which):
    net, args = _small_net(golden, dev) if which == "small" else _full_net(2)
    fmap, H, W, tok, mask = args
    gen = torch.Generator().manual_seed(3)
    wx = torch.randn(fmap.shape[0], W, generator=gen)
    wy = torch.randn(fmap.shape[0], H, generator=gen)
    n64 = copy.deepcopy(net).double()
    g64 = _grads(n64, *_forward64(n64, fmap.double(), H, W, tok.double(), mask.double()), wx.double(), wy.double())
    ng = net.to(dev).train()
    a = _to(args, dev)
    fused = _grads(ng, *ng(*a), wx.to(dev), wy.to(dev))
    stock = _grads(ng, *ng(*a, stock=True), wx.to(dev), wy.to(dev))

    def err(gs):
        return float(np.sqrt(sum(float(((g - r) ** 2).sum()) for g, r in zip(gs, g64))))
    ref = float(np.sqrt(sum(float((r ** 2).sum()) for r in g64)))
    e_fused, e_stock = err(fused) / ref, err(stock) / ref
    assert e_fused <= 2.0 * e_stock + 1e-7, (e_fused, e_stock)


def test_autocast_trainer_step(dev):
    """MN/trainer.py:173-257 under autocast + GradScaler: the network into mix_with_uniform, pdf_l1_loss and recon_l1,
    then clip_grad_norm_ and the optimiser step, on the fused route and on the stock route."""
    from attwarp_amd import losses, model, pipeline
    net0, args = _full_net(4)
    a = _to(args, dev)
    img = 96
    gen = torch.Generator(device=dev).manual_seed(9)
    A_full = torch.rand(4, 1, img, img, device=dev, generator=gen)
    A, pxg, pyg = pipeline.trainer_attention_targets(A_full, ["sqrt", "none", "identity", "sqrt"])
    dtypes = {}
    for stock in (False, True):
        net = copy.deepcopy(net0).to(dev).train()
        opt = torch.optim.AdamW(net.parameters(), lr=3e-4, weight_decay=1e-4)
        scaler = torch.amp.GradScaler("cuda")
        with torch.autocast("cuda"):
            px, py = net(*a, stock=stock)
            px_s, py_s = model.mix_with_uniform(px, 0.1), model.mix_with_uniform(py, 0.1)
            loss = losses.pdf_l1_loss(px_s, py_s, pxg, pyg, img, img) + 0.1 * losses.recon_l1(px_s, py_s, A)
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        scaler.step(opt)
        scaler.update()
        assert np.isfinite(scaler.get_scale()) and scaler.get_scale() > 0
        assert all(p.grad is not None for p in net.parameters())
        dtypes[stock] = (px.dtype, py.dtype, loss.dtype)
    assert dtypes[False] == dtypes[True]


def _gpu_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_training_step_kernel_trace(dev):
    net, args = _full_net(4)
    net = net.to(dev).train()
    a = _to(args, dev)

    def step(stock):
        def run():
            net.zero_grad(set_to_none=True)
            px, py = net(*a, stock=stock)
            (px.sum() + (py * py).sum()).backward()
        return run
    fused, stock = _gpu_kernels(step(False)), _gpu_kernels(step(True))
    for k in ("film_axis_means_kernel", "film_axis_means_backward_kernel", "safe_softmax_kernel",
              "safe_softmax_backward_kernel"):
        assert any(k in n for n in fused), k
        assert not any(k in n for n in stock), k
    assert len(fused) + 20 <= len(stock), (len(fused), len(stock))
