"""GPU tests of attwarp_amd.optim.AdamW (csrc/optim.hip) against tests/optim_ref.py, the float64 restatement.

Tolerance (per compared tensor of p, m, v): the stock float32 route (clip_grad_norm_ + torch.optim.AdamW, with the stock
GradScaler lines where a scaler is used) runs on the GPU from the same inputs; with e = max |x - restatement|,
    e_kernel <= 2 * e_stock + 8 * 2^-24 * max|restatement| * steps taken.
grad_norm is compared with the restatement at 2^-22 relative.  Skips, misalignment and repeatability are exact.
Recorded on an MI355X (one-step cases, max-abs over max|ref|, kernel / stock): p 9.7e-8 / 9.7e-8, m 1.09e-7 / 1.09e-7,
v 1.24e-7 / 1.37e-7."""
import copy

import pytest
import torch

from optim_ref import AdamWRef, Scale

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -24
HYPER = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _optim():
    from attwarp_amd import optim
    return optim


def _numels():
    C = _optim().CHUNK
    return [1, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3]


def _randn(shapes, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen) * scale for s in shapes]


def _loaded_state(shapes, seed, t=7):
    gen = torch.Generator().manual_seed(seed)
    m = [torch.randn(s, generator=gen) * 0.03 for s in shapes]
    v = [torch.rand(s, generator=gen) * 2e-3 + 1e-5 for s in shapes]
    return m, v, [t] * len(shapes)


def _torch_state_dict(n, m, v, t, group):
    """A torch.optim.AdamW state dict holding the given moments and step counts."""
    g = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False, foreach=None,
             capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
    g.update(group)
    g["params"] = list(range(n))
    return {"state": {i: {"step": torch.tensor(float(t[i])), "exp_avg": m[i].clone(), "exp_avg_sq": v[i].clone()}
                      for i in range(n)}, "param_groups": [g]}


def _params(p0, dev):
    return [torch.nn.Parameter(p.to(dev)) for p in p0]


def _snapshot(opt, params):
    """p, m, v (float64 CPU lists) and the step counts of an optimiser of either class."""
    out = {"p": [], "m": [], "v": [], "t": []}
    for p in params:
        st = opt.state.get(p, {})
        out["p"].append(p.detach().double().cpu())
        out["m"].append(st["exp_avg"].double().cpu() if st else torch.zeros(p.shape, dtype=torch.float64))
        out["v"].append(st["exp_avg_sq"].double().cpu() if st else torch.zeros(p.shape, dtype=torch.float64))
        out["t"].append(int(st["step"]) if st else 0)
    return out


def _check(ours, stock, ref, steps, what=""):
    """The bound of the module docstring for every tensor of p, m, v; returns the worst ratios for the record."""
    assert ours["t"] == stock["t"] == list(ref.t), (what, ours["t"], stock["t"], ref.t)
    worst = {}
    for name, r_all in (("p", ref.p), ("m", ref.m), ("v", ref.v)):
        for i, r in enumerate(r_all):
            e_k = float((ours[name][i] - r).abs().max())
            e_s = float((stock[name][i] - r).abs().max())
            mag = float(r.abs().max())
            bound = 2.0 * e_s + 8.0 * EPS32 * mag * max(steps, 1)
            assert e_k <= bound, f"{what} {name}[{i}] numel {r.numel()}: kernel {e_k:.3e} stock {e_s:.3e} bound {bound:.3e}"
            w = worst.setdefault(name, [0.0, 0.0])
            w[0], w[1] = max(w[0], e_k / max(mag, 1e-300)), max(w[1], e_s / max(mag, 1e-300))
    return worst


def _check_norm(got, ref_norm):
    assert abs(float(got) - ref_norm) <= 2.0 ** -22 * ref_norm, (float(got), ref_norm)


def _stock_step(opt, params, grads, mgn):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()
    if mgn is not None:
        torch.nn.utils.clip_grad_norm_(params, mgn)
    opt.step()


def _ours_step(opt, params, grads):
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()


# ---- one-step parity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", [0, 7])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("clip", ["active", "inactive", None])
def test_one_step_parity(dev, clip, wd, t0):
    optim = _optim()
    shapes = [(n,) for n in _numels()]
    p0, g0 = _randn(shapes, 1), _randn(shapes, 2, 0.05)
    total = float(torch.cat([g.double() for g in g0]).norm())
    mgn = {"active": 0.25 * total, "inactive": 1e30, None: None}[clip]
    hyper = dict(HYPER, weight_decay=wd)
    ref = AdamWRef(p0, [dict(idx=list(range(len(p0))), **hyper)], max_grad_norm=mgn)
    po, ps = _params(p0, dev), _params(p0, dev)
    ours = optim.AdamW(po, **hyper, max_grad_norm=mgn)
    stock = torch.optim.AdamW(ps, **hyper)
    if t0:
        m, v, t = _loaded_state(shapes, 3, t0)
        ref.load(m, v, t)
        ours.load_state_dict(_torch_state_dict(len(p0), m, v, t, hyper))
        stock.load_state_dict(_torch_state_dict(len(p0), m, v, t, hyper))
    gd = [g.to(dev) for g in g0]
    keep = [g.clone() for g in gd]
    _ours_step(ours, po, gd)
    _stock_step(stock, ps, gd, mgn)
    assert ref.step(g0)
    assert all(torch.equal(a, b) for a, b in zip(gd, keep)), "gradients were written"
    worst = _check(_snapshot(ours, po), _snapshot(stock, ps), ref, 1, f"clip={clip} wd={wd} t0={t0}")
    print(f"one step clip={clip} wd={wd} t0={t0}: (kernel, stock) relative distance to float64 {worst}")
    _check_norm(ours.grad_norm, ref.grad_norm)
    assert ours.grad_norm.dtype == torch.float32 and ours.grad_norm.dim() == 0 and ours.grad_norm.device == po[0].device
    assert all(ours.state[p]["step"].dtype == torch.float32 and ours.state[p]["step"].dim() == 0 for p in po)


# ---- layouts ---------------------------------------------------------------------------------------------------------
def _slice_of(t, off, dev):
    buf = torch.zeros(t.numel() + off, device=dev)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def test_misaligned_views_equal_aligned_bit_for_bit(dev):
    """p, m, v as slices of flat buffers at element offsets 1, 2, 3 (the gradient at yet another offset): the scalar route
    computes the same bits as the 16-byte route, the norm included."""
    optim = _optim()
    shapes = [(n,) for n in _numels()]
    p0, g0 = _randn(shapes, 4), _randn(shapes, 5, 0.05)
    m, v, t = _loaded_state(shapes, 6)
    total = float(torch.cat([g.double() for g in g0]).norm())
    res = {}
    for layout in ("aligned", "views"):
        if layout == "aligned":
            params = _params(p0, dev)
            grads = [g.to(dev) for g in g0]
        else:
            params = [torch.nn.Parameter(_slice_of(p, 1 + i % 3, dev)) for i, p in enumerate(p0)]
            grads = [_slice_of(g, (4 + i % 3) % 4, dev) for i, g in enumerate(g0)]
            assert all(p.data_ptr() % 16 != 0 for p in params)
        opt = optim.AdamW(params, **HYPER, max_grad_norm=0.25 * total)
        opt.load_state_dict(_torch_state_dict(len(p0), m, v, t, HYPER))
        if layout == "views":
            for i, p in enumerate(params):
                opt.state[p]["exp_avg"] = _slice_of(opt.state[p]["exp_avg"], (2 + i % 3) % 4, dev)
                opt.state[p]["exp_avg_sq"] = _slice_of(opt.state[p]["exp_avg_sq"], (3 + i % 3) % 4, dev)
        for _ in range(2):
            _ours_step(opt, params, grads)
        res[layout] = ([p.detach().clone() for p in params], [opt.state[p]["exp_avg"].clone() for p in params],
                       [opt.state[p]["exp_avg_sq"].clone() for p in params], opt.grad_norm.clone(),
                       [int(opt.state[p]["step"]) for p in params])
    a, b = res["aligned"], res["views"]
    for k in range(3):
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), "pmv"[k]
    assert torch.equal(a[3], b[3]) and a[4] == b[4] == [9] * len(p0)


def test_channels_last_gradient_and_parameter(dev):
    optim = _optim()
    p0, g0 = _randn([(8, 6, 3, 3), (5,)], 7), _randn([(8, 6, 3, 3), (5,)], 8, 0.05)
    res = []
    for p_cl, g_cl in ((False, False), (False, True), (True, False), (True, True)):
        params = _params(p0, dev)
        grads = [g.to(dev) for g in g0]
        if p_cl:
            params[0] = torch.nn.Parameter(params[0].detach().contiguous(memory_format=torch.channels_last))
        if g_cl:
            grads[0] = grads[0].contiguous(memory_format=torch.channels_last)
        keep = grads[0].clone()
        opt = optim.AdamW(params, **HYPER, max_grad_norm=0.1)
        for _ in range(2):
            _ours_step(opt, params, grads)
        assert torch.equal(grads[0], keep) and grads[0].stride() == keep.stride()
        assert opt.state[params[0]]["exp_avg"].stride() == params[0].stride()
        res.append([params[0].detach().clone(), opt.state[params[0]]["exp_avg"].clone(),
                    opt.state[params[0]]["exp_avg_sq"].clone(), params[1].detach().clone()])
    for r in res[1:]:
        # the norm's summation order follows the memory order: within a unit of its float32 rounding, elementwise equal
        # where the layouts agree
        for x, y in zip(res[0], r):
            assert torch.allclose(x, y, rtol=4 * EPS32, atol=0)
    assert all(torch.equal(x, y) for x, y in zip(res[0], res[1])), "a channels-last gradient of a contiguous weight"


# ---- many tensors, many partials ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 130])
def test_more_tensors_than_one_launch_holds(dev, n):
    """65 and 130 tensors (2 and 3 launch groups), one of 3 chunks in the last group, clip active: the norm spans groups."""
    optim = _optim()
    C = optim.CHUNK
    shapes = [(1 + i % 7,) for i in range(n - 1)] + [(3 * C,)]
    p0, g0 = _randn(shapes, 9), _randn(shapes, 10, 0.05)
    total = float(torch.cat([g.double() for g in g0]).norm())
    mgn = 0.5 * total
    ref = AdamWRef(p0, [dict(idx=list(range(n)), **HYPER)], max_grad_norm=mgn)
    po, ps = _params(p0, dev), _params(p0, dev)
    ours, stock = optim.AdamW(po, **HYPER, max_grad_norm=mgn), torch.optim.AdamW(ps, **HYPER)
    gd = [g.to(dev) for g in g0]
    for step in (1, 2):
        _ours_step(ours, po, gd)
        _stock_step(stock, ps, gd, mgn)
        assert ref.step(g0)
        _check(_snapshot(ours, po), _snapshot(stock, ps), ref, step, f"n={n} step={step}")
        _check_norm(ours.grad_norm, ref.grad_norm)


def test_more_partials_than_one_stride_of_the_finishing_sum(dev):
    """One tensor of 4 * 256 + 1 chunks: the finishing workgroup's threads each sum several partials; two runs agree bit
    for bit and the norm is the restatement's."""
    optim = _optim()
    n = (4 * 256 + 1) * optim.CHUNK - 5
    gen = torch.Generator(device=dev).manual_seed(12)
    p0 = torch.randn(n, device=dev, generator=gen)
    g = torch.randn(n, device=dev, generator=gen) * 0.05
    ref_norm = float(g.double().norm())
    out = []
    for _ in range(2):
        p = torch.nn.Parameter(p0.clone())
        opt = optim.AdamW([p], **HYPER, max_grad_norm=0.5 * ref_norm)
        _ours_step(opt, [p], [g])
        out.append((p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(),
                    opt.grad_norm.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*out))
    _check_norm(out[0][3], ref_norm)
    coef = 0.5 * ref_norm / (ref_norm + 1e-6)
    want_m = (1.0 - HYPER["betas"][0]) * coef * g.double()
    assert float((out[0][1].double() - want_m).abs().max()) <= 8 * EPS32 * float(want_m.abs().max())


# ---- AMP ---------------------------------------------------------------------------------------------------------------
def _amp_grads(shapes, scale, step):
    g = _randn(shapes, 100 + step, 0.05)
    raw = [x * scale for x in g]                    # a power-of-two scale: exact
    if step == 2:
        raw[-1].view(-1)[-1] = float("inf")
    if step == 3:
        raw[0].view(-1)[0] = float("nan")
    return raw


@pytest.mark.parametrize("order", ["step", "unscale_first"])
def test_amp_with_the_stock_gradscaler(dev, order):
    """init_scale=1024, growth_interval=2; step 2 carries an inf in the last element of the last tensor, step 3 a NaN in the
    1-element tensor: both are skipped bit for bit and halve the scale, step 4 uses the un-advanced t = 2, steps 4 and 5
    double the scale.  Scale and tracker follow the restatement's schedule and the stock route's."""
    optim = _optim()
    shapes = [(n,) for n in _numels()]
    p0 = _randn(shapes, 13)
    mgn = 0.3
    ref = AdamWRef(p0, [dict(idx=list(range(len(p0))), **HYPER)], max_grad_norm=mgn)
    sched = Scale(init_scale=1024.0, growth_interval=2)
    po, ps = _params(p0, dev), _params(p0, dev)
    ours, stock = optim.AdamW(po, **HYPER, max_grad_norm=mgn), torch.optim.AdamW(ps, **HYPER)
    sc_o = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    sc_s = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    sc_o.scale(torch.zeros((), device=dev)), sc_s.scale(torch.zeros((), device=dev))
    taken_steps = 0
    scales = []
    for step in range(1, 6):
        scale = float(sched.scale)
        raw = _amp_grads(shapes, scale, step)
        before = _snapshot(ours, po) if step > 1 else None
        bits = [(p.detach().clone(), ours.state[p]["exp_avg"].clone(), ours.state[p]["exp_avg_sq"].clone(),
                 ours.state[p]["step"].clone()) for p in po] if step > 1 else None
        for p, g in zip(po, raw):
            p.grad = g.to(dev)
        if order == "unscale_first":
            sc_o.unscale_(ours)
        sc_o.step(ours)
        sc_o.update()
        for p, g in zip(ps, raw):
            p.grad = g.to(dev)
        sc_s.unscale_(stock)
        torch.nn.utils.clip_grad_norm_(ps, mgn)
        sc_s.step(stock)
        sc_s.update()
        taken = ref.step(raw, scale=scale)
        sched.update(not taken)
        assert taken == (step not in (2, 3))
        taken_steps += int(taken)
        if taken:
            _check(_snapshot(ours, po), _snapshot(stock, ps), ref, taken_steps, f"{order} step={step}")
            _check_norm(ours.grad_norm, ref.grad_norm)
        else:
            for p, (bp, bm, bv, bt) in zip(po, bits):
                st = ours.state[p]
                assert torch.equal(p.detach(), bp) and torch.equal(st["exp_avg"], bm) and torch.equal(st["exp_avg_sq"], bv)
                assert torch.equal(st["step"], bt)
            assert _snapshot(ours, po)["t"] == before["t"] == list(ref.t)
            assert not torch.isfinite(ours.grad_norm)
        so, ss = sc_o.state_dict(), sc_s.state_dict()
        assert so["scale"] == ss["scale"] == float(sched.scale), (step, so, ss, sched.scale)
        assert so["_growth_tracker"] == ss["_growth_tracker"] == sched.tracker
        scales.append(so["scale"])
    assert scales == [1024.0, 512.0, 256.0, 256.0, 512.0] and list(ref.t) == [3] * len(p0)


def test_no_host_sync_under_the_scaler(dev):
    optim = _optim()
    w = torch.nn.Parameter(torch.randn(300, device=dev))
    x = torch.randn(300, device=dev)
    opt = optim.AdamW([w], **HYPER, max_grad_norm=1.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    for _ in range(2):                                  # first use: lazy initialisations outside the checked region
        opt.zero_grad(set_to_none=True)
        scaler.scale((w * x).sum()).backward()
        scaler.step(opt)
        scaler.update()
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            x.sum().item()
            raised = False
        except RuntimeError:
            raised = True
        if not raised:
            pytest.skip("set_sync_debug_mode('error') does not flag .item() on this build")
        opt.zero_grad(set_to_none=True)
        scaler.scale((w * x).sum()).backward()
        scaler.step(opt)
        scaler.update()
        norm = opt.grad_norm                            # a device tensor: reading it later is the caller's sync
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert int(opt.state[w]["step"]) == 3 and torch.isfinite(norm)


# ---- None gradients, groups, state dict --------------------------------------------------------------------------------
def test_parameter_without_gradient_is_left_out(dev):
    optim = _optim()
    shapes = [(257,), (33,), (5,)]
    p0 = _randn(shapes, 14)
    ref = AdamWRef(p0, [dict(idx=[0, 1, 2], **HYPER)], max_grad_norm=0.2)
    po, ps = _params(p0, dev), _params(p0, dev)
    ours, stock = optim.AdamW(po, **HYPER, max_grad_norm=0.2), torch.optim.AdamW(ps, **HYPER)
    for step in (1, 2, 3):
        g0 = _randn(shapes, 20 + step, 0.05)
        if step == 2:
            g0[1] = None
            hold = (po[1].detach().clone(), ours.state[po[1]]["exp_avg"].clone(), ours.state[po[1]]["exp_avg_sq"].clone())
        gd = [None if g is None else g.to(dev) for g in g0]
        _ours_step(ours, po, gd)
        _stock_step(stock, ps, gd, 0.2)
        assert ref.step(g0)
        if step == 2:
            st = ours.state[po[1]]
            assert torch.equal(po[1].detach(), hold[0]) and torch.equal(st["exp_avg"], hold[1]) and torch.equal(st["exp_avg_sq"], hold[2])
        _check(_snapshot(ours, po), _snapshot(stock, ps), ref, step, f"step={step}")
        _check_norm(ours.grad_norm, ref.grad_norm)
    assert list(ref.t) == [3, 2, 3]
    for p in po:
        p.grad = None
    ours.step()
    assert float(ours.grad_norm) == 0.0 and _snapshot(ours, po)["t"] == [3, 2, 3]


def test_two_param_groups_with_a_global_clip(dev):
    optim = _optim()
    C = optim.CHUNK
    shapes = [(C + 1,), (7,), (300,), (2, 3, 4)]
    p0 = _randn(shapes, 15)
    h0 = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
    h1 = dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.0)
    ref = AdamWRef(p0, [dict(idx=[0, 1], **h0), dict(idx=[2, 3], **h1)], max_grad_norm=0.5)
    po, ps = _params(p0, dev), _params(p0, dev)
    ours = optim.AdamW([dict(params=po[:2], **h0), dict(params=po[2:], **h1)], max_grad_norm=0.5)
    stock = torch.optim.AdamW([dict(params=ps[:2], **h0), dict(params=ps[2:], **h1)])
    for step in (1, 2, 3):
        g0 = _randn(shapes, 30 + step, 0.05)
        gd = [g.to(dev) for g in g0]
        _ours_step(ours, po, gd)
        _stock_step(stock, ps, gd, 0.5)
        assert ref.step(g0)
        _check(_snapshot(ours, po), _snapshot(stock, ps), ref, step, f"step={step}")
        _check_norm(ours.grad_norm, ref.grad_norm)


def test_state_dict_interchanges_with_torch_adamw(dev):
    optim = _optim()
    shapes = [(257,), (4, 5), (1,)]
    p0 = _randn(shapes, 16)
    grads = [_randn(shapes, 40 + s, 0.05) for s in range(4)]
    mgn = 0.2
    for first in ("ours", "torch"):
        ref = AdamWRef(p0, [dict(idx=[0, 1, 2], **HYPER)], max_grad_norm=mgn)
        pa, pb = _params(p0, dev), _params(p0, dev)
        make = {"ours": lambda ps: optim.AdamW(ps, **HYPER, max_grad_norm=mgn), "torch": lambda ps: torch.optim.AdamW(ps, **HYPER)}
        step = {"ours": _ours_step, "torch": lambda o, ps, g: _stock_step(o, ps, g, mgn)}
        second = "torch" if first == "ours" else "ours"
        a, b = make[first](pa), make[second](pb)
        for s in (0, 1):
            step[first](a, pa, [g.to(dev) for g in grads[s]])
            assert ref.step(grads[s])
        sd = copy.deepcopy(a.state_dict())
        assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
        assert sd["state"][0]["step"].dim() == 0 and sd["state"][0]["step"].dtype == torch.float32
        if first == "ours":
            assert set(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0]) | \
                {"max_grad_norm", "norm_eps"} == set(sd["param_groups"][0])
        with torch.no_grad():
            for x, y in zip(pb, pa):
                x.copy_(y)
        b.load_state_dict(sd)
        if second == "ours":
            assert b.param_groups[0]["max_grad_norm"] == mgn and b.param_groups[0]["norm_eps"] == 1e-6
        # continue on both sides
        for s in (2, 3):
            gd = [g.to(dev) for g in grads[s]]
            step[first](a, pa, gd)
            step[second](b, pb, gd)
            assert ref.step(grads[s])
        sa, sb = _snapshot(a, pa), _snapshot(b, pb)
        o, t = (sa, sb) if first == "ours" else (sb, sa)
        _check(o, t, ref, 4, f"first={first}")
        assert o["t"] == [4, 4, 4]


# ---- streams -----------------------------------------------------------------------------------------------------------
def test_side_stream_and_alternating_streams(dev):
    optim = _optim()
    shapes = [(n,) for n in _numels()]
    p0 = _randn(shapes, 17)
    grads = [[g.to(dev) for g in _randn(shapes, 50 + s, 0.05)] for s in range(4)]
    torch.cuda.synchronize()

    def run(mode):
        params = _params(p0, dev)
        opt = optim.AdamW(params, **HYPER, max_grad_norm=0.2)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        norms, ev = [], None
        for k, g in enumerate(grads):
            for p, x in zip(params, g):
                p.grad = x
            if mode == "default":
                opt.step()
            else:
                s = s1 if (mode == "side" or k % 2 == 0) else s2
                if ev is not None:
                    s.wait_event(ev)
                with torch.cuda.stream(s):
                    opt.step()
                    ev = s.record_event()
            norms.append(opt.grad_norm)
        torch.cuda.synchronize()
        return ([p.detach().clone() for p in params] + [opt.state[p]["exp_avg_sq"].clone() for p in params]
                + [opt.grad_norm.clone()], [int(opt.state[p]["step"]) for p in params])

    base, t = run("default")
    assert t == [4] * len(p0)
    for mode in ("side", "alternating"):
        got, t2 = run(mode)
        assert t2 == t and all(torch.equal(x, y) for x, y in zip(base, got)), mode


# ---- rejections --------------------------------------------------------------------------------------------------------
def test_rejections(dev):
    optim = _optim()
    P = lambda *a, **k: torch.nn.Parameter(torch.zeros(*a, device=dev, **k))
    with pytest.raises(TypeError, match="float32"):
        optim.AdamW([P(4, dtype=torch.float16)])
    with pytest.raises(TypeError, match="float32"):
        optim.AdamW([P(4, dtype=torch.float64)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.AdamW([P(4), torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(ValueError, match="amsgrad"):
        optim.AdamW([P(4)], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        optim.AdamW([P(4)], maximize=True)
    with pytest.raises(ValueError, match="tensor lr"):
        optim.AdamW([P(4)], lr=torch.tensor(1e-3, device=dev))
    with pytest.raises(ValueError, match="without gaps"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(8, device=dev)[::2])])
    p = P(4, 3)
    opt = optim.AdamW([p])
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3)).to(dev)
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    q = P(4)
    opt = optim.AdamW([q])
    q.grad_dtype = None
    q.grad = torch.zeros(4, device=dev, dtype=torch.float16)
    with pytest.raises(TypeError, match="gradients must be float32"):
        opt.step()
    r = P(4)
    ams = torch.optim.AdamW([r], amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        optim.AdamW([r]).load_state_dict(ams.state_dict())
    assert not opt.state[q] and float(q.abs().sum()) == 0.0


# ---- integration -------------------------------------------------------------------------------------------------------
def test_marginalnet_three_steps_under_autocast(dev, golden):
    """MarginalNet(32, 48, hidden=16) under autocast + GradScaler (MN/trainer.py:210-264): three steps with this optimiser;
    a deep copy takes the reference's four lines on the SAME raw gradients (so the comparison has no feedback through the
    network) and the float64 restatement follows them too."""
    from attwarp_amd import model
    optim = _optim()
    g = golden("marginalnet")
    net = model.MarginalNet(32, 48, hidden=16)
    net.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd|")})
    net = net.to(dev).train()
    twin = copy.deepcopy(net)
    args = (torch.from_numpy(g["fmap"]).to(dev), 24, 24, torch.from_numpy(g["ttok"]).to(dev), torch.from_numpy(g["tmask"]).to(dev))
    po, ps = list(net.parameters()), list(twin.parameters())
    hyper = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    ref = AdamWRef([p.detach().cpu() for p in po], [dict(idx=list(range(len(po))), **hyper)], max_grad_norm=1.0)
    ours, stock = optim.AdamW(po, **hyper, max_grad_norm=1.0), torch.optim.AdamW(ps, **hyper)
    sc_o, sc_s = torch.amp.GradScaler("cuda", init_scale=1024.0), torch.amp.GradScaler("cuda", init_scale=1024.0)
    sc_s.scale(torch.zeros((), device=dev))
    gen = torch.Generator(device=dev).manual_seed(5)
    for step in (1, 2, 3):
        with torch.autocast("cuda"):
            px, py = net(*args)
            px_s, py_s = model.mix_with_uniform(px, 0.1), model.mix_with_uniform(py, 0.1)
            loss = (px_s * torch.randn(px.shape, device=dev, generator=gen)).sum() + (py_s * py_s).sum()
        ours.zero_grad(set_to_none=True)
        sc_o.scale(loss).backward()
        raw = [p.grad.clone() for p in po]
        assert all(x is not None for x in raw)
        sc_o.step(ours)
        sc_o.update()
        assert all(torch.equal(p.grad, x) for p, x in zip(po, raw)), "scaler.step(opt) left the scaled gradients"
        for p, x in zip(ps, raw):
            p.grad = x.clone()
        sc_s.unscale_(stock)
        stock_norm = torch.nn.utils.clip_grad_norm_(ps, 1.0)
        sc_s.step(stock)
        sc_s.update()
        assert ref.step([x.cpu() for x in raw], scale=1024.0)
        _check(_snapshot(ours, po), _snapshot(stock, ps), ref, step, f"step={step}")
        _check_norm(ours.grad_norm, ref.grad_norm)
        assert abs(float(stock_norm) - ref.grad_norm) <= 1e-4 * ref.grad_norm
        assert sc_o.get_scale() == sc_s.get_scale() == 1024.0
