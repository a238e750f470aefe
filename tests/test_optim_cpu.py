"""CPU-only checks of the optimiser step: tests/optim_ref.py (the float64 restatement the GPU tests compare against) is
pinned against the real torch.optim.AdamW + clip_grad_norm_ + torch.amp.GradScaler("cpu") on float64 parameters, at the
operating point and at every hyperparameter edge of tests/optim_cases.py; its float32 per-element restatement is pinned
against torch's float32 CPU route with the bound the GPU tests put on the kernel, on the inputs of the GPU sweep
(tests/test_optim_sweep_gpu.py), so those inputs are ones a correct float32 implementation passes; and the parts of
attwarp_amd.optim that need no GPU (rejections, the workspace size of the library, the state-dict keys)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import optim_cases as oc
from test_optim_gpu import _numels
from optim_ref import AdamWRef, Scale, adamw_element_f32, clip_coef, inv_scale32, next_count

SHAPES = [(1,), (3,), (4097,), (256, 256, 3, 3), (512, 256)]


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_restatement_matches_torch_float64():
    """Six steps, an inf gradient at step 3, growth_interval=2: p, m, v, step counts, scale and norm agree to 1e-12."""
    gen = torch.Generator().manual_seed(11)
    p0 = [torch.randn(s, generator=gen, dtype=torch.float64) for s in SHAPES]
    hyper = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
    params = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.AdamW(params, **hyper)
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0, growth_interval=2)
    scaler.scale(torch.zeros(()))                      # creates the scale tensor, as scaler.scale(loss) does in a trainer
    ref = AdamWRef(p0, [dict(idx=list(range(len(p0))), **hyper)], max_grad_norm=1.0)
    sched = Scale(init_scale=1024.0, growth_interval=2)
    worst = 0.0
    for step in range(1, 7):
        scale = float(sched.scale)
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * 0.05 * scale for s in SHAPES]
        if step == 3:
            grads[-1].view(-1)[-1] = float("inf")
        for p, g in zip(params, grads):
            p.grad = g.clone()
        scaler.unscale_(opt)
        norm = torch.nn.utils.clip_grad_norm_(params, 1.0)
        scaler.step(opt)
        scaler.update()
        taken = ref.step(grads, scale=scale)
        sched.update(not taken)
        assert taken == (step != 3)
        assert float(scaler.get_scale()) == float(sched.scale)
        assert int(scaler._growth_tracker.item()) == sched.tracker
        if taken:
            worst = max(worst, abs(float(norm) - ref.grad_norm) / ref.grad_norm)
        else:
            assert math.isinf(float(norm)) and math.isinf(ref.grad_norm)
        for i, p in enumerate(params):
            st = opt.state[p]
            assert int(st["step"]) == ref.t[i]
            worst = max(worst, _rel(p.detach(), ref.p[i]), _rel(st["exp_avg"], ref.m[i]), _rel(st["exp_avg_sq"], ref.v[i]))
    assert [float(x) for x in (sched.scale,)] == [2048.0] and ref.t == [5] * len(SHAPES)
    print(f"restatement vs torch float64: worst relative distance {worst:.3e}")
    assert worst <= 1e-12, worst


def _cpu_snapshot(opt, params):
    out = {"p": [], "m": [], "v": [], "t": []}
    for p in params:
        st = opt.state.get(p, {})
        out["p"].append(p.detach().double())
        out["m"].append(st["exp_avg"].double() if st else torch.zeros(p.shape, dtype=torch.float64))
        out["v"].append(st["exp_avg_sq"].double() if st else torch.zeros(p.shape, dtype=torch.float64))
        out["t"].append(int(st["step"]) if st else 0)
    return out


def _edge_setup(t0, clip, dtype, n=4097):
    """The edge sweep on the CPU in `dtype`: one param group per edge.  Returns the stock optimiser and its parameters,
    the float64 restatement, the float32 gradients and max_grad_norm."""
    edges = oc.edge_hypers()
    p0, g0, m, v, t = oc.edge_inputs(n, t0)
    mgn = oc.clip_value(clip, oc.total_norm(g0))
    groups = [dict(idx=[i], **h) for i, (_, h) in enumerate(edges)]
    ref = AdamWRef(p0, groups, max_grad_norm=mgn)
    params = [torch.nn.Parameter(p.to(dtype)) for p in p0]
    opt = torch.optim.AdamW([dict(params=[p], **h) for p, (_, h) in zip(params, edges)], foreach=False)
    if t0:
        ref.load(m, v, t)
        opt.load_state_dict(oc.torch_state_dict(groups, [x.to(dtype) for x in m], [x.to(dtype) for x in v], t))
    return opt, params, ref, g0, mgn, (m, v)


def _all_nan_edges(t0, clip):
    """With coef == 0 and zero moments the edge eps == 0 divides 0 by 0: p is NaN in every element, on every route."""
    return [i for i, (name, _) in enumerate(oc.edge_hypers()) if name == "eps=0.0" and t0 == 0 and clip == "zero"]


@pytest.mark.parametrize("clip", oc.CLIPS)
@pytest.mark.parametrize("t0", oc.T0S)
def test_restatement_matches_torch_float64_at_the_hyperparameter_edges(t0, clip):
    """Two steps of every edge of optim_cases.edge_hypers() (betas 0 ... 0.99999, eps 0 ... 1, lr 0 and 1, decay factors 1, 0
    and -0.5), fresh and loaded state with |m| >> |g|, clip absent, active, 0 and inf: 1e-12 as at the operating point."""
    opt, params, ref, g0, mgn, _ = _edge_setup(t0, clip, torch.float64)
    worst = 0.0
    for step in (1, 2):
        for p, g in zip(params, g0):
            p.grad = g.double()
        if mgn is not None:
            norm = torch.nn.utils.clip_grad_norm_(params, mgn)
            assert abs(float(norm) - oc.total_norm(g0)) <= 1e-12 * float(norm)
        opt.step()
        assert ref.step(g0)
        if clip == "zero":
            assert ref.coef == 0.0
        for i, p in enumerate(params):
            st = opt.state[p]
            assert int(st["step"]) == ref.t[i] == t0 + step
            if i in _all_nan_edges(t0, clip):
                assert bool(torch.isnan(p).all()) and bool(torch.isnan(ref.p[i]).all())
                assert bool((st["exp_avg"] == 0).all()) and bool((ref.m[i] == 0).all()) and bool((ref.v[i] == 0).all())
                continue
            worst = max(worst, _rel(p.detach(), ref.p[i]), _rel(st["exp_avg"], ref.m[i]), _rel(st["exp_avg_sq"], ref.v[i]))
    print(f"edges t0={t0} clip={clip}: restatement vs torch float64, worst relative distance {worst:.3e}")
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("clip", oc.CLIPS)
@pytest.mark.parametrize("t0", oc.T0S)
def test_element_f32_meets_the_kernel_bound_against_torch_float32(t0, clip):
    """adamw_element_f32 in the kernel's place: torch's float32 CPU AdamW(foreach=False) + clip_grad_norm_ is the stock
    side, the float64 restatement the reference, the bound 2 e_stock + 8 * 2^-24 * max|ref| per tensor of p, m, v -- on the
    inputs of the GPU sweep.  With the moment update in the single form m + w1 (g - m) this fails at beta1 = 0 on loaded
    state: 1.19e-7 against 2.0e-10.  (The counts of `ours` are the restatement's here; the GPU sweep passes the kernel's.)"""
    opt, params, ref, g0, mgn, (m, v) = _edge_setup(t0, clip, torch.float32)
    f32 = oc.F32Follower(ref, [p.detach() for p in params])
    if t0:
        f32.load(m, v)
    for p, g in zip(params, g0):
        p.grad = g.clone()
    if mgn is not None:
        torch.nn.utils.clip_grad_norm_(params, mgn)
    opt.step()
    assert ref.step(g0)
    f32.step(g0)
    stock = _cpu_snapshot(opt, params)
    ours = dict(f32.snapshot(), t=stock["t"])
    worst, excluded = oc.check_masked(ours, stock, ref, 1, f"t0={t0} clip={clip}")
    full = list(range(g0[0].numel()))
    assert excluded == [full if i in _all_nan_edges(t0, clip) else [] for i in range(len(g0))]
    print(f"edges t0={t0} clip={clip}: (element_f32, torch float32) distance to float64 over max|ref|: {oc.fmt(worst)}")


def test_element_f32_meets_the_kernel_bound_over_300_steps_of_inexact_scales():
    """The GPU sweep's horizon case on the CPU: the 11 tensors of test_optim_gpu._numels(), 300 steps under
    torch.amp.GradScaler("cpu") with init_scale 1000,
    growth 1.7 every 7 steps, backoff 0.3 (no scale is a power of two, every inv_scale is rounded), an inf at steps 50 and
    51, a NaN at step 200, clip active.  Scale and tracker follow Scale at every step; at steps 1, 10, 100 and 300
    adamw_element_f32 meets the kernel's bound (steps taken) against torch's float32 CPU route: stock alone holds it up
    to the last checkpoint."""
    H = oc.HORIZON
    shapes = [(n,) for n in _numels()]
    gen = torch.Generator().manual_seed(13)
    p0 = [torch.randn(s, generator=gen) for s in shapes]
    ref = AdamWRef(p0, [dict(idx=list(range(len(p0))), **oc.HYPER)], max_grad_norm=H["max_grad_norm"])
    f32 = oc.F32Follower(ref, p0)
    sched = Scale(**H["scaler"])
    params = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.AdamW(params, **oc.HYPER, foreach=False)
    scaler = torch.amp.GradScaler("cpu", **H["scaler"])
    scaler.scale(torch.zeros(()))
    taken_steps = 0
    for step in range(1, H["steps"] + 1):
        scale = float(sched.scale)
        assert math.log2(scale) != round(math.log2(scale))
        raw = oc.horizon_grads(shapes, scale, step)
        for p, g in zip(params, raw):
            p.grad = g.clone()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(params, H["max_grad_norm"])
        scaler.step(opt)
        scaler.update()
        taken = ref.step(raw, scale=scale)
        sched.update(not taken)
        assert taken == (step not in H["inf_steps"] + H["nan_steps"])
        assert float(scaler.get_scale()) == float(sched.scale), (step, float(scaler.get_scale()), float(sched.scale))
        assert int(scaler._growth_tracker.item()) == sched.tracker
        if taken:
            taken_steps += 1
            f32.step(raw)
        if step in H["checkpoints"]:
            stock = _cpu_snapshot(opt, params)
            worst, excluded = oc.check_masked(dict(f32.snapshot(), t=stock["t"]), stock, ref, taken_steps, f"step={step}")
            assert not any(excluded)
            print(f"horizon step {step} ({taken_steps} taken): (element_f32, torch float32) over max|ref|: {oc.fmt(worst)}")
    assert taken_steps == 297 and ref.t == [297.0] * len(p0)


def test_clip_coefficient_and_step_count_are_total():
    """norm + norm_eps == 0 gives inf or NaN instead of raising; the clamp is torch.clamp(max=1)'s; counts follow float32."""
    inf, nan = float("inf"), float("nan")
    for mgn, total, eps, want in ((None, 3.0, 0.0, 1.0), (1.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, nan), (0.0, 2.0, 1e-6, 0.0),
                                  (inf, 2.0, 1e-6, 1.0), (inf, inf, 1e-6, nan), (1.0, inf, 1e-6, 0.0), (1.0, nan, 1e-6, nan),
                                  (1.0, 4.0, 0.0, 0.25), (1.0, 1.0, -1.0, 1.0), (1.0, 1.0, -3.0, -0.5)):
        got = clip_coef(mgn, total, eps)
        if mgn is not None:
            t = float(torch.clamp(torch.tensor(mgn, dtype=torch.float64) / (torch.tensor(total, dtype=torch.float64) + eps), max=1.0))
            assert got == t or (got != got and t != t), (mgn, total, eps, got, t)
        assert got == want or (got != got and want != want), (mgn, total, eps, got)
    assert [next_count(t) for t in (0, 7, 2 ** 24 - 2, 2 ** 24 - 1, 2 ** 24)] == [1.0, 8.0, 2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24]
    step = torch.tensor(2.0 ** 24)
    step += 1
    assert float(step) == next_count(2 ** 24)


def test_element_f32_rounds_every_operation_on_its_own():
    """Against an exact evaluation (float64 holds every float32 product and sum of two float32 exactly enough to round
    once more): each intermediate of adamw_element_f32 is the float32 rounding of the exact operation on its float32
    operands, in both branches of the moment update."""
    rng = np.random.default_rng(5)
    f, d = np.float32, np.float64
    p, m, g_raw = (rng.standard_normal(1000).astype(f) for _ in range(3))
    v = (rng.random(1000) * 2e-3).astype(f)
    for b1 in (0.0, 0.3, 0.5, 0.9):
        hyper, t, inv, coef = dict(lr=3e-3, betas=(b1, 0.99), eps=1e-8, weight_decay=1e-2), 8.0, 1.0 / 3.0, 0.37
        got = adamw_element_f32(p, m, v, g_raw, inv, coef, hyper, t)
        r = lambda x: np.asarray(x, dtype=d).astype(f)                      # one rounding to float32
        w1, w2 = f(1.0 - b1), f(1.0 - 0.99)
        g = r(d(r(d(g_raw) * d(f(inv)))) * d(f(coef)))
        pd = r(d(p) * d(f(1.0 - 3e-3 * 1e-2)))
        diff = r(d(g) - d(m))
        if w1 < 0.5:
            m1 = r(d(m) + d(r(d(w1) * d(diff))))
        else:
            m1 = r(d(g) - d(r(d(diff) * d(r(d(1.0) - d(w1))))))
        v1 = r(d(r(d(v) * d(f(0.99)))) + d(r(d(r(d(w2) * d(g))) * d(g))))
        den = r(d(r(d(np.sqrt(v1)) / d(f(math.sqrt(1.0 - 0.99 ** t))))) + d(f(1e-8)))
        p1 = r(d(pd) - d(r(d(f(3e-3 / (1.0 - b1 ** t))) * d(r(d(m1) / d(den))))))
        assert np.array_equal(got[1], m1) and np.array_equal(got[2], v1) and np.array_equal(got[0], p1), b1
        if b1 == 0.0:
            assert np.array_equal(got[1], g)                                 # torch.lerp's upper branch: weight 1 returns g


def test_inv_scale_is_the_float64_reciprocal_rounded_once():
    for s in (1024.0, 3.0, 65536.0, 0.1):
        want = float(torch.tensor(s, dtype=torch.float32).double().reciprocal().float())
        assert inv_scale32(s) == want


def test_rejections_without_a_gpu():
    from attwarp_amd import optim
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(ValueError, match="tensor lr"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4))], lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match="amsgrad"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4))], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4))], maximize=True)
    with pytest.raises(ValueError, match="global"):
        optim.AdamW([dict(params=[torch.nn.Parameter(torch.zeros(4))], max_grad_norm=1.0),
                     dict(params=[torch.nn.Parameter(torch.zeros(4))], max_grad_norm=2.0)])
    assert optim.AdamW._step_supports_amp_scaling is True


def test_workspace_bytes_follow_the_chunk():
    """The Python CHUNK is the library's: one more chunk costs one more float64 partial, one more tensor a partial and a
    64-byte record."""
    from attwarp_amd import _lib, optim
    lib = _lib.load()
    wb = lib.attwarp_adamw_workspace_bytes
    assert wb(optim.CHUNK, 1) - wb(optim.CHUNK - 1, 1) == 8
    assert wb(2 * optim.CHUNK - 1, 1) == wb(optim.CHUNK, 1)
    assert wb(optim.CHUNK, 2) - wb(optim.CHUNK, 1) == 8 + 64
    assert wb(0, 0) == 32 and wb(-1, 1) == 0
    assert ctypes.sizeof(_lib.AdamWTensor) == 88


def test_step_call_rejects_bad_arguments_on_the_host():
    """attwarp_adamw_step validates before it launches: no GPU is touched by these calls."""
    from attwarp_amd import _lib
    lib = _lib.load()
    desc = (_lib.AdamWTensor * 1)()
    one = ctypes.c_void_p(64)
    args = lambda ws_bytes: (ctypes.cast(desc, ctypes.c_void_p), 1, 1.0, 1e-6, None, None, one, one, one, ws_bytes, None)
    assert lib.attwarp_adamw_step(*args(4096)) == -1 and b"null pointer" in lib.attwarp_last_error()
    desc[0].p = desc[0].g = desc[0].m = desc[0].v = 64
    desc[0].numel, desc[0].beta1, desc[0].beta2 = 5000, 0.9, 0.999
    assert lib.attwarp_adamw_step(*args(32 + 8 + 64)) == -1 and b"workspace" in lib.attwarp_last_error()
    desc[0].g = 66
    assert lib.attwarp_adamw_step(*args(4096)) == -1 and b"4-byte aligned" in lib.attwarp_last_error()
    desc[0].g, desc[0].beta1 = 64, 1.0
    assert lib.attwarp_adamw_step(*args(4096)) == -1 and b"betas" in lib.attwarp_last_error()
