"""GPU sweep of attwarp_amd.optim.AdamW (csrc/optim.hip) away from its operating point: hyperparameter edges, per-tensor
counts and slots across launch groups, value edges on a plain step, and 300 steps under a GradScaler whose scales are no
powers of two.  tests/test_optim_gpu.py covers sizes, alignment, streams and the stock scaler at the operating point.

Tolerance: that module's, unchanged.  Per tensor of p, m, v, with stock float32 (clip_grad_norm_ + torch.optim.AdamW) run
on the same GPU from the same inputs and e = max |x - float64 restatement|:
    e_kernel <= 2 * e_stock + 8 * 2^-24 * max|restatement| * steps taken;
grad_norm at 2^-22 relative.  Non-finite entries are compared as a pattern that must equal stock's and are left out of the
distances by what STOCK shows (optim_cases.check_masked).  Where nothing is rounded before the element (no clip or a clip
coefficient of exactly 0 or 1, no scale) p, m and v must equal optim_ref.adamw_element_f32 bit for bit.
tests/test_optim_cpu.py runs the same inputs without a GPU, adamw_element_f32 in the kernel's place and torch's float32
CPU route as stock: they are inputs a correct float32 implementation passes."""
import pytest
import torch

import optim_cases as oc
from optim_ref import AdamWRef, Scale
from test_optim_gpu import (HYPER, _check_norm, _loaded_state, _numels, _optim, _ours_step, _params, _randn, _snapshot,
                            _stock_step, dev)  # noqa: F401  (dev is the module's GPU fixture)

pytestmark = pytest.mark.gpu


def _assert_bits(ours, f32, what):
    """p, m, v equal the float32 restatement bit for bit."""
    want = f32.snapshot()
    for name in "mvp":
        for i, (a, b) in enumerate(zip(ours[name], want[name])):
            a, b = a.reshape(-1), b.reshape(-1)
            if not oc.same_bits(a, b):
                bad = torch.nonzero(~((a == b) | (torch.isnan(a) & torch.isnan(b)))).flatten()
                k = int(bad[0]) if bad.numel() else -1
                raise AssertionError(f"{what} {name}[{i}]: {bad.numel()} elements differ from adamw_element_f32, first at {k}: "
                                     f"{float(a[k])!r} != {float(b[k])!r}")


# ---- a, b: hyperparameter edges side by side -----------------------------------------------------------------------------
@pytest.mark.parametrize("clip", oc.CLIPS)
@pytest.mark.parametrize("t0", oc.T0S)
def test_hyperparameter_edges_side_by_side(dev, t0, clip):
    """One param group per edge of optim_cases.edge_hypers() in a single step(): beta1 0, 0.3, 0.5, 0.999; beta2 0, 0.5,
    0.99999; eps 0, 1e-3, 1; lr 0, 1; decay factor 1, 0, -0.5; betas (0, 0).  Tensors of CHUNK + 1 elements (a full vector
    chunk and a one-element tail), |g| ~ 1e-4, fresh state or loaded state with |m| ~ 1 (torch.lerp's two branches differ
    visibly there), clip absent, active, 0 (coef exactly 0: m and v only decay) and inf.  Without an active clip nothing is
    rounded before the element and p, m, v must be adamw_element_f32's bits (p included: no case has shown the device's
    float64 pow to differ from the host's in step_size or bc2_sqrt)."""
    optim = _optim()
    edges = oc.edge_hypers()
    p0, g0, m, v, t = oc.edge_inputs(optim.CHUNK + 1, t0)
    mgn = oc.clip_value(clip, oc.total_norm(g0))
    groups = [dict(idx=[i], **h) for i, (_, h) in enumerate(edges)]
    ref = AdamWRef(p0, groups, max_grad_norm=mgn)
    f32 = oc.F32Follower(ref, p0)
    po, ps = _params(p0, dev), _params(p0, dev)
    ours = optim.AdamW([dict(params=[p], **h) for p, (_, h) in zip(po, edges)], max_grad_norm=mgn)
    stock = torch.optim.AdamW([dict(params=[p], **h) for p, (_, h) in zip(ps, edges)])
    if t0:
        ref.load(m, v, t)
        f32.load(m, v)
        ours.load_state_dict(oc.torch_state_dict(groups, m, v, t))
        stock.load_state_dict(oc.torch_state_dict(groups, m, v, t))
    gd = [g.to(dev) for g in g0]
    _ours_step(ours, po, gd)
    _stock_step(stock, ps, gd, mgn)
    assert ref.step(g0)
    f32.step(g0)
    what = f"edges t0={t0} clip={clip}"
    so, ss = _snapshot(ours, po), _snapshot(stock, ps)
    for i, (name, _) in enumerate(edges[:3]):
        e_k, e_s = (float((x["m"][i] - ref.m[i]).abs().max()) for x in (so, ss))
        print(f"{what} {name}: max|m - ref| kernel {e_k:.3e} stock {e_s:.3e} (max|ref| {float(ref.m[i].abs().max()):.3e})")
    worst, excluded = oc.check_masked(so, ss, ref, 1, what, f32=f32.snapshot())
    print(f"{what}: (kernel, stock) distance to float64 over max|ref|: {oc.fmt(worst)}")
    # eps == 0 with coef == 0 and zero moments divides 0 by 0: p is NaN in every element, on every route; nothing else is
    nan_edges = [i for i, (name, _) in enumerate(edges) if name == "eps=0.0" and t0 == 0 and clip == "zero"]
    assert excluded == [list(range(optim.CHUNK + 1)) if i in nan_edges else [] for i in range(len(edges))]
    _check_norm(ours.grad_norm, ref.grad_norm)
    assert so["t"] == [t0 + 1] * len(edges)
    if clip == "zero":
        assert ref.coef == 0.0
    if clip != "active":
        assert ref.coef in (0.0, 1.0)
        _assert_bits(so, f32, what)


def test_all_zero_gradient_with_norm_eps_zero(dev):
    """norm + norm_eps == 0 under a positive max_grad_norm: coef = min(inf, 1) = 1, grad_norm is exactly 0, p only decays and
    m, v stay +0 bit for bit -- for gradients of +0 and of -0.  Stock cannot express norm_eps: it is AdamW on the gradients
    as they are."""
    optim = _optim()
    shapes = [(optim.CHUNK + 1,), (optim.CHUNK + 1,)]
    p0 = _randn(shapes, 61)
    g0 = [torch.zeros(shapes[0]), -torch.zeros(shapes[1])]
    assert bool(torch.signbit(g0[1]).all())
    ref = AdamWRef(p0, [dict(idx=[0, 1], **HYPER)], max_grad_norm=1.0, norm_eps=0.0)
    f32 = oc.F32Follower(ref, p0)
    po, ps = _params(p0, dev), _params(p0, dev)
    ours = optim.AdamW(po, **HYPER, max_grad_norm=1.0, norm_eps=0.0)
    stock = torch.optim.AdamW(ps, **HYPER)
    gd = [g.to(dev) for g in g0]
    for step in (1, 2):
        _ours_step(ours, po, gd)
        _stock_step(stock, ps, gd, None)
        assert ref.step(g0) and ref.coef == 1.0 and ref.grad_norm == 0.0
        f32.step(g0)
        so = _snapshot(ours, po)
        _, excluded = oc.check_masked(so, _snapshot(stock, ps), ref, step, f"step={step}", f32=f32.snapshot())
        assert excluded == [[], []]
        assert float(ours.grad_norm) == 0.0 and not bool(torch.signbit(ours.grad_norm))
        for p in po:
            st = ours.state[p]
            assert bool((st["exp_avg"].view(torch.int32) == 0).all()) and bool((st["exp_avg_sq"].view(torch.int32) == 0).all())
        _assert_bits(so, f32, f"step={step}")
        decay = torch.tensor(1.0 - HYPER["lr"] * HYPER["weight_decay"], dtype=torch.float64).float()
        assert all(torch.equal(p.detach().cpu(), q * decay if step == 1 else (q * decay) * decay) for p, q in zip(po, p0))


# ---- c: per-tensor counts and slots across launch groups -------------------------------------------------------------------
def test_per_tensor_counts_and_slots_across_launch_groups(dev):
    """130 tensors (three launch groups of 64, 64, 2) in three param groups whose borders (40, 100) are not the launches',
    3 * CHUNK - 5 elements at flat indices 63, 64, 127, 128 and 1 ... 7 elsewhere, a distinct loaded count per tensor out of
    {0, 1, 2, 7, 1000, 10^6, 2^24 - 2, 2^24 - 1, 2^24}.  Four steps with a changing set of None gradients: every third; all
    of 64..129 (whole launches vanish, the ticket total shrinks); all but 128; none.  A mix-up of slot, record or count
    between tensors shows in the counts (compared with stock's and the restatement's; 2^24 stays 2^24), in absent tensors
    (which keep their bits) or in p, which depends on the count through both bias corrections."""
    optim = _optim()
    C, N = optim.CHUNK, 130
    shapes = [(3 * C - 5,) if i in (63, 64, 127, 128) else (1 + i % 7,) for i in range(N)]
    counts = [0, 1, 2, 7, 1000, 10 ** 6, 2 ** 24 - 2, 2 ** 24 - 1, 2 ** 24]
    t0 = [counts[i % len(counts)] for i in range(N)]
    hypers = [HYPER, dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.0),
              dict(lr=1e-3, betas=(0.5, 0.999), eps=1e-4, weight_decay=0.1)]
    groups = [dict(idx=list(range(a, b)), **h) for (a, b), h in zip(((0, 40), (40, 100), (100, N)), hypers)]
    mgn = 0.5
    p0 = _randn(shapes, 71)
    m, v, _ = _loaded_state(shapes, 72)
    ref = AdamWRef(p0, groups, max_grad_norm=mgn)
    ref.load(m, v, t0)
    po, ps = _params(p0, dev), _params(p0, dev)
    ours = optim.AdamW([dict(params=[po[i] for i in g["idx"]], **h) for g, h in zip(groups, hypers)], max_grad_norm=mgn)
    stock = torch.optim.AdamW([dict(params=[ps[i] for i in g["idx"]], **h) for g, h in zip(groups, hypers)])
    ours.load_state_dict(oc.torch_state_dict(groups, m, v, t0))
    stock.load_state_dict(oc.torch_state_dict(groups, m, v, t0))
    assert _snapshot(ours, po)["t"] == t0
    absent_of = {1: set(range(0, N, 3)), 2: set(range(64, N)), 3: set(range(N)) - {128}, 4: set()}
    taken = [0] * N
    for step in (1, 2, 3, 4):
        absent = absent_of[step]
        g0 = [None if i in absent else g for i, g in enumerate(_randn(shapes, 80 + step, 0.05))]
        hold = {i: (po[i].detach().clone(), ours.state[po[i]]["exp_avg"].clone(), ours.state[po[i]]["exp_avg_sq"].clone(),
                    ours.state[po[i]]["step"].clone()) for i in absent}
        gd = [None if g is None else g.to(dev) for g in g0]
        _ours_step(ours, po, gd)
        _stock_step(stock, ps, gd, mgn)
        assert ref.step(g0) and ref.coef < 1.0
        taken = [k + (i not in absent) for i, k in enumerate(taken)]
        for i, (bp, bm, bv, bt) in hold.items():
            st = ours.state[po[i]]
            assert torch.equal(po[i].detach(), bp) and torch.equal(st["exp_avg"], bm) and torch.equal(st["exp_avg_sq"], bv) \
                and torch.equal(st["step"], bt), (step, i)
        so = _snapshot(ours, po)
        worst, excluded = oc.check_masked(so, _snapshot(stock, ps), ref, taken, f"step={step}")
        assert not any(excluded)
        assert so["t"] == [min(a + k, 2 ** 24) for a, k in zip(t0, taken)]
        _check_norm(ours.grad_norm, ref.grad_norm)
        print(f"counts and slots step {step}: (kernel, stock) over max|ref|: {oc.fmt(worst)}")
    assert so["t"][6] == so["t"][7] == so["t"][8] == 2 ** 24 and t0[6:9] == [2 ** 24 - 2, 2 ** 24 - 1, 2 ** 24]


# ---- d: value edges on a plain step ----------------------------------------------------------------------------------------
VALUE_CLASSES = {"denormal": 1e-40, "square_underflows": 1e-30, "float32_norm_overflows": 1e18, "v_overflows": 1e30,
                 "signed_zero": 0.0, "+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan")}


@pytest.mark.parametrize("t0", [0, 7])
@pytest.mark.parametrize("clip", [None, "active"])
@pytest.mark.parametrize("cls", list(VALUE_CLASSES))
def test_value_edges_on_a_plain_step(dev, cls, clip, t0):
    """A plain opt.step() (no scaler: nothing skips) on a tensor of CHUNK + 1 elements and one of 257, the special gradients
    at indices 0, CHUNK - 1 (vector route) and CHUNK (the tail): +-1e-40, +-1e-30, +-1e18, +-1e30 and +-0 at all three, a
    single +inf at 0, a single -inf at CHUNK - 1, a single NaN at CHUNK.  The non-finite pattern of p, m, v equals stock's
    and the restatement's, and the set left out of the distances is the injected indices where float32 must go non-finite
    (1e30: v overflows; inf; NaN) and empty otherwise; under a clip NaN makes everything NaN and inf gives grad_norm = inf,
    coef = 0, NaN at the inf element alone and a pure decay everywhere else.  Under the clip the stock side multiplies the
    gradients by float32(coef) of the restatement: clip_grad_norm_'s float32 norm overflows at 1e18."""
    optim = _optim()
    C = optim.CHUNK
    shapes = [(C + 1,), (257,)]
    p0, g0 = _randn(shapes, 91), _randn(shapes, 92, 0.05)
    val = VALUE_CLASSES[cls]
    finite_class = val == val and abs(val) != float("inf")
    injected = [0, C - 1, C] if finite_class else [{"+inf": 0, "-inf": C - 1, "nan": C}[cls]]
    for k, i in enumerate(injected):
        g0[0][i] = -val if (finite_class and k == 1) else val
    if cls == "signed_zero":
        assert bool(torch.signbit(g0[0][C - 1])) and not bool(torch.signbit(g0[0][0]))
    mgn = None if clip is None else (0.25 * oc.total_norm(g0) if finite_class else 0.3)
    ref = AdamWRef(p0, [dict(idx=[0, 1], **HYPER)], max_grad_norm=mgn)
    f32 = oc.F32Follower(ref, p0)
    po, ps = _params(p0, dev), _params(p0, dev)
    ours, stock = optim.AdamW(po, **HYPER, max_grad_norm=mgn), torch.optim.AdamW(ps, **HYPER)
    if t0:
        m, v, t = _loaded_state(shapes, 93, t0)
        ref.load(m, v, t)
        f32.load(m, v)
        ours.load_state_dict(oc.torch_state_dict(ref.groups, m, v, t))
        stock.load_state_dict(oc.torch_state_dict(ref.groups, m, v, t))
    assert ref.step(g0)
    f32.step(g0)
    gd = [g.to(dev) for g in g0]
    _ours_step(ours, po, gd)
    coef32 = torch.tensor(ref.coef, dtype=torch.float64).float().to(dev)
    _stock_step(stock, ps, gd if clip is None else [g * coef32 for g in gd], None)
    what = f"{cls} clip={clip} t0={t0}"
    so = _snapshot(ours, po)
    worst, excluded = oc.check_masked(so, _snapshot(stock, ps), ref, 1, what, f32=f32.snapshot())
    print(f"value edge {what}: (kernel, stock) over max|ref| on the finite elements: {oc.fmt(worst)}")
    if cls == "nan" and clip is not None:
        assert excluded == [list(range(C + 1)), list(range(257))]
        assert ref.coef != ref.coef and bool(torch.isnan(ours.grad_norm))
    elif cls in ("v_overflows", "+inf", "-inf", "nan"):
        assert excluded == [injected, []]
    else:
        assert excluded == [[], []]
    if cls in ("+inf", "-inf"):
        assert float(ours.grad_norm) == float("inf") == ref.grad_norm
        if clip is not None:
            assert ref.coef == 0.0
            assert all(bool(torch.isnan(so[k][0][injected[0]])) for k in "pmv")
    elif cls == "nan":
        assert bool(torch.isnan(ours.grad_norm)) and ref.grad_norm != ref.grad_norm
    else:
        _check_norm(ours.grad_norm, ref.grad_norm)
    if clip is None or cls in ("+inf", "-inf"):
        assert ref.coef in (0.0, 1.0)                       # nothing is rounded before the element
        _assert_bits(so, f32, what)


# ---- e: horizon and inexact scales -----------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_300_steps_under_a_gradscaler_of_inexact_scales(dev):
    """The 11 tensors of test_optim_gpu._numels(), 300 steps under the stock GradScaler with init_scale 1000, growth 1.7 every
    7 steps, backoff 0.3: no scale is a power of two and every inv_scale is rounded.  An inf at steps 50 and 51, a NaN at
    step 200 (skipped: bits kept), clip active.  Scale and tracker follow optim_ref.Scale and the stock route at every step;
    at steps 1, 10, 100 and 300 p, m, v meet the bound with the steps taken.  tests/test_optim_cpu.py runs the same 300
    steps on the CPU with adamw_element_f32 in the kernel's place: the bound holds there to the last checkpoint."""
    optim = _optim()
    H = oc.HORIZON
    shapes = [(n,) for n in _numels()]
    p0 = _randn(shapes, 13)
    ref = AdamWRef(p0, [dict(idx=list(range(len(p0))), **HYPER)], max_grad_norm=H["max_grad_norm"])
    sched = Scale(**H["scaler"])
    po, ps = _params(p0, dev), _params(p0, dev)
    ours, stock = optim.AdamW(po, **HYPER, max_grad_norm=H["max_grad_norm"]), torch.optim.AdamW(ps, **HYPER)
    sc_o, sc_s = torch.amp.GradScaler("cuda", **H["scaler"]), torch.amp.GradScaler("cuda", **H["scaler"])
    sc_o.scale(torch.zeros((), device=dev)), sc_s.scale(torch.zeros((), device=dev))
    taken_steps = 0
    for step in range(1, H["steps"] + 1):
        scale = float(sched.scale)
        raw = oc.horizon_grads(shapes, scale, step)
        skipping = step in H["inf_steps"] + H["nan_steps"]
        if skipping:
            bits = [(p.detach().clone(), ours.state[p]["exp_avg"].clone(), ours.state[p]["exp_avg_sq"].clone(),
                     ours.state[p]["step"].clone()) for p in po]
        for p, g in zip(po, raw):
            p.grad = g.to(dev)
        sc_o.step(ours)
        sc_o.update()
        for p, g in zip(ps, raw):
            p.grad = g.to(dev)
        sc_s.unscale_(stock)
        torch.nn.utils.clip_grad_norm_(ps, H["max_grad_norm"])
        sc_s.step(stock)
        sc_s.update()
        taken = ref.step(raw, scale=scale)
        sched.update(not taken)
        assert taken == (not skipping)
        taken_steps += int(taken)
        if skipping:
            for p, (bp, bm, bv, bt) in zip(po, bits):
                st = ours.state[p]
                assert torch.equal(p.detach(), bp) and torch.equal(st["exp_avg"], bm) and torch.equal(st["exp_avg_sq"], bv)
                assert torch.equal(st["step"], bt)
            assert not bool(torch.isfinite(ours.grad_norm))
        so, ss = sc_o.state_dict(), sc_s.state_dict()
        assert so["scale"] == ss["scale"] == float(sched.scale), (step, so, ss, sched.scale)
        assert so["_growth_tracker"] == ss["_growth_tracker"] == sched.tracker, (step, so, ss, sched.tracker)
        if step in H["checkpoints"]:
            worst, excluded = oc.check_masked(_snapshot(ours, po), _snapshot(stock, ps), ref, taken_steps, f"step={step}")
            assert not any(excluded)
            _check_norm(ours.grad_norm, ref.grad_norm)
            print(f"horizon step {step} ({taken_steps} taken): (kernel, stock) over max|ref|: {oc.fmt(worst)}")
    assert taken_steps == 297 and list(ref.t) == [297] * len(p0)
