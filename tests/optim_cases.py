"""Inputs and comparisons shared by the CPU pins (tests/test_optim_cpu.py) and the GPU sweep (tests/test_optim_sweep_gpu.py)
of the optimiser step, so that the GPU cases are ones a correct float32 implementation is shown to pass without a GPU."""
import numpy as np
import torch

from optim_ref import adamw_element_f32

HYPER = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
CLIPS = ["none", "active", "zero", "inf"]
T0S = [0, 7, 1000]


def edge_hypers():
    """One factor at a time around HYPER, every edge the constructor accepts; (name, hyper) in a fixed order."""
    out = []
    for b1 in (0.0, 0.3, 0.5, 0.999):
        out.append((f"beta1={b1}", dict(HYPER, betas=(b1, HYPER["betas"][1]))))
    for b2 in (0.0, 0.5, 0.99999):
        out.append((f"beta2={b2}", dict(HYPER, betas=(HYPER["betas"][0], b2))))
    for eps in (0.0, 1e-3, 1.0):
        out.append((f"eps={eps}", dict(HYPER, eps=eps)))
    for lr in (0.0, 1.0):
        out.append((f"lr={lr}", dict(HYPER, lr=lr)))
    for k in (0.0, 1.0, 1.5):                               # the decay factor 1 - lr * wd: 1, exactly 0, -0.5
        wd = k / HYPER["lr"]
        assert 1.0 - HYPER["lr"] * wd == 1.0 - k
        out.append((f"lr*wd={k}", dict(HYPER, weight_decay=wd)))
    out.append(("beta1=0,beta2=0", dict(HYPER, betas=(0.0, 0.0))))
    return out


def edge_inputs(n, t0):
    """Per edge one tensor of n elements: p ~ 1, |g| ~ 1e-4 and, for t0 > 0, loaded state with |m| ~ 1 >> |g| and v in
    [1e-5, 2e-3].  Returns p, g, m, v (lists of float32 tensors; m and v zero for t0 == 0) and the counts."""
    k = len(edge_hypers())
    gen = torch.Generator().manual_seed(700 + t0)
    p = [torch.randn(n, generator=gen) for _ in range(k)]
    g = [torch.randn(n, generator=gen) * 1e-4 for _ in range(k)]
    if t0:
        m = [torch.randn(n, generator=gen) for _ in range(k)]
        v = [torch.rand(n, generator=gen) * (2e-3 - 1e-5) + 1e-5 for _ in range(k)]
    else:
        m, v = [torch.zeros(n) for _ in range(k)], [torch.zeros(n) for _ in range(k)]
    return p, g, m, v, [t0] * k


def clip_value(clip, total):
    return {"none": None, "active": 0.25 * total, "zero": 0.0, "inf": float("inf")}[clip]


def total_norm(grads):
    return float(torch.cat([g.double().reshape(-1) for g in grads if g is not None]).norm())


def torch_state_dict(groups, m, v, t):
    """A torch.optim.AdamW state dict of several param groups.  groups: [{"idx": [...], lr, betas, eps, weight_decay}]."""
    base = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                decoupled_weight_decay=True)
    pgs = []
    for grp in groups:
        pg = dict(base, **{k: x for k, x in grp.items() if k != "idx"})
        pg["params"] = list(grp["idx"])
        pgs.append(pg)
    n = sum(len(grp["idx"]) for grp in groups)
    return {"state": {i: {"step": torch.tensor(float(t[i])), "exp_avg": m[i].clone(), "exp_avg_sq": v[i].clone()}
                      for i in range(n)}, "param_groups": pgs}


class F32Follower:
    """adamw_element_f32 over the tensors of an AdamWRef: call step() right after ref.step() took the same gradients; the
    counts, inv_scale and the float64 clip coefficient of the step are the restatement's."""

    def __init__(self, ref, params):
        self.ref = ref
        self.p = [np.array(torch.as_tensor(x).detach().float().cpu().numpy().reshape(-1)) for x in params]
        self.m = [np.zeros_like(x) for x in self.p]
        self.v = [np.zeros_like(x) for x in self.p]

    def load(self, m, v):
        self.m = [np.array(x.detach().float().cpu().numpy().reshape(-1)) for x in m]
        self.v = [np.array(x.detach().float().cpu().numpy().reshape(-1)) for x in v]

    def step(self, grads):
        for grp in self.ref.groups:
            for i in grp["idx"]:
                if grads[i] is None:
                    continue
                g = grads[i].detach().float().cpu().numpy().reshape(-1)
                self.p[i], self.m[i], self.v[i] = adamw_element_f32(self.p[i], self.m[i], self.v[i], g, self.ref.inv_scale,
                                                                    self.ref.coef, grp, self.ref.t[i])

    def snapshot(self):
        return {k: [torch.from_numpy(x).double() for x in getattr(self, k)] for k in "pmv"}


# ---- comparisons -------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24


def pattern(x):
    """0 where x is finite, +1 / -1 at +inf / -inf, 2 at NaN."""
    x = x.reshape(-1)
    out = torch.zeros(x.numel(), dtype=torch.int8)
    out[torch.isposinf(x)], out[torch.isneginf(x)], out[torch.isnan(x)] = 1, -1, 2
    return out


def check_masked(ours, stock, ref, steps, what="", f32=None):
    """The bound of tests/test_optim_gpu.py, e_kernel <= 2 e_stock + 8 * 2^-24 * max|ref| * steps per tensor of p, m, v,
    with non-finite entries handled explicitly (max() over a NaN would fail every comparison, a masked NaN none): the
    non-finite pattern of `ours` must EQUAL stock's (and that of the float32 restatement `f32` where given) in p, m and v;
    an element that is non-finite in any of the three on the stock side is left out of all three distances.  `steps` is
    the number of steps taken, or a list with one number per tensor.  Returns the
    worst (kernel, stock) distances over max|ref| and, per tensor, the indices left out -- taken from stock, never from
    `ours`."""
    assert ours["t"] == stock["t"] == list(ref.t), (what, ours["t"], stock["t"], ref.t)
    worst, excluded = {}, []
    for i in range(len(ref.p)):
        bad = torch.zeros(ref.p[i].numel(), dtype=torch.bool)
        for name in "pmv":
            want = pattern(stock[name][i])
            got = pattern(ours[name][i])
            assert torch.equal(got, want), (f"{what} {name}[{i}]: non-finite pattern differs from stock's at "
                                            f"{torch.nonzero(got != want).flatten()[:8].tolist()}")
            if f32 is not None:
                assert torch.equal(pattern(f32[name][i]), want), f"{what} {name}[{i}]: float32 restatement's pattern differs"
            bad |= want != 0
        excluded.append(torch.nonzero(bad).flatten().tolist())
        keep = ~bad
        if not bool(keep.any()):
            continue
        for name, r_all in (("p", ref.p), ("m", ref.m), ("v", ref.v)):
            r = r_all[i].reshape(-1)[keep]
            assert bool(torch.isfinite(r).all()), f"{what} {name}[{i}]: the float64 restatement is non-finite where stock is finite"
            e_k = float((ours[name][i].reshape(-1)[keep] - r).abs().max())
            e_s = float((stock[name][i].reshape(-1)[keep] - r).abs().max())
            mag = float(r.abs().max())
            taken = steps[i] if isinstance(steps, (list, tuple)) else steps
            bound = 2.0 * e_s + 8.0 * EPS32 * mag * max(taken, 1)
            assert e_k <= bound, f"{what} {name}[{i}] numel {r.numel()}: kernel {e_k:.3e} stock {e_s:.3e} bound {bound:.3e}"
            w = worst.setdefault(name, [0.0, 0.0])
            w[0], w[1] = max(w[0], e_k / max(mag, 1e-300)), max(w[1], e_s / max(mag, 1e-300))
    return worst, excluded


def same_bits(a, b):
    """float32 bit equality of two tensors (given as float32 or as float64 copies of float32); NaN equals NaN."""
    a, b = a.reshape(-1).float(), b.reshape(-1).float()
    nan = torch.isnan(a) & torch.isnan(b)
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | nan).all())


def fmt(worst):
    return ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in worst.items())


# ---- the 300-step run under a GradScaler whose scales are no powers of two ------------------------------------------------
HORIZON = dict(steps=300, checkpoints=(1, 10, 100, 300), inf_steps=(50, 51), nan_steps=(200,), max_grad_norm=0.3,
               scaler=dict(init_scale=1000.0, growth_factor=1.7, backoff_factor=0.3, growth_interval=7))


def horizon_grads(shapes, scale, step):
    gen = torch.Generator().manual_seed(1000 + step)
    raw = [torch.randn(s, generator=gen) * 0.05 * scale for s in shapes]
    if step in HORIZON["inf_steps"]:
        raw[-1].view(-1)[-1] = float("inf")
    if step in HORIZON["nan_steps"]:
        raw[0].view(-1)[0] = float("nan")
    return raw
