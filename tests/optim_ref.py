"""float64 torch-CPU restatement of the trainer's optimiser tail (reference MN/trainer.py:259-264 with torch.optim.AdamW):
GradScaler unscale, clip_grad_norm_, AdamW with decoupled weight decay, the skipped step and the scale schedule of
torch._amp_update_scale_.  The skip and the schedule are written from their definition, not by calling torch's.
adamw_element_f32 states the per-element arithmetic of DESIGN 3.11 in numpy float32, one rounding at a time.
tests/test_optim_cpu.py pins both against the real torch classes: the float64 one on float64 parameters, the float32 one
against torch's float32 CPU route with the bound of the GPU tests."""
import math

import numpy as np
import torch


def inv_scale32(scale):
    """GradScaler.unscale_: the reciprocal is taken in float64 and rounded to float32."""
    return float(np.float32(1.0 / np.float64(np.float32(scale))))


def clip_coef(max_grad_norm, total, norm_eps):
    """min(max_grad_norm / (total + norm_eps), 1) in float64 as torch.clamp(max=1) takes it: a zero divisor gives inf or
    NaN, never an exception; NaN stays NaN and +inf becomes 1.  1 when max_grad_norm is None."""
    if max_grad_norm is None:
        return 1.0
    with np.errstate(all="ignore"):
        q = np.float64(max_grad_norm) / (np.float64(total) + np.float64(norm_eps))
    return float(q) if (q < 1.0 or q != q) else 1.0


def next_count(t):
    """The step count is a float32 on both routes: 2^24 + 1 rounds back to 2^24."""
    return float(np.float32(np.float32(t) + np.float32(1.0)))


def lerp_to(m, g, w):
    """torch.lerp(m, g, w), the moment update of torch.optim.AdamW: m + w (g - m) for w < 0.5, g - (g - m)(1 - w) from
    0.5 on.  Every operation in the type of its operands."""
    d = g - m
    return m + w * d if w < 0.5 else g - d * (1 - w)


def adamw_element_f32(p, m, v, g_raw, inv_scale, coef, hyper, t):
    """DESIGN 3.11's per-element arithmetic (adamw_element of csrc/optim.hip) on float32 numpy arrays, every operation
    rounded on its own.  hyper: {"lr",
    "betas", "eps", "weight_decay"}; t: the tensor's count AFTER this step; inv_scale, coef: the step's, rounded to float32
    here like the seven constants, each computed in float64 and rounded once.  Returns the new (p, m, v)."""
    f = np.float32
    lr, (b1, b2), eps, wd = hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"]
    decay, w1, b2f, w2, epsf = f(1.0 - lr * wd), f(1.0 - b1), f(b2), f(1.0 - b2), f(eps)
    step_size, bc2_sqrt = f(lr / (1.0 - b1 ** t)), f(math.sqrt(1.0 - b2 ** t))
    p, m, v, g_raw = (np.asarray(x, dtype=f) for x in (p, m, v, g_raw))
    with np.errstate(all="ignore"):
        g = (g_raw * f(inv_scale)) * f(coef)
        p = p * decay
        m = lerp_to(m, g, w1)
        v = v * b2f + (w2 * g) * g
        denom = np.sqrt(v) / bc2_sqrt + epsf
        p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == f
    return p, m, v


class Scale:
    """The scale and growth tracker of torch.amp.GradScaler (float32 scale, integer tracker).  The factors stay float64 and
    the product is taken in float64 and rounded once, as torch._amp_update_scale_ does: with factors such as 1.7 or 0.3 a
    float32 product of float32 factors gives other scales."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.scale = np.float32(init_scale)
        self.tracker = 0
        self.growth, self.backoff, self.interval = np.float64(growth_factor), np.float64(backoff_factor), growth_interval

    def update(self, found_inf):
        if found_inf:
            self.scale = np.float32(np.float64(self.scale) * self.backoff)
            self.tracker = 0
            return
        self.tracker += 1
        if self.tracker == self.interval:
            grown = np.float32(np.float64(self.scale) * self.growth)
            if np.isfinite(grown):
                self.scale = grown
            self.tracker = 0


class AdamWRef:
    """State of one optimiser: per tensor p, m, v (float64 tensors) and a step count t (a float holding a float32 value).
    After step(): grad_norm, coef (float64, before its rounding to float32) and inv_scale of that step.

    groups: list of dicts {"idx": [tensor indices], "lr", "betas", "eps", "weight_decay"}."""

    def __init__(self, params, groups, max_grad_norm=None, norm_eps=1e-6):
        self.p = [torch.as_tensor(p).detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.groups, self.max_grad_norm, self.norm_eps = groups, max_grad_norm, norm_eps
        self.grad_norm, self.coef, self.inv_scale = 0.0, 1.0, 1.0

    def load(self, m, v, t):
        self.m = [torch.as_tensor(x).detach().double().clone() for x in m]
        self.v = [torch.as_tensor(x).detach().double().clone() for x in v]
        self.t = [float(np.float32(x)) for x in t]

    def step(self, grads, scale=None):
        """grads: per tensor the RAW (scaled) gradient or None.  scale: the GradScaler's scale or None.  Returns True
        when the step was taken; under a scale a non-finite gradient skips it (p, m, v, t untouched)."""
        inv = 1.0 if scale is None else inv_scale32(scale)
        g = [None if x is None else torch.as_tensor(x).detach().double() * inv for x in grads]
        present = [x for x in g if x is not None]
        total = math.sqrt(sum(float((x * x).sum()) for x in present)) if present else 0.0
        self.grad_norm, self.inv_scale = total, inv
        if scale is not None and not all(bool(torch.isfinite(x).all()) for x in present):
            return False
        coef = self.coef = clip_coef(self.max_grad_norm, total, self.norm_eps)
        for grp in self.groups:
            lr, (b1, b2), eps, wd = grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"]
            for i in grp["idx"]:
                if g[i] is None:
                    continue
                gi = g[i] * coef
                t = self.t[i] = next_count(self.t[i])
                self.p[i] = self.p[i] * (1.0 - lr * wd)
                self.m[i] = lerp_to(self.m[i], gi, 1.0 - b1)
                self.v[i] = b2 * self.v[i] + (1.0 - b2) * gi * gi
                denom = self.v[i].sqrt() / math.sqrt(1.0 - b2 ** t) + eps
                self.p[i] = self.p[i] - lr / (1.0 - b1 ** t) * self.m[i] / denom
        return True
