"""float64 torch-CPU restatement of the trainer's optimiser tail (reference MN/trainer.py:259-264 with torch.optim.AdamW):
GradScaler unscale, clip_grad_norm_, AdamW with decoupled weight decay, the skipped step and the scale schedule of
torch._amp_update_scale_.  The skip and the schedule are written from their definition, not by calling torch's.
tests/test_optim_cpu.py pins it against the real torch classes on float64 parameters."""
import math

import numpy as np
import torch


def inv_scale32(scale):
    """GradScaler.unscale_: the reciprocal is taken in float64 and rounded to float32."""
    return float(np.float32(1.0 / np.float64(np.float32(scale))))


class Scale:
    """The scale and growth tracker of torch.amp.GradScaler (float32 scale, integer tracker)."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.scale = np.float32(init_scale)
        self.tracker = 0
        self.growth, self.backoff, self.interval = np.float32(growth_factor), np.float32(backoff_factor), growth_interval

    def update(self, found_inf):
        if found_inf:
            self.scale = np.float32(self.scale * self.backoff)
            self.tracker = 0
            return
        self.tracker += 1
        if self.tracker == self.interval:
            grown = np.float32(self.scale * self.growth)
            if np.isfinite(grown):
                self.scale = grown
            self.tracker = 0


class AdamWRef:
    """State of one optimiser: per tensor p, m, v (float64 tensors) and an integer step count t.

    groups: list of dicts {"idx": [tensor indices], "lr", "betas", "eps", "weight_decay"}."""

    def __init__(self, params, groups, max_grad_norm=None, norm_eps=1e-6):
        self.p = [torch.as_tensor(p).detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.groups, self.max_grad_norm, self.norm_eps = groups, max_grad_norm, norm_eps
        self.grad_norm = 0.0

    def load(self, m, v, t):
        self.m = [torch.as_tensor(x).detach().double().clone() for x in m]
        self.v = [torch.as_tensor(x).detach().double().clone() for x in v]
        self.t = [int(x) for x in t]

    def step(self, grads, scale=None):
        """grads: per tensor the RAW (scaled) gradient or None.  scale: the GradScaler's scale or None.  Returns True
        when the step was taken; under a scale a non-finite gradient skips it (p, m, v, t untouched)."""
        inv = 1.0 if scale is None else inv_scale32(scale)
        g = [None if x is None else torch.as_tensor(x).detach().double() * inv for x in grads]
        present = [x for x in g if x is not None]
        total = math.sqrt(sum(float((x * x).sum()) for x in present)) if present else 0.0
        self.grad_norm = total
        if scale is not None and not all(bool(torch.isfinite(x).all()) for x in present):
            return False
        coef = 1.0
        if self.max_grad_norm is not None:
            coef = min(self.max_grad_norm / (total + self.norm_eps), 1.0)
        for grp in self.groups:
            lr, (b1, b2), eps, wd = grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"]
            for i in grp["idx"]:
                if g[i] is None:
                    continue
                gi = g[i] * coef
                self.t[i] += 1
                t = self.t[i]
                self.p[i] = self.p[i] * (1.0 - lr * wd)
                self.m[i] = self.m[i] + (1.0 - b1) * (gi - self.m[i])
                self.v[i] = b2 * self.v[i] + (1.0 - b2) * gi * gi
                denom = self.v[i].sqrt() / math.sqrt(1.0 - b2 ** t) + eps
                self.p[i] = self.p[i] - lr / (1.0 - b1 ** t) * self.m[i] / denom
        return True
