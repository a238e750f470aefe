"""The trainer's optimiser step on HIP kernels (csrc/optim.hip): GradScaler unscale, global gradient-norm clipping and
AdamW in two launches.

The reference ends every training step on stock ops (MN/trainer.py:259-264)::

    scaler.unscale_(opt)
    grad_norm = torch.nn.utils.clip_grad_norm_(net.parameters(), cfg.grad_clip)
    scaler.step(opt)
    scaler.update()

With ``opt = attwarp_amd.optim.AdamW(net.parameters(), lr=cfg.lr, weight_decay=cfg.wd, max_grad_norm=cfg.grad_clip)`` the
same update is ``scaler.step(opt); scaler.update(); grad_norm = opt.grad_norm``: the stock ``torch.amp.GradScaler`` hands
its scale and its found-inf flag over as device tensors (the ``_step_supports_amp_scaling`` protocol) and nothing
synchronises with the host.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

CHUNK = 4096          # elements a workgroup owns (csrc/optim.hip: ATTWARP_ADAMW_CHUNK)

__all__ = ["AdamW", "CHUNK"]


def _dense(t: torch.Tensor) -> bool:
    """True when the elements of `t` fill one gap-free block of memory (in any dimension order)."""
    if t.is_contiguous():
        return True
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda x: x[1]):
        if stride != expect:
            return False
        expect *= size
    return True


class AdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (decoupled weight decay, no amsgrad, no maximize) with the GradScaler unscale and
    ``clip_grad_norm_(parameters, max_grad_norm)`` folded into its step: two HIP launches per 64 tensors.

    ``g = grad * inv_scale``; ``total_norm`` = L2 norm of g over all tensors of all groups (float64 accumulation, fixed
    order: bitwise repeatable); ``coef = min(max_grad_norm / (total_norm + norm_eps), 1)`` (1 when ``max_grad_norm`` is
    None); then AdamW on ``g * coef``.  ``grad_norm`` (0-dim float32 on the device) holds ``total_norm`` of the last
    ``step()``, before clipping: the value ``clip_grad_norm_`` returns.  The first moment is ``torch.lerp(m, g, 1 - beta1)``
    in both of its forms: ``m + w (g - m)`` for ``w < 0.5`` and ``g - (g - m)(1 - w)`` from 0.5 on (``beta1 <= 0.5``).

    **Gradients are read, never written**: after ``step()`` every ``.grad`` still holds the values backward left there
    (scaled by the GradScaler, unclipped), unlike after ``scaler.unscale_`` and ``clip_grad_norm_``.

    Under ``scaler.step(opt)`` the scale and the found-inf flag are read on the device; when the flag is set, parameters,
    moments and step counts keep their bits.  ``scaler.unscale_(opt)`` may still be called first (the gradients are then
    taken as unscaled).  A plain ``opt.step()`` never skips.  Step counts are per tensor, float32, on the device; a
    parameter whose ``.grad`` is None is left out of the step.

    Only float32 parameters and dense float32 gradients on one GPU; ``amsgrad``, ``maximize`` and a tensor ``lr`` are
    rejected.  ``max_grad_norm`` and ``norm_eps`` are global: every param group must carry the same values.
    ``state_dict()`` / ``load_state_dict()`` interchange with ``torch.optim.AdamW``.
    """

    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, max_grad_norm=None,
                 norm_eps=1e-6, amsgrad=False, maximize=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("attwarp_amd.optim.AdamW: a tensor lr is not supported (pass a float)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True,
                        max_grad_norm=max_grad_norm, norm_eps=norm_eps)
        super().__init__(params, defaults)
        self._check_groups()
        flat = [p for group in self.param_groups for p in group["params"]]
        for p in flat:
            self._check_param(p)
        self._device = _lib.require_gpu(*flat)
        _lib.load()
        self._slot = {p: i for i, p in enumerate(flat)}
        total = sum(p.numel() for p in flat)
        # everything the kernels need besides the tensors, allocated once: step counts, grad_norm, the workspace
        # (partials, ticket, step and per-tensor records; zero before its first use) and the host descriptor array
        self._steps = torch.zeros(len(flat), dtype=torch.float32, device=self._device)
        self.grad_norm = torch.zeros((), dtype=torch.float32, device=self._device)
        self._ws_bytes = int(_lib.load().attwarp_adamw_workspace_bytes(total, len(flat)))
        self._ws = torch.zeros(self._ws_bytes, dtype=torch.uint8, device=self._device)
        self._desc = (_lib.AdamWTensor * max(len(flat), 1))()

    # ---- checks -------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_param(p):
        if not p.is_cuda:
            raise RuntimeError(f"attwarp_amd.optim.AdamW: parameter on {p.device}; the HIP kernels need GPU tensors "
                               "(there is no CPU fallback)")
        if p.dtype != torch.float32:
            raise TypeError(f"attwarp_amd.optim.AdamW: parameters must be float32, got {p.dtype}")
        if p.is_sparse or not _dense(p):
            raise ValueError("attwarp_amd.optim.AdamW: parameters must be dense strided tensors without gaps "
                             f"(shape {tuple(p.shape)}, strides {p.stride()})")

    def _check_groups(self):
        first = self.param_groups[0]
        for group in self.param_groups:
            if group.get("amsgrad", False):
                raise ValueError("attwarp_amd.optim.AdamW: amsgrad is not supported")
            if group.get("maximize", False):
                raise ValueError("attwarp_amd.optim.AdamW: maximize is not supported")
            if not group.get("decoupled_weight_decay", True):
                raise ValueError("attwarp_amd.optim.AdamW: only decoupled weight decay (AdamW) is supported")
            if isinstance(group["lr"], torch.Tensor):
                raise ValueError("attwarp_amd.optim.AdamW: a tensor lr is not supported (pass a float)")
            b1, b2 = group["betas"]
            if isinstance(b1, torch.Tensor) or isinstance(b2, torch.Tensor):
                raise ValueError("attwarp_amd.optim.AdamW: tensor betas are not supported (pass floats)")
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
                raise ValueError(f"attwarp_amd.optim.AdamW: betas {group['betas']} outside [0, 1)")
            if group["lr"] < 0.0 or group["eps"] < 0.0 or group["weight_decay"] < 0.0:
                raise ValueError("attwarp_amd.optim.AdamW: negative lr, eps or weight_decay")
            if group["max_grad_norm"] != first["max_grad_norm"] or group["norm_eps"] != first["norm_eps"]:
                raise ValueError("attwarp_amd.optim.AdamW: the clip is global; max_grad_norm and norm_eps must be the "
                                 "same in every param group")
        if first["max_grad_norm"] is not None and not first["max_grad_norm"] >= 0.0:
            raise ValueError(f"attwarp_amd.optim.AdamW: max_grad_norm {first['max_grad_norm']} must be None or >= 0")

    def add_param_group(self, param_group):
        if hasattr(self, "_steps"):
            raise RuntimeError("attwarp_amd.optim.AdamW: the workspace is sized at construction; pass every param "
                               "group to the constructor")
        super().add_param_group(param_group)

    # ---- state --------------------------------------------------------------------------------------------------
    def _init_state(self, p):
        st = self.state[p]
        st["step"] = self._steps[self._slot[p]]              # a 0-dim view: the kernel advances it
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def state_dict(self):
        """As torch.optim.AdamW's; the step counts are copies (the live ones are views of one device array)."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (v.clone() if n == "step" else v) for n, v in st.items()} for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Accepts a state dict of this class or of torch.optim.AdamW (``max_grad_norm`` and ``norm_eps`` then keep
        their current values)."""
        keep = [(g["max_grad_norm"], g["norm_eps"]) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, (mgn, ne) in zip(self.param_groups, keep):
            group.setdefault("max_grad_norm", mgn)
            group.setdefault("norm_eps", ne)
            group.setdefault("decoupled_weight_decay", True)
        self._check_groups()
        for p, st in self.state.items():
            if not st:
                continue
            slot = self._steps[self._slot[p]]
            slot.copy_(torch.as_tensor(st["step"], dtype=torch.float32))
            st["step"] = slot
            for name in ("exp_avg", "exp_avg_sq"):
                t = st[name]
                if t.dtype != torch.float32 or t.device != p.device or t.shape != p.shape or t.stride() != p.stride():
                    st[name] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(t)

    # ---- the step -----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        """One optimiser step.  Reads ``self.grad_scale`` / ``self.found_inf`` when ``GradScaler.step`` has set them
        (device tensors, never ``.item()``); leaves every ``.grad`` as it is."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale = getattr(self, "grad_scale", None)
        found_inf = getattr(self, "found_inf", None)
        for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.numel() == 1
                                      and t.device == self._device):
                raise TypeError(f"attwarp_amd.optim.AdamW: {name} must be a one-element float32 tensor on {self._device}")
        self._check_groups()
        desc, n, keep = self._desc, 0, []
        for group in self.param_groups:
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            for p in group["params"]:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                if g.is_sparse:
                    raise RuntimeError("attwarp_amd.optim.AdamW: sparse gradients are not supported")
                if g.dtype != torch.float32:
                    raise TypeError(f"attwarp_amd.optim.AdamW: gradients must be float32, got {g.dtype}")
                if g.device != self._device:
                    raise RuntimeError(f"attwarp_amd.optim.AdamW: gradient on {g.device}, parameter on {self._device}")
                if g.stride() != p.stride():
                    # e.g. a channels-last gradient of a contiguous weight: one copy into the parameter's layout
                    g = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)
                    keep.append(g)
                st = self.state[p]
                if not st:
                    st = self._init_state(p)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                if m.stride() != p.stride() or v.stride() != p.stride() or m.dtype != torch.float32 or v.dtype != torch.float32:
                    raise RuntimeError("attwarp_amd.optim.AdamW: exp_avg / exp_avg_sq must be float32 in the parameter's layout")
                d = desc[n]
                d.p, d.g, d.m, d.v = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                d.numel = p.numel()
                d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = lr, b1, b2, eps, wd
                d.step_slot = self._slot[p]
                n += 1
        if n == 0:
            self.grad_norm.zero_()
            return loss
        mgn = self.param_groups[0]["max_grad_norm"]
        with torch.cuda.device(self._device):
            _lib.call("attwarp_adamw_step", ctypes.cast(desc, ctypes.c_void_p), n, -1.0 if mgn is None else float(mgn),
                      float(self.param_groups[0]["norm_eps"]), _lib.ptr(grad_scale), _lib.ptr(found_inf),
                      _lib.ptr(self._steps), _lib.ptr(self.grad_norm), _lib.ptr(self._ws), self._ws_bytes,
                      _lib.stream_ptr(self._device))
        del keep        # stream ordered: the caching allocator reuses the copies only behind the kernels
        return loss
