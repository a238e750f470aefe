"""Drop-in for ``model/marginalnet_full_dataset/model.py``.

``safe_softmax`` (reference :8-14) is the "row/col marginal softmax" of the hot path and runs as a
HIP kernel.  ``MarginalNet`` (:17-95) is the producer of the path's input in the end-to-end
configuration ("next" row 1): its dense convolutions and linear layers are MFMA-class
library work and run on stock PyTorch-ROCm ops, the memory-bound tail between them (masked text-token
mean, FiLM + the two axis means) on HIP kernels that read each tensor once.  The tail is the same in
training: ``film_axis_means`` and ``safe_softmax`` are autograd Functions with HIP backwards
(``once_differentiable``), so the trainer's ``net(...)`` runs no stock op but the library GEMMs and,
when the feature map is resized, the bilinear interpolation.  ``forward(..., stock=True)``
runs the whole network on stock ops instead (the baseline of the tests and tools).  Parameter names are the
reference's, so checkpoints saved by the reference trainer (``{"model": state_dict}``,
MN/trainer.py:660-683) load unchanged.
Its weights are the payload of the one RCCL broadcast of the multi-GPU path (``attwarp_amd.dist``).
``mix_with_uniform`` and ``entropy`` (reference :98-106), the two helpers of the trainer's step, run forward and
backward on the row kernels of ``attwarp_amd.losses``.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import call, ptr, require_gpu, stream_ptr


_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
SOFTMAX_BACKWARD_MAX_N = 4096           # attwarp_safe_softmax_backward: 3N floats of LDS per row
FILM_MAX_TILE = 4096                    # film_axis_means kernels: H*(W+1) floats of LDS per plane


def safe_softmax_stock(logits: torch.Tensor, dim: int = 1, eps: float = 1e-6) -> torch.Tensor:
    """The reference's formula (model.py:8-14) on differentiable stock ops, any device: the baseline route, and the
    training route for rows longer than ``SOFTMAX_BACKWARD_MAX_N`` or dtypes the kernels do not take."""
    z = torch.nan_to_num(logits, nan=0.0, posinf=0.0, neginf=0.0)
    p = torch.nan_to_num(F.softmax(z - z.amax(dim=dim, keepdim=True), dim=dim), nan=0.0, posinf=0.0, neginf=0.0)
    return p / p.sum(dim=dim, keepdim=True).clamp_min(eps)


def _softmax_rows(x: torch.Tensor, d: int) -> torch.Tensor:
    """float32 [rows, N] view of ``x`` with the softmax dim ``d`` last."""
    x = x.detach().to(torch.float32)
    if d != x.dim() - 1:
        x = x.movedim(d, -1)
    return x.contiguous().reshape(-1, x.shape[-1])


def _safe_softmax_kernel(x2: torch.Tensor, eps: float, dev: torch.device) -> torch.Tensor:
    out = torch.empty_like(x2)
    with torch.cuda.device(dev):
        call("attwarp_safe_softmax", ptr(x2), x2.shape[0], x2.shape[1], float(eps), ptr(out), stream_ptr(dev))
    return out


def _from_rows(out: torch.Tensor, like: torch.Tensor, d: int) -> torch.Tensor:
    shape = list(like.shape)
    shape.append(shape.pop(d))
    out = out.reshape(shape)
    return out.movedim(-1, d) if d != like.dim() - 1 else out


class _SafeSoftmax(torch.autograd.Function):
    """safe_softmax with grad: forward = the attwarp_safe_softmax kernel; backward (``once_differentiable``) =
    attwarp_safe_softmax_backward, which recomputes the forward from the saved float32 logits."""

    @staticmethod
    def forward(ctx, logits, dim, eps, out_dtype):
        dev = logits.device
        d = dim % logits.dim()
        x2 = _softmax_rows(logits, d)
        out = _safe_softmax_kernel(x2, eps, dev)
        ctx.save_for_backward(x2)
        ctx.d, ctx.eps, ctx.dtype = d, float(eps), logits.dtype
        return _from_rows(out, logits, d).to(out_dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x2,) = ctx.saved_tensors
        dev = x2.device
        g2 = _softmax_rows(g, ctx.d)
        gl = torch.empty_like(x2)
        with torch.cuda.device(dev):
            call("attwarp_safe_softmax_backward", ptr(x2), ptr(g2), x2.shape[0], x2.shape[1], ctx.eps, ptr(gl),
                 stream_ptr(dev))
        return _from_rows(gl, g, ctx.d).to(ctx.dtype), None, None, None


def safe_softmax(logits: torch.Tensor, dim: int = 1, eps: float = 1e-6) -> torch.Tensor:
    """Softmax with NaN/Inf guards and re-normalisation (reference model.py:8-14).

    With grad (training) it is an autograd Function on HIP kernels, forward and backward (``once_differentiable``),
    returning the dtype the stock formula returns: float32 under ``torch.autocast`` (``F.softmax`` autocasts up),
    ``logits.dtype`` otherwise.  Rows longer than ``SOFTMAX_BACKWARD_MAX_N``, float64 logits and empty inputs take
    ``safe_softmax_stock``.  Without grad: the forward kernel, returning ``logits.dtype``."""
    dev = require_gpu(logits)
    if logits.dim() < 1:
        raise ValueError("safe_softmax expects at least one dimension")
    if _lib.needs_grad(logits):           # training
        if (logits.dtype not in _KERNEL_DTYPES or logits.numel() == 0
                or logits.shape[dim] > SOFTMAX_BACKWARD_MAX_N):
            return safe_softmax_stock(logits, dim, eps)
        out_dtype = torch.float32 if torch.is_autocast_enabled(dev.type) else logits.dtype
        return _SafeSoftmax.apply(logits, dim, float(eps), out_dtype)
    x = logits.detach().to(torch.float32)
    d = dim % x.dim()
    if d != x.dim() - 1:
        x = x.movedim(d, -1)
    shape = x.shape
    x2 = x.contiguous().reshape(-1, shape[-1])
    out = _safe_softmax_kernel(x2, eps, dev)
    out = out.reshape(shape)
    if d != logits.dim() - 1:
        out = out.movedim(-1, d)
    return out.to(logits.dtype) if logits.dtype.is_floating_point else out


def masked_token_mean(txt_tok: torch.Tensor, txt_mask: torch.Tensor) -> torch.Tensor:
    """``(txt_tok * txt_mask).sum(1) / txt_mask.sum(1).clamp_min(1)`` (reference :77-78) in one pass.
    txt_tok [B,Lt,D] float32/float16/bfloat16, txt_mask [B,Lt,1] or [B,Lt] -> [B,D] float32."""
    dev = require_gpu(txt_tok, txt_mask)
    if _lib.needs_grad(txt_tok, txt_mask):
        m = txt_mask.float().reshape(txt_tok.shape[0], txt_tok.shape[1], 1)
        return (txt_tok.float() * m).sum(dim=1) / m.sum(dim=1).clamp_min(1.0)
    tok = txt_tok.detach().contiguous()
    B, Lt, D = tok.shape
    mask = txt_mask.detach().float().reshape(B, Lt).contiguous()
    out = torch.empty(B, D, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        call("attwarp_masked_token_mean", ptr(tok), _lib.dtype_id(tok), ptr(mask), B, Lt, D, ptr(out), stream_ptr(dev))
    return out


def _film_stock(v: torch.Tensor, gamma_beta: torch.Tensor):
    gamma, beta = gamma_beta.float().chunk(2, dim=1)
    w = gamma[:, :, None, None] * v.float() + beta[:, :, None, None]
    return w.mean(dim=2), w.mean(dim=3)


class _FilmAxisMeans(torch.autograd.Function):
    """film_axis_means with grad: forward = attwarp_film_axis_means_t (v, gamma_beta read in their own dtypes),
    backward (``once_differentiable``) = attwarp_film_axis_means_backward: dv in v's dtype, dgamma_beta in
    gamma_beta's, one pass over v."""

    @staticmethod
    def forward(ctx, v, gamma_beta):
        dev = v.device
        x, gb = v.detach().contiguous(), gamma_beta.detach().contiguous()
        B, Ch, H, W = x.shape
        vx = torch.empty(B, Ch, W, device=dev, dtype=torch.float32)
        vy = torch.empty(B, Ch, H, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            call("attwarp_film_axis_means_t", ptr(x), _lib.dtype_id(x), ptr(gb), _lib.dtype_id(gb), B, Ch, H, W,
                 ptr(vx), ptr(vy), stream_ptr(dev))
        ctx.save_for_backward(x, gb)
        return vx, vy

    @staticmethod
    @once_differentiable
    def backward(ctx, gx, gy):
        x, gb = ctx.saved_tensors
        dev = x.device
        B, Ch, H, W = x.shape
        gx = gx.detach().to(torch.float32).contiguous()
        gy = gy.detach().to(torch.float32).contiguous()
        dv, dgb = torch.empty_like(x), torch.empty_like(gb)
        with torch.cuda.device(dev):
            call("attwarp_film_axis_means_backward", ptr(x), _lib.dtype_id(x), ptr(gb), _lib.dtype_id(gb), ptr(gx),
                 ptr(gy), B, Ch, H, W, ptr(dv), ptr(dgb), stream_ptr(dev))
        return dv, dgb


def film_axis_means(v: torch.Tensor, gamma_beta: torch.Tensor):
    """``v = gamma*v + beta; vx = v.mean(2); vy = v.mean(3)`` (reference :80-88) in one pass over ``v``.
    v [B,Ch,H,W] float32, gamma_beta [B,2*Ch] (``film`` output) -> (vx [B,Ch,W], vy [B,Ch,H]) float32.

    With grad (training) it is an autograd Function differentiable in both arguments, forward and backward on HIP
    (``once_differentiable``); v and gamma_beta may then be float16 / bfloat16 (autocast) and are read as they are,
    gradients come back in their dtypes.  Planes with H*(W+1) > ``FILM_MAX_TILE`` and float64 inputs take the same
    formula on stock float32 ops.  Without grad: float32 inputs on attwarp_film_axis_means (H*(W+1) <= 4096)."""
    dev = require_gpu(v, gamma_beta)
    if _lib.needs_grad(v, gamma_beta):
        B, Ch, H, W = v.shape
        if tuple(gamma_beta.shape) != (B, 2 * Ch):
            raise ValueError(f"gamma_beta must be [B, 2*Ch] = {(B, 2 * Ch)}; got {tuple(gamma_beta.shape)}")
        if (H * (W + 1) > FILM_MAX_TILE or v.numel() == 0
                or v.dtype not in _KERNEL_DTYPES or gamma_beta.dtype not in _KERNEL_DTYPES):
            return _film_stock(v, gamma_beta)
        return _FilmAxisMeans.apply(v, gamma_beta)
    x = v.detach().float().contiguous()
    gb = gamma_beta.detach().float().contiguous()
    B, Ch, H, W = x.shape
    if tuple(gb.shape) != (B, 2 * Ch):
        raise ValueError(f"gamma_beta must be [B, 2*Ch] = {(B, 2 * Ch)}; got {tuple(gb.shape)}")
    vx = torch.empty(B, Ch, W, device=dev, dtype=torch.float32)
    vy = torch.empty(B, Ch, H, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        call("attwarp_film_axis_means", ptr(x), ptr(gb), B, Ch, H, W, ptr(vx), ptr(vy), stream_ptr(dev))
    return vx, vy


class MarginalNet(nn.Module):
    """Predicts px (B,W) and py (B,H) from a visual token map and text tokens.

    Same architecture and state_dict keys as the reference (model.py:25-53): ``proj_v`` 1x1 conv ->
    SiLU -> 3x3 conv -> SiLU; ``txt_pool`` two Linear+SiLU; ``film`` Linear -> (gamma, beta);
    ``head_x`` / ``head_y`` Conv1d(k=5) -> SiLU -> Conv1d(1).
    """

    def __init__(self, d_vis_in: int, d_txt_in: int, hidden: int = 256, eps: float = 1e-6):
        super().__init__()
        self.eps = float(eps)
        self.proj_v = nn.Sequential(nn.Conv2d(d_vis_in, hidden, 1), nn.SiLU(),
                                    nn.Conv2d(hidden, hidden, 3, padding=1), nn.SiLU())
        self.txt_pool = nn.Sequential(nn.Linear(d_txt_in, hidden), nn.SiLU(), nn.Linear(hidden, hidden), nn.SiLU())
        self.film = nn.Linear(hidden, 2 * hidden)

        def head():
            return nn.Sequential(nn.Conv1d(hidden, hidden, 5, padding=2), nn.SiLU(), nn.Conv1d(hidden, 1, 1))

        self.head_x = head()
        self.head_y = head()

    def forward_logits(self, fmap_v, H: int, W: int, txt_tok, txt_mask):
        """Everything before the two softmaxes (reference :69-91); any device."""
        v = self.proj_v(fmap_v.float())
        v = F.interpolate(v, size=(H, W), mode="bilinear", align_corners=False)
        m = txt_mask.float()
        t = (txt_tok.float() * m).sum(dim=1) / m.sum(dim=1).clamp_min(1.0)
        gamma, beta = self.film(self.txt_pool(t)).chunk(2, dim=1)
        v = gamma[:, :, None, None] * v + beta[:, :, None, None]
        logit_x = self.head_x(v.mean(dim=2)).squeeze(1)
        logit_y = self.head_y(v.mean(dim=3)).squeeze(1)
        return logit_x, logit_y

    def forward_logits_fused(self, fmap_v, H: int, W: int, txt_tok, txt_mask):
        """GPU path of :meth:`forward`: the library GEMMs (convolutions, linear layers) on stock PyTorch-ROCm ops,
        the memory-bound tail around them on two HIP kernels that read each tensor once
        (``masked_token_mean``: reference :77-78; ``film_axis_means``: reference :80-88).  Differentiable: with grad
        ``film_axis_means`` has a HIP backward (``masked_token_mean`` has none; :meth:`forward` keeps text inputs that
        require grad off this path)."""
        v = self.proj_v(fmap_v.float())
        if tuple(v.shape[-2:]) != (H, W):       # same-size bilinear (align_corners=False) is the identity
            v = F.interpolate(v, size=(H, W), mode="bilinear", align_corners=False)
        t = masked_token_mean(txt_tok, txt_mask)
        vx, vy = film_axis_means(v, self.film(self.txt_pool(t)))
        return self.head_x(vx).squeeze(1), self.head_y(vy).squeeze(1)

    def forward(self, fmap_v, H: int, W: int, txt_tok, txt_mask, *, stock: bool = False):
        """px [B,W], py [B,H].  Inference and training alike: library GEMMs + the fused HIP tail + safe_softmax; with
        grad (MN/trainer.py:210-260: ``loss.backward()`` reaches the parameters) the tail's backwards are HIP kernels
        too.  ``stock=True`` runs the whole network on stock ops (``forward_logits`` + ``safe_softmax_stock``), the
        reference route the tests and tools compare against.  Training also takes that route when the text inputs
        require grad (the token mean has no HIP backward) or when a plane is larger than the tail kernels take
        (H*(W+1) > 4096)."""
        if not stock and _lib.needs_grad(fmap_v, txt_tok, txt_mask, *self.parameters()):
            require_gpu(fmap_v, txt_tok, txt_mask)
            stock = _lib.needs_grad(txt_tok, txt_mask) or H * (W + 1) > FILM_MAX_TILE
        if stock:
            lx, ly = self.forward_logits(fmap_v, H, W, txt_tok, txt_mask)
            return safe_softmax_stock(lx, dim=1, eps=self.eps), safe_softmax_stock(ly, dim=1, eps=self.eps)
        lx, ly = self.forward_logits_fused(fmap_v, H, W, txt_tok, txt_mask)
        return safe_softmax(lx, dim=1, eps=self.eps), safe_softmax(ly, dim=1, eps=self.eps)


class _MixUniform(torch.autograd.Function):
    """out = (1 - alpha) p + alpha / N, backward dp = (1 - alpha) g: both the scale-shift kernel, float32."""

    @staticmethod
    def forward(ctx, p, alpha):
        dev = require_gpu(p)
        x = p.detach().to(torch.float32).contiguous()
        c1 = 1.0 - alpha                     # both constants reach the kernel rounded to float32, as torch's scalars
        out = torch.empty_like(x)
        with torch.cuda.device(dev):
            call("attwarp_scale_shift", ptr(x), x.numel(), c1, alpha / p.size(1), ptr(out), stream_ptr(dev))
        ctx.c1, ctx.dtype = c1, p.dtype
        return out.to(p.dtype) if p.dtype.is_floating_point else out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        dev = g.device
        x = g.detach().to(torch.float32).contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(dev):
            call("attwarp_scale_shift", ptr(x), x.numel(), ctx.c1, 0.0, ptr(out), stream_ptr(dev))
        return out.to(ctx.dtype), None


def mix_with_uniform(p: torch.Tensor, alpha: float) -> torch.Tensor:
    """``(1 - alpha) * p + alpha / p.size(1)`` (reference model.py:98-101); returns ``p`` itself when alpha <= 0."""
    if alpha <= 0:
        return p
    return _MixUniform.apply(p, float(alpha))


class _Entropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, eps):
        from .losses import _loss, _rows
        dev = require_gpu(p)
        x = _rows(p, "p")
        B, N = x.shape
        ctx.save_for_backward(x)
        ctx.eps, ctx.dtype = float(eps), p.dtype
        return _loss("attwarp_entropy", dev, B, ptr(x), B, N, float(eps))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dev = x.device
        B, N = x.shape
        gs = g.detach().to(torch.float32).reshape(()).contiguous()
        gp = torch.empty_like(x)
        with torch.cuda.device(dev):
            call("attwarp_entropy_backward", ptr(x), B, N, ctx.eps, ptr(gs), ptr(gp), stream_ptr(dev))
        return gp.to(ctx.dtype), None


def entropy(p: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """``-(q * q.log()).sum(dim=1).mean()`` with q = p.clamp_min(eps) (reference model.py:104-106); p (B, N) -> float32
    scalar.  Forward and backward on HIP (gradient 0 where p < eps)."""
    return _Entropy.apply(p, eps)


def load_reference_checkpoint(net: MarginalNet, path_or_dict) -> MarginalNet:
    """Load a checkpoint written by the reference trainer (``torch.save({"epoch","model","opt","cfg"})``,
    MN/trainer.py:660-683) or a bare state_dict."""
    sd = torch.load(path_or_dict, map_location="cpu") if isinstance(path_or_dict, (str, bytes)) else path_or_dict
    if isinstance(sd, dict) and "model" in sd and not any(k.startswith("proj_v") for k in sd):
        sd = sd["model"]
    net.load_state_dict(sd)
    return net
