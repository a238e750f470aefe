"""Drop-in for ``model/marginalnet_full_dataset/losses.py`` (reference lines 11-77), plus the trainer's image-resolution
PDF loss (``pdf_l1_loss``, MN/trainer.py:216-250) as one fused entry point.

Same names, parameter names, order and defaults as the reference.  Every function runs on HIP kernels (losses.hip,
profiles.hip): forward and backward of the losses, forward of the two target builders.  Inputs are computed in float32
(float16 / bfloat16, as seen under the trainer's ``autocast``, are upcast); loss scalars are float32 0-d tensors on the
input's device; gradients come back in each input's dtype.  CPU tensors raise (there is no CPU fallback).

Autograd: the losses are ``torch.autograd.Function``s with ``once_differentiable`` backwards on HIP, with respect to
their distribution arguments.  The attention map ``A`` of the recon losses and the GT PDFs of ``pdf_l1_loss`` are
targets: when one of them requires grad, the call takes the package's convention for such inputs (``_lib.needs_grad``)
and runs the same formula on differentiable stock ops.  ``build_axis_cdf_targets`` and ``cdf_from_density_downsample``
are forward-only kernels with that same convention.  Losses reduce to their scalar in one launch without float atomics
(bitwise repeatable); see DESIGN.md "training losses" for the tie conventions of the backwards.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib, _tables
from ._lib import call, ptr, require_gpu, stream_ptr
from .checkpoint_utils import cdf_from_density, upsample_pdf_right_inverse


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _rows(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() != 2:
        raise ValueError(f"{name} must be (B, N); got shape {tuple(t.shape)}")
    return _f32(t)


def _maps(A: torch.Tensor, name: str = "A") -> torch.Tensor:
    """(B,1,H,W) or (B,H,W) -> (B,H,W) float32 contiguous."""
    if A.dim() == 4 and A.shape[1] == 1:
        return _f32(A[:, 0])
    if A.dim() == 3:
        return _f32(A)
    raise ValueError(f"{name} must be (B,1,H,W); got shape {tuple(A.shape)}")


# One uint32 arrival counter per (device, stream) for the in-launch reductions of the loss forwards: the kernel leaves it
# at 0, and launches on one stream never overlap, so they can share it.
_TICKETS: dict = {}


def _ticket(dev: torch.device) -> torch.Tensor:
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS.setdefault(key, torch.zeros(1, dtype=torch.int32, device=dev))
    return t


def _loss(name: str, dev: torch.device, nparts: int, *args) -> torch.Tensor:
    """Run a loss forward entry point: (args..., parts, ticket, loss, stream) -> float32 0-d tensor."""
    parts = torch.empty(nparts, device=dev, dtype=torch.float64)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        call(name, *args, ptr(parts), ptr(_ticket(dev)), ptr(loss), stream_ptr(dev))
    return loss


def _grad_scalar(g: torch.Tensor) -> torch.Tensor:
    return g.detach().to(torch.float32).reshape(()).contiguous()


def _back(g: torch.Tensor, like: torch.Tensor, dtype: torch.dtype, needed: bool):
    return g.reshape(like.shape).to(dtype) if needed else None


# ---- l1_cdf_loss (reference :11-12) -------------------------------------------------------------------------------------
class _L1Cdf(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p_pred, p_gt):
        dev = require_gpu(p_pred, p_gt)
        p, q = _rows(p_pred, "p_pred"), _rows(p_gt, "p_gt")
        if p.shape != q.shape:
            raise ValueError(f"l1_cdf_loss: shapes differ: {tuple(p.shape)} vs {tuple(q.shape)}")
        B, N = p.shape
        ctx.save_for_backward(p, q)
        ctx.dtypes = (p_pred.dtype, p_gt.dtype)
        return _loss("attwarp_l1_cdf_loss", dev, B, ptr(p), ptr(q), B, N)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, q = ctx.saved_tensors
        dev = p.device
        B, N = p.shape
        gp, gq = torch.empty_like(p), torch.empty_like(q)
        gs = _grad_scalar(g)
        with torch.cuda.device(dev):
            call("attwarp_l1_cdf_loss_backward", ptr(p), ptr(q), B, N, ptr(gs), ptr(gp), ptr(gq), stream_ptr(dev))
        return _back(gp, p, ctx.dtypes[0], ctx.needs_input_grad[0]), _back(gq, q, ctx.dtypes[1], ctx.needs_input_grad[1])


def l1_cdf_loss(p_pred: torch.Tensor, p_gt: torch.Tensor) -> torch.Tensor:
    """``F.l1_loss(cdf_from_density(p_pred), cdf_from_density(p_gt))`` (reference :11-12); p (B, N)."""
    return _L1Cdf.apply(p_pred, p_gt)


# ---- sym_kl (reference :15-22) ------------------------------------------------------------------------------------------
class _SymKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p_in, q_in, eps):
        dev = require_gpu(p_in, q_in)
        p, q = _rows(p_in, "p"), _rows(q_in, "q")
        if p.shape != q.shape:
            raise ValueError(f"sym_kl: shapes differ: {tuple(p.shape)} vs {tuple(q.shape)}")
        B, N = p.shape
        ctx.save_for_backward(p, q)
        ctx.eps, ctx.dtypes = float(eps), (p_in.dtype, q_in.dtype)
        return _loss("attwarp_sym_kl", dev, B, ptr(p), ptr(q), B, N, float(eps))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, q = ctx.saved_tensors
        dev = p.device
        B, N = p.shape
        gp, gq = torch.empty_like(p), torch.empty_like(q)
        gs = _grad_scalar(g)
        with torch.cuda.device(dev):
            call("attwarp_sym_kl_backward", ptr(p), ptr(q), B, N, ctx.eps, ptr(gs), ptr(gp), ptr(gq), stream_ptr(dev))
        return (_back(gp, p, ctx.dtypes[0], ctx.needs_input_grad[0]),
                _back(gq, q, ctx.dtypes[1], ctx.needs_input_grad[1]), None)


def sym_kl(p: torch.Tensor, q: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """Symmetric KL of the eps-clamped, renormalised rows of p and q (reference :15-22); p, q (B, N)."""
    return _SymKL.apply(p, q, eps)


# ---- separable_recon_loss / recon_l1 (reference :25-47) -----------------------------------------------------------------
def _recon_stock(px, py, A, l1: bool):
    """The reference's formula on differentiable stock ops (the convention for an ``A`` that requires grad)."""
    Apos = A.clamp_min(0)
    Apos = Apos / Apos.sum(dim=(2, 3), keepdim=True).clamp_min(1e-6)
    P = torch.einsum("bh,bw->bhw", py, px)
    P = P / P.sum(dim=(1, 2), keepdim=True).clamp_min(1e-6)
    return (F.l1_loss if l1 else F.mse_loss)(P.unsqueeze(1), Apos)


class _Recon(torch.autograd.Function):
    @staticmethod
    def forward(ctx, px_in, py_in, A_in, kind):
        dev = require_gpu(px_in, py_in, A_in)
        px, py, A = _rows(px_in, "px"), _rows(py_in, "py"), _maps(A_in)
        B, H, W = A.shape
        if tuple(px.shape) != (B, W) or tuple(py.shape) != (B, H):
            raise ValueError(f"recon loss: px {tuple(px.shape)} / py {tuple(py.shape)} do not match A (B,1,H,W) = "
                             f"{tuple(A_in.shape)}")
        ctx.save_for_backward(px, py, A)
        ctx.kind, ctx.dtypes = kind, (px_in.dtype, py_in.dtype)
        return _loss("attwarp_recon_loss", dev, B, ptr(px), ptr(py), ptr(A), B, H, W, kind)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        px, py, A = ctx.saved_tensors
        dev = px.device
        B, H, W = A.shape
        gpx, gpy = torch.empty_like(px), torch.empty_like(py)
        gs = _grad_scalar(g)
        with torch.cuda.device(dev):
            call("attwarp_recon_loss_backward", ptr(px), ptr(py), ptr(A), B, H, W, ctx.kind, ptr(gs), ptr(gpx), ptr(gpy),
                 stream_ptr(dev))
        return (_back(gpx, px, ctx.dtypes[0], ctx.needs_input_grad[0]),
                _back(gpy, py, ctx.dtypes[1], ctx.needs_input_grad[1]), None, None)


def separable_recon_loss(px: torch.Tensor, py: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """MSE between the normalised outer product py px^T and the normalised A+ (reference :25-34).
    px (B,W), py (B,H), A (B,1,H,W).  The (B,H,W) product is never materialised: one pass over A."""
    require_gpu(px, py, A)
    if _lib.needs_grad(A):
        return _recon_stock(px, py, A, l1=False)
    return _Recon.apply(px, py, A, _lib.RECON_MSE)


def recon_l1(px: torch.Tensor, py: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """Mean absolute error between the normalised outer product and the normalised A+ (reference :37-47)."""
    require_gpu(px, py, A)
    if _lib.needs_grad(A):
        return _recon_stock(px, py, A, l1=True)
    return _Recon.apply(px, py, A, _lib.RECON_L1)


# ---- target builders (reference :50-77), forward only ---------------------------------------------------------------
def build_axis_cdf_targets(A: torch.Tensor, L: int = 128) -> Tuple[torch.Tensor, torch.Tensor]:
    """A (B,1,H,W) -> (Fx, Fy) (B, L) float32: axis sums of nan_to_num(A.clamp_min(0)), normalised, pooled to L,
    cumsum, renormalised, last entry 1 (reference :50-67).  One HBM pass over A, then a per-row finalise."""
    dev = require_gpu(A)
    L = int(L)
    if _lib.needs_grad(A):
        Ac = torch.nan_to_num(A.float().clamp_min(0), nan=0.0, posinf=0.0, neginf=0.0)
        return (cdf_from_density_downsample(Ac.sum(dim=2).squeeze(1), L),
                cdf_from_density_downsample(Ac.sum(dim=3).squeeze(1), L))
    x = _maps(A)
    B, H, W = x.shape
    Fx = torch.empty(B, L, device=dev, dtype=torch.float32)
    Fy = torch.empty(B, L, device=dev, dtype=torch.float32)
    ws = torch.empty(_lib.load().attwarp_axis_sums_workspace_bytes(B, H, W), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        call("attwarp_build_axis_cdf_targets", ptr(x), B, H, W, L, ptr(Fx), ptr(Fy), ptr(ws), stream_ptr(dev))
    return Fx, Fy


def cdf_from_density_downsample(p: torch.Tensor, L: int) -> torch.Tensor:
    """Densities p (B,N) -> CDF (B,L) float32 via pool(pdf) -> cumsum -> renorm (reference :70-77)."""
    dev = require_gpu(p)
    L = int(L)
    if _lib.needs_grad(p):
        q = torch.nan_to_num(p.float().clamp_min(0), nan=0.0, posinf=0.0, neginf=0.0)
        q = q / q.sum(dim=1, keepdim=True).clamp_min(1e-6)
        Fp = torch.cumsum(F.adaptive_avg_pool1d(q.unsqueeze(1), L).squeeze(1), dim=1)
        Fp = Fp / Fp[:, -1:].clamp_min(1e-6)
        return torch.cat([Fp[:, :-1], Fp.new_ones(Fp.size(0), 1)], dim=1)
    x = _rows(p, "p")
    B, N = x.shape
    out = torch.empty(B, L, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        call("attwarp_cdf_downsample", ptr(x), B, N, L, ptr(out), stream_ptr(dev))
    return out


# ---- the trainer's image-resolution PDF loss (MN/trainer.py:216-250) --------------------------------------------------
def _pdf_l1_stock(px_s, py_s, px_gt_vis, py_gt_vis, W, H, eps):
    """MN/trainer.py:216-250 on the package's differentiable ops (the convention for GT PDFs that require grad)."""
    def img(p, n):
        u = upsample_pdf_right_inverse(p, n, eps).clamp_min(0)
        return u / u.sum(dim=1, keepdim=True).clamp_min(1e-6)
    return F.l1_loss(img(px_s, W), img(px_gt_vis, W)) + F.l1_loss(img(py_s, H), img(py_gt_vis, H))


class _PdfL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, px_s, py_s, px_gt, py_gt, W, H, eps):
        dev = require_gpu(px_s, py_s, px_gt, py_gt)
        px, py = _rows(px_s, "px_s"), _rows(py_s, "py_s")
        gx, gy = _rows(px_gt, "px_gt_vis"), _rows(py_gt, "py_gt_vis")
        if gx.shape != px.shape or gy.shape != py.shape or px.shape[0] != py.shape[0]:
            raise ValueError(f"pdf_l1_loss: shapes px_s {tuple(px.shape)}, py_s {tuple(py.shape)}, px_gt_vis "
                             f"{tuple(gx.shape)}, py_gt_vis {tuple(gy.shape)} do not match")
        B, Lx = px.shape
        Ly = py.shape[1]
        # the inverse tables stay referenced by ctx until the backward has been enqueued (the device cache is FIFO)
        inv_x = _tables.right_inverse_inv(Lx, W, eps, dev)
        inv_y = _tables.right_inverse_inv(Ly, H, eps, dev)
        ctx.save_for_backward(px, py, gx, gy)
        ctx.inv, ctx.dims, ctx.dtypes = (inv_x, inv_y), (B, Lx, Ly, W, H), (px_s.dtype, py_s.dtype)
        return _loss("attwarp_pdf_l1_loss", dev, 2 * B, ptr(px), ptr(py), ptr(gx), ptr(gy), B, Lx, Ly, W, H, ptr(inv_x),
                     ptr(inv_y))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        px, py, gx, gy = ctx.saved_tensors
        dev = px.device
        B, Lx, Ly, W, H = ctx.dims
        inv_x, inv_y = ctx.inv
        gpx, gpy = torch.empty_like(px), torch.empty_like(py)
        gs = _grad_scalar(g)
        with torch.cuda.device(dev):
            call("attwarp_pdf_l1_loss_backward", ptr(px), ptr(py), ptr(gx), ptr(gy), B, Lx, Ly, W, H, ptr(inv_x),
                 ptr(inv_y), ptr(gs), ptr(gpx), ptr(gpy), stream_ptr(dev))
        return (_back(gpx, px, ctx.dtypes[0], ctx.needs_input_grad[0]),
                _back(gpy, py, ctx.dtypes[1], ctx.needs_input_grad[1]), None, None, None, None, None)


def pdf_l1_loss(px_s: torch.Tensor, py_s: torch.Tensor, px_gt_vis: torch.Tensor, py_gt_vis: torch.Tensor,
                W: int, H: int, eps: float = 1e-8) -> torch.Tensor:
    """The trainer's ``L_pdf`` (MN/trainer.py:216-250): the low-resolution PDFs (px_s, px_gt_vis (B,Lx); py_s, py_gt_vis
    (B,Ly)) are up-sampled by the right inverse to W and H (``eps``: its ridge term, as ``upsample_pdf_right_inverse``),
    clamped at 0 and renormalised with clamp_min(1e-6); returns ``l1_loss(x) + l1_loss(y)``.  One launch forward, one
    backward (gradients for px_s and py_s; the GT PDFs are targets).  An image axis shorter than its low resolution has a
    singular system once the float32 Gram matrix has lost a ridge as small as the default: building its table raises
    ``numpy.linalg.LinAlgError`` (the reference's float32 solve fails there too); with an ``eps`` that float32 keeps the
    kernels serve such lengths."""
    W, H = int(W), int(H)
    require_gpu(px_s, py_s, px_gt_vis, py_gt_vis)
    if _lib.needs_grad(px_gt_vis, py_gt_vis):
        return _pdf_l1_stock(px_s, py_s, px_gt_vis, py_gt_vis, W, H, float(eps))
    return _PdfL1.apply(px_s, py_s, px_gt_vis, py_gt_vis, W, H, float(eps))
