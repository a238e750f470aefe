"""Batched, device-resident launcher of the hot path.

The reference runs the path one image at a time on the host (``main_batched.py:243-303`` inner loop,
``checkpoint_utils.py:157`` per-sample loop, PNG files in between).  Here a whole batch stays in HBM:

``warp_from_attention_stack``  (BASELINE configs 2-4)
    captured last-query attention rows [T,B,heads,kv]
      -> A1+A2 aggregation                    (attwarp_attn_reduce_stack)
      -> A6 marginals of the 24x24 map        (attwarp_gt_marginals)
      -> A8+A9+A11 PDF -> CDF -> inverse maps (attwarp_axis_maps_from_pdf, one launch, both axes)
      -> A12 bilinear resample                (attwarp_remap_bilinear)

``warp_from_pdf``  (MarginalNet inference chain, MN/trainer.py:285-289)
``warp_from_masks``  (main_batched chain: revise_mask -> uint8 -> LANCZOS -> float64 marginals -> warp)

All launches go to the caller's current stream; no host synchronisation, so the whole step can be
captured in a HIP graph (``capture_step``).
"""
from __future__ import annotations

import ctypes
import math
import threading
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, _tables, jpeg, png
from ._batch import TABLE, _upload, _upload_filled, file_bytes, packed_views, per_kind, planned_table, uploaded      # noqa: F401 (the pool's old home)
from ._lib import call, ptr, require_gpu, stream_ptr
from . import attention_extraction as ae
from . import checkpoint_utils as cu
from . import new_method as nm

GRID = 24                             # side of the image-token grid (ae.NUM_IMAGE_TOKENS = GRID * GRID)


def adaptive_avg_pool2d(A: torch.Tensor, output_size=(GRID, GRID), sanitize: bool = False) -> torch.Tensor:
    """``F.adaptive_avg_pool2d(A, output_size)`` as the reference calls it on full-resolution attention maps
    (MN/trainer.py:197,433,465): A [B,C,H,W] or [B,H,W] float -> same rank with (H,W) replaced by ``output_size``.
    Window rows ``[floor(i*H/oh), ceil((i+1)*H/oh))``, float64 accumulation rounded once (DESIGN.md "parity").
    ``sanitize=True`` also applies the trainer's ``nan_to_num(nan=0, posinf=0, neginf=0).clamp_min(0)`` (:202)."""
    dev = require_gpu(A)
    if A.dim() not in (3, 4):
        raise ValueError(f"adaptive_avg_pool2d expects [B,C,H,W] or [B,H,W]; got {tuple(A.shape)}")
    oh, ow = (int(output_size), int(output_size)) if isinstance(output_size, int) else (int(output_size[0]), int(output_size[1]))
    x = A.detach().float().contiguous()
    H, W = x.shape[-2], x.shape[-1]
    planes = x.numel() // (H * W)
    out = torch.empty(*x.shape[:-2], oh, ow, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        call("attwarp_adaptive_avg_pool", ptr(x), planes, H, W, oh, ow, int(bool(sanitize)), ptr(out), stream_ptr(dev))
    return out


def trainer_attention_targets(A_full: torch.Tensor, transforms, grid=(GRID, GRID)
                              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The trainer's attention targets (MN/trainer.py:173-202 and :220-236) in one pass over the full-resolution map.

    A_full (B,1,H,W) float; ``transforms``: one name per sample as ``transform_for_sample`` returns them ("sqrt": the
    sqrt branch; "none": identity plus the uniform override of the GT marginals; anything else: identity).
    Returns ``(A, px_gt_vis, py_gt_vis)``: the pooled map (B,1,gh,gw) after the trainer's sanitise -- bit for bit the
    stock-op transform followed by ``adaptive_avg_pool2d(..., sanitize=True)`` -- and its ``gt_marginals`` (B,gw), (B,gh)
    with the "none" rows set to 1/L.  A NaN or +inf cell makes its window 0 (the trainer's blend turns it into NaN, the
    sanitise into 0); -inf counts as 0.  Forward only (the trainer computes it under its data path, not the graph)."""
    dev = require_gpu(A_full)
    if A_full.dim() != 4 or A_full.shape[1] != 1:
        raise ValueError(f"trainer_attention_targets expects A_full (B,1,H,W); got {tuple(A_full.shape)}")
    B, _, H, W = A_full.shape
    names = list(transforms)
    if len(names) != B:
        raise ValueError(f"trainer_attention_targets: {len(names)} transform names for a batch of {B}")
    gh, gw = (int(grid), int(grid)) if isinstance(grid, int) else (int(grid[0]), int(grid[1]))
    # pinned host memory + an asynchronous copy: the launch does not wait for the host (the caching host allocator keeps
    # the buffer until the copy has run)
    modes = torch.tensor([_lib.TT_SQRT if t == "sqrt" else _lib.TT_NONE if t == "none" else _lib.TT_IDENTITY
                          for t in names], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    x = A_full.detach().float().contiguous()
    A = torch.empty(B, 1, gh, gw, device=dev, dtype=torch.float32)
    px = torch.empty(B, gw, device=dev, dtype=torch.float32)
    py = torch.empty(B, gh, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        call("attwarp_trainer_attention_targets", ptr(x), ptr(modes), B, H, W, gh, gw, ptr(A), ptr(px), ptr(py),
             stream_ptr(dev))
    return A, px, py


def axis_maps_from_pdf(px: torch.Tensor, py: torch.Tensor, size_hw: Tuple[int, int],
                       out_size: Optional[Tuple[int, int]] = None, eps: float = 1e-8
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """px [B,n], py [B,n] low-resolution PDFs -> (map_x [B,W_out], map_y [B,H_out]).
    Equals upsample_pdf_right_inverse(.).clamp_min(0) -> cdf_from_density -> grid construction."""
    dev = require_gpu(px, py)
    H, W = int(size_hw[0]), int(size_hw[1])
    H_out, W_out = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    x, y = px.detach().float().contiguous(), py.detach().float().contiguous()
    B, n = x.shape
    inv_x = _tables.right_inverse_inv(n, W, eps, dev)
    inv_y = _tables.right_inverse_inv(n, H, eps, dev)
    mx = torch.empty(B, W_out, device=dev, dtype=torch.float32)
    my = torch.empty(B, H_out, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        call("attwarp_axis_maps_from_pdf", ptr(x), ptr(y), B, n, W, H, W_out, H_out, ptr(inv_x), ptr(inv_y), ptr(mx),
             ptr(my), stream_ptr(dev))
    return mx, my


def warp_from_pdf(images: torch.Tensor, px: torch.Tensor, py: torch.Tensor, out_size=None, channels_last=False,
                  mode: str = "cv2") -> torch.Tensor:
    """images [B,C,H,W] (or [B,H,W,C]) float32/uint8; px [B,24] over x, py [B,24] over y."""
    if channels_last:
        H, W = images.shape[1], images.shape[2]
    else:
        H, W = images.shape[2], images.shape[3]
    mx, my = axis_maps_from_pdf(px, py, (H, W), out_size)
    return cu.remap_separable(images, mx, my, mode=mode, channels_last=channels_last)


def axis_maps_from_attention_steps(steps: torch.Tensor, size_hw: Tuple[int, int],
                                   out_size: Optional[Tuple[int, int]] = None, eps: float = 1e-8,
                                   return_attention: bool = False, maps_out=None):
    """Per-step aggregated maps [T,B,g*g] in the attention dtype (output of the A1 kernel: float32 / float16 /
    bfloat16) -> (map_x, map_y) in ONE launch: mean over steps (rounded in that dtype, llava.py:409-411), marginals of the
    g x g map, PDF up-sample, CDF, inverse maps.  Bit-identical to attn_finalize -> float() -> gt_marginals ->
    axis_maps_from_pdf."""
    dev = require_gpu(steps)
    s = steps.detach().contiguous()
    if s.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError("axis_maps_from_attention_steps: float32 / float16 / bfloat16 step maps expected")
    T, B, ntok = s.shape
    g = int(round(ntok ** 0.5))
    if g * g != ntok:
        raise ValueError(f"step maps of {ntok} tokens are not a square grid")
    H, W = int(size_hw[0]), int(size_hw[1])
    H_out, W_out = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    inv_x = _tables.right_inverse_inv(g, W, eps, dev)
    inv_y = _tables.right_inverse_inv(g, H, eps, dev)
    if maps_out is None:
        mx = torch.empty(B, W_out, device=dev, dtype=torch.float32)
        my = torch.empty(B, H_out, device=dev, dtype=torch.float32)
    else:                       # caller-owned static buffers (graph replay)
        mx, my = maps_out
        if tuple(mx.shape) != (B, W_out) or tuple(my.shape) != (B, H_out) or mx.dtype != torch.float32 or my.dtype != torch.float32:
            raise ValueError("axis_maps_from_attention_steps: maps_out must be float32 [B,W_out], [B,H_out]")
        if not (mx.is_contiguous() and my.is_contiguous()) or mx.device != dev or my.device != dev:
            raise ValueError("axis_maps_from_attention_steps: maps_out must be dense tensors on the device of `steps` "
                             "(the kernel writes dense [B,W_out] / [B,H_out] rows through the raw pointers)")
    att = torch.empty(B, ntok, device=dev, dtype=torch.float32) if return_attention else None
    with torch.cuda.device(dev):
        call("attwarp_axis_maps_from_steps_t", ptr(s), _lib.dtype_id(s), T, B, g, W, H, W_out, H_out, ptr(inv_x), ptr(inv_y),
             ptr(mx), ptr(my), ptr(att), stream_ptr(dev))
    return (mx, my, att) if return_attention else (mx, my)


def attention_step_maps(rows: torch.Tensor, starts: torch.Tensor, ntok: int = ae.NUM_IMAGE_TOKENS,
                        starts_tiled: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A1 over a captured stack: rows [T,B,heads,kv] -> per-step maps [T,B,ntok] (one launch)."""
    r = rows.contiguous()
    T, B, heads, kv = r.shape
    if starts_tiled is None:
        starts_tiled = starts.repeat(T)
    steps = ae.attn_reduce_step(r.view(T * B, heads, 1, kv), starts_tiled, ntok)
    return steps.view(T, B, ntok)


def warp_from_attention_stack(images: torch.Tensor, rows: torch.Tensor, starts: torch.Tensor, out_size=None,
                              channels_last=False, mode: str = "cv2", out: Optional[torch.Tensor] = None,
                              starts_tiled: Optional[torch.Tensor] = None) -> torch.Tensor:
    """images: batch on the GPU; rows [T,B,heads,kv] last-query attention rows; starts int32 [B].
    Three launches: A1 (step maps) -> fused A2+A6+A8+A9+A11 (maps) -> A12 (warp), for attention in any of the three dtypes."""
    if channels_last:
        H, W = images.shape[1], images.shape[2]
    else:
        H, W = images.shape[2], images.shape[3]
    # any attention dtype (float32 / the model's float16 / bfloat16): A1 per step, then the fused A2 .. A11 launch
    steps = attention_step_maps(rows, starts, ae.NUM_IMAGE_TOKENS, starts_tiled)
    mx, my = axis_maps_from_attention_steps(steps, (H, W), out_size)
    return cu.remap_separable(images, mx, my, mode=mode, channels_last=channels_last, out=out)


def warp_from_masks(images_u8: torch.Tensor, attn24: torch.Tensor, out_size=(500, 500), enhance_coe=10,
                    kernel_size=3, transform="identity", exp_scale=1.0, exp_divisor=1.0, apply_inverse=False,
                    mode: str = "cv2") -> torch.Tensor:
    """The ``main_batched.py:243-287`` chain for a batch of equally sized images.
    images_u8 [B,H,W,3] uint8 (channel order is irrelevant to the warp); attn24 [B,24,24].
    -> [B,H_out,W_out,3] uint8."""
    B, H, W, _ = images_u8.shape
    rev = ae.revise_mask(attn24.float(), kernel_size=kernel_size, enhance_coe=enhance_coe)
    mota = ae.upsample_mask_lanczos(rev, (W, H))                       # uint8 [B,H,W]
    mx, my = nm.attention_axis_maps(mota, out_size[1], out_size[0], transform, exp_scale, exp_divisor, apply_inverse)
    return nm.remap_hwc(images_u8, mx, my, mode)


@torch.no_grad()
def warp_from_marginalnet(net, fmap_v: torch.Tensor, txt_tok: torch.Tensor, txt_mask: torch.Tensor,
                          images: torch.Tensor, out_size=None, channels_last=False, mode: str = "cv2"):
    """BASELINE config 5's device-resident chain: MarginalNet(hidden=256) forward (stock PyTorch-ROCm ops +
    the HIP safe_softmax) -> px, py over the 24 x 24 grid -> A8+A9+A11 (one launch) -> A12 warp.
    Mirrors the inference block of the reference trainer (MN/trainer.py:210, :285-289).
    Returns (warped images, px, py)."""
    px, py = net(fmap_v, GRID, GRID, txt_tok, txt_mask)
    return warp_from_pdf(images, px, py, out_size, channels_last, mode), px, py


OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def expand2square(images_u8: torch.Tensor, background=None) -> torch.Tensor:
    """LLaVA-1.5's ``image_aspect_ratio == "pad"`` step (``expand2square`` of the external LLaVA checkout, called by
    ``process_images``: AGW/attention_extraction/functions.py:262-271) for a uint8 [B,H,W,C] batch on the GPU: the
    images centred (offset ``(long - short) // 2``) on a square canvas of ``background`` (default
    ``int(mean * 255)`` per channel, as LLaVA passes it).  Square batches are returned as they are."""
    dev = require_gpu(images_u8)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
        raise TypeError("expand2square expects a uint8 [B,H,W,C] tensor")
    B, H, W, C = images_u8.shape
    if H == W:
        return images_u8
    if background is None:
        background = tuple(int(x * 255) for x in OPENAI_CLIP_MEAN)
    if len(background) < C:
        raise ValueError(f"background needs {C} channel values; got {len(background)}")
    n = max(H, W)
    out = torch.tensor(list(background[:C]), dtype=torch.uint8, device=dev).expand(B, n, n, C).contiguous()
    if W > H:
        o = (W - H) // 2
        out[:, o:o + H] = images_u8
    else:
        o = (H - W) // 2
        out[:, :, o:o + W] = images_u8
    return out


def clip_preprocess(images_u8: torch.Tensor, size: int = 336, dtype: torch.dtype = torch.float16,
                    mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD, pad_to_square: bool = False) -> torch.Tensor:
    """Warped uint8 RGB batch [B,H,W,3] -> CLIP-ready [B,3,size,size] on the GPU ("next" row 3).

    Replaces the PNG round trip of the reference (``cv2.imwrite`` new_method.py:491 -> ``Image.open`` +
    ``process_images`` evaluate_accuracy.py:157-158) with two launches.  Arithmetic = HF CLIPImageProcessor
    (PIL backend) as LLaVA-1.5 configures it: PIL BICUBIC resize of the shorter edge to ``size``, center crop,
    ``float32(float64(u8) * (1/255))``, ``(x - mean) / std`` in float32; ``dtype`` float32 or float16
    (LLaVA casts to float16, functions.py:270-271).  Bit-identical to the processor for float32.
    ``pad_to_square=True`` runs :func:`expand2square` first (LLaVA-1.5's ``image_aspect_ratio="pad"``; a no-op for
    the square warps of the reference drivers)."""
    dev = require_gpu(images_u8)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
        raise TypeError("clip_preprocess expects a uint8 [B,H,W,C] tensor")
    if pad_to_square:
        images_u8 = expand2square(images_u8, tuple(int(float(v) * 255) for v in mean))
    if dtype not in (torch.float32, torch.float16):
        raise TypeError("clip_preprocess: dtype must be float32 or float16")
    x = images_u8.contiguous()
    B, H, W, C = x.shape
    short, long_ = (H, W) if H <= W else (W, H)
    new_long = int(size * long_ / short)
    nh, nw = (size, new_long) if H <= W else (new_long, size)
    top, left = (nh - size) // 2, (nw - size) // 2
    bx, kx, ksx = _tables.lanczos_tables(W, nw, dev, "bicubic")
    by, ky, ksy = _tables.lanczos_tables(H, nh, dev, "bicubic")
    tmp = torch.empty(B, H, size, C, device=dev, dtype=torch.uint8)
    out = torch.empty(B, C, size, size, device=dev, dtype=dtype)
    m = (ctypes.c_float * C)(*[float(v) for v in mean[:C]])
    s = (ctypes.c_float * C)(*[float(v) for v in std[:C]])
    with torch.cuda.device(dev):
        call("attwarp_clip_preprocess_u8", ptr(x), B, H, W, C, top, left, size, ptr(bx), ptr(kx), ksx, ptr(by), ptr(ky),
             ksy, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), ptr(tmp), ptr(out),
             _lib.F32 if dtype == torch.float32 else _lib.F16, stream_ptr(dev))
    return out


_CLIP_IMAGE_DTYPE = np.dtype(_lib.ClipImage)            # attwarp_clip_image as a record array: one column per field
# the per-image record inside a planned table (clip_ragged.hip: ClipImageDev): the caller's record + the launcher's choices
_CLIP_RECORD_DTYPE = np.dtype(_CLIP_IMAGE_DTYPE.descr + [("tmp_off", "<i8"), ("fused", "<i4"), ("ny", "<i4"), ("rb", "<i4"),
                                                         ("nr_cap", "<i4"), ("window", "<i4"), ("reserved2", "<i4")])


def _clip_tables(n_in: int, n_out: int, device: torch.device):
    """Pillow's 8-bit BICUBIC tables n_in -> n_out on the device, at their own tap count (identity tables for
    n_in == n_out): (bounds int32 [n_out,2], kk int32 [n_out,ksize], ksize)."""
    key = ("clip_bicubic", n_in, n_out, str(device))
    t = _tables._DEV_CACHE.get(key)
    if t is None:
        bounds, kk, ksize = _tables._lanczos_tables_host(n_in, n_out, "bicubic")
        kk = np.ascontiguousarray(kk[:, :ksize])
        t = _tables._cache_put(key, (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize))
    return t


def clip_geometry(H: int, W: int, size: int, pad_to_square: bool) -> dict:
    """The geometry columns of one image's attwarp_clip_image record.  ``pad_to_square``: LLaVA's expand2square canvas of
    side max(H, W) with the image centred on it (offset ``(n - short) // 2``), resized to size x size.  Otherwise the HF
    processor's own route: shorter edge to ``size``, longer edge to ``int(size * long / short)``, centre crop; Pillow runs
    the vertical pass first on a source more than 100 times as high as wide that it shrinks vertically."""
    if pad_to_square:
        n = max(H, W)
        return dict(canvas_w=n, canvas_h=n, pad_x=(n - W) // 2, pad_y=(n - H) // 2, nw=size, nh=size, left=0, top=0,
                    vertical_first=0)
    short, long_ = (H, W) if H <= W else (W, H)
    new_long = int(size * long_ / short)
    nh, nw = (size, new_long) if H <= W else (new_long, size)
    return dict(canvas_w=W, canvas_h=H, pad_x=0, pad_y=0, nw=nw, nh=nh, left=(nw - size) // 2, top=(nh - size) // 2,
                vertical_first=int(H > 100 * W and nh < H))


class ClipBatch:
    """One batch of uint8 [H_i,W_i,C] GPU images planned for ``attwarp_clip_images_u8``: the coefficient
    tables (cached per distinct ``(n_in, n_out)``), the record table (host copy + device copy, uploaded through the pinned
    staging pool), the uint8 intermediate of the images that take the two-launch route and the output [B,C,size,size].
    ``run()`` enqueues the launch(es) on the current stream -- any stream: it first waits for the event recorded behind the
    uploads of the constructor -- and may be captured in a graph; a capture cannot wait for that event, so it must begin
    after the constructing stream's work (``capture_step`` does that).  The images are referenced, not copied: keep them
    alive and unchanged until the launch has run, and let the stream that wrote them be ordered before the one ``run()`` is
    called on.  The padded canvas of ``pad_to_square`` is never built: the kernels read the background where a tap leaves
    the image."""

    def __init__(self, images, size: int = 336, dtype: torch.dtype = torch.float16, mean=OPENAI_CLIP_MEAN,
                 std=OPENAI_CLIP_STD, pad_to_square: bool = True, background=None, out: Optional[torch.Tensor] = None):
        size = int(size)
        if size < 1:
            raise ValueError(f"ClipBatch: size must be positive (got {size})")
        if dtype not in (torch.float32, torch.float16):
            raise TypeError("ClipBatch: dtype must be float32 or float16")
        images = list(images)
        if not images:
            raise ValueError("ClipBatch: empty batch")
        for im in images:
            if not isinstance(im, torch.Tensor):
                raise TypeError("ClipBatch: uint8 [H,W,C] GPU tensors expected (clip_preprocess_ragged uploads host images)")
        dev = require_gpu(*images)
        for im in images:
            if im.dtype != torch.uint8:
                raise TypeError(f"ClipBatch: images must be uint8 (got {im.dtype})")
            if im.dim() != 3:
                raise ValueError(f"ClipBatch: images must be [H,W,C] (got {tuple(im.shape)})")
        C = int(images[0].shape[2])
        if C not in (1, 3) or any(int(im.shape[2]) != C for im in images):
            raise ValueError("ClipBatch: every image must have the same channel count, 1 or 3")
        if any(im.numel() == 0 for im in images):
            raise ValueError("ClipBatch: empty image")
        if len(mean) < C or len(std) < C:
            raise ValueError(f"ClipBatch: mean and std need {C} channel values")
        if background is None:
            background = tuple(int(float(m) * 255) for m in mean[:C])
        if len(background) < C or any(not 0 <= int(v) <= 255 for v in background[:C]):
            raise ValueError(f"ClipBatch: background needs {C} channel values in 0 .. 255")
        self.images = [im if im.is_contiguous() else im.contiguous() for im in images]
        self.B, self.C, self.size, self.dtype, self._dev = len(images), C, size, dtype, dev
        self.pad_to_square = bool(pad_to_square)
        rec = np.zeros(self.B, dtype=_CLIP_IMAGE_DTYPE)
        geo = [clip_geometry(int(im.shape[0]), int(im.shape[1]), size, self.pad_to_square) for im in self.images]
        tx = [_clip_tables(g["canvas_w"], g["nw"], dev) for g in geo]
        ty = [_clip_tables(g["canvas_h"], g["nh"], dev) for g in geo]
        rec["image"] = [im.data_ptr() for im in self.images]
        rec["H"] = [int(im.shape[0]) for im in self.images]
        rec["W"] = [int(im.shape[1]) for im in self.images]
        for k in geo[0]:
            rec[k] = [g[k] for g in geo]
        rec["bounds_x"] = [t[0].data_ptr() for t in tx]; rec["kk_x"] = [t[1].data_ptr() for t in tx]
        rec["bounds_y"] = [t[0].data_ptr() for t in ty]; rec["kk_y"] = [t[1].data_ptr() for t in ty]
        rec["ksize_x"] = [t[2] for t in tx]; rec["ksize_y"] = [t[2] for t in ty]
        self._keep = tx + ty
        rp = ctypes.c_void_p(rec.ctypes.data)
        self.table_host, self.header = planned_table(
            ("attwarp_clip_images_table_bytes", rp, self.B, C, size), ("attwarp_clip_images_plan", rp, self.B, C, size, TABLE),
            _lib.ClipHeader, _lib.AttWarpError, "attwarp_clip_images_table_bytes: ")
        self.table_dev = uploaded(self.table_host, dev)
        self.tmp = torch.empty(int(self.header.tmp_bytes), device=dev, dtype=torch.uint8) if self.header.tmp_bytes else None
        if out is None:
            out = torch.empty(self.B, C, size, size, device=dev, dtype=dtype)
        elif tuple(out.shape) != (self.B, C, size, size) or out.dtype != dtype or not out.is_contiguous() or out.device != dev:
            raise ValueError("ClipBatch: out must be a dense (B,C,size,size) tensor of `dtype` on the images' device")
        self.out = out
        self._mean = (ctypes.c_float * C)(*[float(v) for v in mean[:C]])
        self._std = (ctypes.c_float * C)(*[float(v) for v in std[:C]])
        self._bg = (ctypes.c_uint8 * C)(*[int(v) for v in background[:C]])
        self._ready = torch.cuda.Event()
        self._ready.record(torch.cuda.current_stream(dev))

    @property
    def plan(self) -> np.ndarray:
        """What the launcher chose per image (structured array): the geometry columns, ``fused`` (1: the one-launch kernel),
        its register ``window`` (8 or 16 taps), band height ``ny``, staged canvas rows per round ``rb`` and LDS rows
        ``nr_cap``; ``fused`` 0, ``window`` 0 and ``tmp_off`` on the two-launch route."""
        off = int(self.header.off_images)
        return self.table_host[off:off + self.B * _CLIP_RECORD_DTYPE.itemsize].view(_CLIP_RECORD_DTYPE)

    @property
    def algorithmic_bytes(self) -> int:
        """Sources read once, the batch written once."""
        return sum(im.numel() for im in self.images) + self.out.numel() * self.out.element_size()

    def run(self) -> torch.Tensor:
        with torch.cuda.device(self._dev):
            if not torch.cuda.is_current_stream_capturing():        # (a capture begins after the constructing stream's work)
                torch.cuda.current_stream(self._dev).wait_event(self._ready)
            call("attwarp_clip_images_u8", self.table_host.ctypes.data, ptr(self.table_dev),
                 ctypes.cast(self._mean, ctypes.c_void_p), ctypes.cast(self._std, ctypes.c_void_p),
                 ctypes.cast(self._bg, ctypes.c_void_p), ptr(self.tmp), ptr(self.out),
                 _lib.F32 if self.dtype == torch.float32 else _lib.F16, stream_ptr(self._dev))
        return self.out


def clip_preprocess_ragged(images, size: int = 336, dtype: torch.dtype = torch.float16, mean=OPENAI_CLIP_MEAN,
                           std=OPENAI_CLIP_STD, pad_to_square: bool = True, background=None) -> torch.Tensor:
    """A batch of images of their own sizes -> CLIP-ready [B,C,size,size] on the GPU, the whole batch per call: what
    LLaVA-1.5's ``process_images`` computes on the CPU one PIL image at a time (functions.py:262-271), bit for bit.
    ``images``: uint8 [H_i,W_i,C] GPU tensors (for instance the views of :func:`upload_images`), or, all of them, host
    images (PIL or numpy), which go through ``upload_images`` first (one transfer).  ``pad_to_square=True`` is
    ``image_aspect_ratio == "pad"`` (``background`` defaults to ``int(mean * 255)`` per channel); ``False`` the HF processor's
    shorter-edge resize + centre crop that :func:`clip_preprocess` computes for a dense batch."""
    images = list(images)
    if not images:
        raise ValueError("clip_preprocess_ragged: empty batch")
    if not any(isinstance(im, torch.Tensor) for im in images):
        images = upload_images(images)
    return ClipBatch(images, size, dtype, mean, std, pad_to_square, background).run()


def _field(obj, key):
    """``obj[key]`` or ``obj.key`` (HF size dictionaries come as either), None when absent."""
    if obj is None:
        return None
    try:
        return obj[key]
    except (KeyError, TypeError, IndexError, AttributeError):
        return getattr(obj, key, None)


def process_images(images, image_processor, model_cfg, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Duck-typed drop-in for LLaVA's ``process_images(images, image_processor, model_cfg)`` (the call at
    AGW/attention_extraction/functions.py:270) on the GPU: ``image_mean``, ``image_std``, the shortest-edge / crop size are
    read from ``image_processor``, ``image_aspect_ratio`` from ``model_cfg``.  ``"pad"`` pads to a square of
    ``int(mean * 255)`` first; an absent or any other plain mode is the processor alone (resize + centre crop).  Returns
    float32 [B,3,size,size] as LLaVA's does (the caller casts; ``dtype=torch.float16`` gives the cast result directly)."""
    mode = getattr(model_cfg, "image_aspect_ratio", None)
    if isinstance(mode, str) and mode.startswith("anyres"):
        raise NotImplementedError("process_images: image_aspect_ratio == 'anyres' (multi-patch inputs) is not implemented")
    size = getattr(image_processor, "size", None)
    short = size if isinstance(size, int) else _field(size, "shortest_edge")
    if short is None and _field(size, "height") is not None and _field(size, "height") == _field(size, "width"):
        short = _field(size, "height") if mode == "pad" else None          # a fixed (h, w) resize is another arithmetic unless the source is square
    crop = getattr(image_processor, "crop_size", None)
    ch, cw = (crop, crop) if isinstance(crop, int) else (_field(crop, "height"), _field(crop, "width"))
    if ch is None:
        ch = cw = short
    if short is None or int(ch) != int(short) or int(cw) != int(short):
        raise NotImplementedError(f"process_images: needs a shortest-edge resize and a square centre crop of one size "
                                  f"(got size={size}, crop_size={crop})")
    for flag in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
        if getattr(image_processor, flag, True) is False:
            raise NotImplementedError(f"process_images: {flag}=False is not implemented")
    resample = getattr(image_processor, "resample", 3)
    if resample is not None and int(resample) != 3:
        raise NotImplementedError(f"process_images: resample must be PIL BICUBIC (3), got {resample}")
    factor = getattr(image_processor, "rescale_factor", 1 / 255)
    if factor is not None and float(factor) != 1 / 255:
        raise NotImplementedError(f"process_images: rescale_factor must be 1/255, got {factor}")
    mean = tuple(float(v) for v in image_processor.image_mean)
    std = tuple(float(v) for v in image_processor.image_std)
    return clip_preprocess_ragged(images, int(short), dtype, mean, std, pad_to_square=(mode == "pad"))


def random_clip_vision_tower(device, dtype: torch.dtype = torch.float16, seed: int = 0):
    """The architecture of LLaVA-1.5's vision tower (openai/clip-vit-large-patch14-336: ViT-L/14 at 336 x 336, 24 layers,
    hidden 1024, 16 heads, MLP 4096) from ``transformers`` with SEEDED RANDOM weights -- the checkpoint, the ``llava``
    package and TextVQA are absent here (no network), so BASELINE configs[4] can be closed as a data flow with the right
    shapes and dtypes, not as an accuracy number.  Stock PyTorch-ROCm ops (MFMA-class library GEMMs): outside the
    hand-kernel scope, like MarginalNet's convolutions (SURVEY 8d "bounding roofline")."""
    from transformers import CLIPVisionConfig, CLIPVisionModel
    cfg = CLIPVisionConfig(image_size=336, patch_size=14, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
                           intermediate_size=4096, projection_dim=768)
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        tower = CLIPVisionModel(cfg)
    finally:
        torch.random.set_rng_state(gen_state)
    return tower.to(device=device, dtype=dtype).eval()


@torch.no_grad()
def vision_tower_features(tower, pixel_values: torch.Tensor, select_layer: int = -2) -> torch.Tensor:
    """LLaVA-1.5's feature selection (``mm_vision_select_layer = -2``, ``mm_vision_select_feature = "patch"``; the reference
    feeds the warped image through it at AGW/evaluate_accuracy.py:157-178): pixel_values [B,3,336,336] ->
    ``hidden_states[-2][:, 1:]`` [B,576,1024] -> the token map [B,1024,24,24] MarginalNet consumes (MN/model.py:55-68)."""
    out = tower(pixel_values=pixel_values.to(next(tower.parameters()).dtype), output_hidden_states=True)
    tok = out.hidden_states[select_layer][:, 1:]
    B, n, d = tok.shape
    g = int(round(n ** 0.5))
    return tok.transpose(1, 2).reshape(B, d, g, g)


@torch.no_grad()
def config5_chain(tower, net, images_u8: torch.Tensor, txt_tok: torch.Tensor, txt_mask: torch.Tensor, out_size=(500, 500),
                  mode: str = "cv2", record=None):
    """BASELINE configs[4] as a device-resident data flow (nothing leaves the GPU, no PNG round trip):

        images_u8 [B,H,W,3] -> CLIP tensor -> vision tower -> token map [B,1024,24,24]                  (the model's own pass)
          -> MarginalNet(1024, 4096, 256)(token map, text tokens) -> px, py [B,24]                     MN/model.py:55-95
          -> A8 + A9 + A11 -> A12: warp of the uint8 images to ``out_size``                             MN/trainer.py:285-289
          -> CLIP tensor of the WARPED images [B,3,336,336] -> vision tower -> features [B,1024,24,24]  evaluate_accuracy.py:157-178

    ``record``: a callable ``record(name)`` invoked after each leg (bench.py records HIP events there).  Returns a dict of
    every intermediate.  Parity of each hand-written leg is pinned elsewhere (clip_preprocess, MarginalNet tail, the warp);
    TextVQA accuracy parity is unobtainable here: LLaVA-1.5-7B's weights, the ``llava`` package and the dataset are absent."""
    rec = record or (lambda name: None)
    dtype = next(tower.parameters()).dtype
    pix0 = clip_preprocess(images_u8, 336, dtype, pad_to_square=True)
    rec("clip_tensor_in")
    fmap = vision_tower_features(tower, pix0)
    rec("tower_in")
    px, py = net(fmap, GRID, GRID, txt_tok, txt_mask)
    rec("marginalnet")
    B, H, W, _ = images_u8.shape
    mx, my = axis_maps_from_pdf(px, py, (H, W), out_size)
    warped = cu.remap_separable(images_u8, mx, my, mode=mode, channels_last=True)
    rec("warp")
    pix1 = clip_preprocess(warped, 336, dtype, pad_to_square=True)
    rec("clip_tensor_warped")
    feats = vision_tower_features(tower, pix1)
    rec("tower_warped")
    return {"pixel_values_in": pix0, "token_map": fmap, "px": px, "py": py, "map_x": mx, "map_y": my, "warped": warped,
            "pixel_values_warped": pix1, "features_warped": feats}


def capture_step(fn, *args, warmup: int = 2):
    """Capture ``fn(*args)`` (a function made only of this package's launches on static tensors) into a
    HIP graph; returns (graph, output).  ``graph.replay()`` re-runs the step with one host call."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warmup):
            out = fn(*args)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn(*args)
    return g, out


def capture_steps(step_fn, k0: int, n: int, dev: torch.device):
    """Capture step_fn(k0, main) .. step_fn(k0 + n - 1, main) as one HIP graph.  The steps launch on the current stream,
    which is ``main``, a private capture stream, over static buffers; a step that forks side streams joins them back into
    ``main`` before it returns."""
    g = torch.cuda.CUDAGraph()
    main = torch.cuda.Stream(device=dev)
    main.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(main):
        with torch.cuda.graph(g, stream=main):
            for k in range(k0, k0 + n):
                step_fn(k, main)
    torch.cuda.current_stream().wait_stream(main)
    return g


class _StepGraphs:
    """Base of the four stream drivers: their HIP graphs, captured on first use, kept by the state they start from and
    replayed after.  A driver defines

        _graph_step(k, main)   the launches of step k inside a capture (see :func:`capture_steps`)
        _graph_start()         (state, k0): the hashable state a graph captured now would start from -- everything that
                               decides which buffers its steps touch -- and the k of its first step
        _advance(m)            move the driver m steps on

    A driver that is reset and run again finds the states of its first pass and captures nothing new (``graph_captures``
    counts).  A base class, not a member holding callbacks: a driver must not sit in a reference cycle.  It owns HIP graphs
    and device buffers, and what reference counting does not free the collector frees whenever it runs -- in the middle of
    another driver's capture, where that is an error."""

    def _init_graphs(self, dev):
        self._graph_dev, self._graphs, self.graph_captures = dev, {}, 0

    def _replay(self, key, k0: int, n: int):
        """The graph of steps k0 .. k0 + n - 1 kept under ``key``: captured on a miss, replayed either way."""
        g = self._graphs.get(key)
        if g is None:
            g = self._graphs[key] = capture_steps(self._graph_step, k0, n, self._graph_dev)
            self.graph_captures += 1
        g.replay()

    def _play(self, n: int):
        """n steps from the current state as ONE graph (one host call), then advance."""
        state, k0 = self._graph_start()
        self._replay((state, n), k0, n)
        self._advance(n)

    def _run_graphs(self, n: int, unroll: int) -> int:
        """Graphs of ``unroll`` steps while they fit into n (none for unroll < 1); returns the number of steps left."""
        while unroll > 0 and n >= unroll:
            self._play(unroll)
            n -= unroll
        return n

    def _run(self, n: int, unroll: int):
        """n steps: graphs of ``unroll`` steps while they fit, then single steps."""
        for _ in range(self._run_graphs(n, unroll)):
            self._play(1)


def _ring(x, who: str, what: str, dtypes, ndim: Optional[int], mismatch=TypeError, strided=TypeError) -> list:
    """A tensor or a list of tensors -> the ring (list) of static buffers a stream driver cycles through: not empty, one
    shape (of ``ndim`` dimensions, None: any), one dtype (out of ``dtypes``, None: any), contiguous -- a graph holds raw
    pointers.  ``mismatch`` / ``strided``: the exception types of the shape-and-dtype and of the contiguity check."""
    ring = list(x) if isinstance(x, (list, tuple)) else [x]
    if not ring:
        raise ValueError(f"{who}: {what} must be a tensor or a non-empty list of tensors")
    t0 = ring[0]
    if any(t.shape != t0.shape or t.dtype != t0.dtype or (ndim is not None and t.dim() != ndim)
           or (dtypes is not None and t.dtype not in dtypes) for t in ring):
        names = "any dtype" if dtypes is None else " / ".join(str(d).replace("torch.", "") for d in dtypes)
        raise mismatch(f"{who}: {what} must have one shape{'' if ndim is None else f' of {ndim} dimensions'} and one dtype "
                       f"({names})")
    if not all(t.is_contiguous() for t in ring):
        raise strided(f"{who}: {what} must be contiguous (static buffers: the graphs hold raw pointers)")
    return ring


_ATTENTION_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


_TRANSFORM_KW = ("transform", "exp_scale", "exp_divisor", "apply_inverse")


def _transform_args(transform="identity", exp_scale=1.0, exp_divisor=1.0, apply_inverse=False) -> tuple:
    """save_warped_image's keyword arguments (new_method.py:405-411; ``_TRANSFORM_KW`` names them in this order) as the
    launches take them: unknown names mean identity (:400-403), float scale and divisor, bool inverse.  A tuple: every
    ragged launch calls this."""
    return transform if transform in nm._KNOWN else "identity", float(exp_scale), float(exp_divisor), bool(apply_inverse)


class OverlappedWarp(_StepGraphs):
    """Steady-state form of ``warp_from_attention_stack`` for a stream of equally shaped batches.  The three kernels of
    a step belong to three different batches and are independent --
        R: the resample of batch k                      (HBM-bound, maps[c])
        M: the map construction of batch k+1            (latency-bound, steps[c] -> maps[1-c])
        A: the attention reduce of batch k+2            (a second bandwidth stream, rows -> steps[1-c])
    -- so they need not run reduce -> maps -> resample back to back for every batch.  ``pattern``:
        "fused": R | M | A as block ranges of ONE launch (attwarp_warp_step_fused; float32 images on the staged resample)
        "am":    A + M as one launch (attwarp_attn_reduce_and_maps), then R on its own (images of >= 4 MB, where the
                 resample is > 90 % of the step and runs best with its stand-alone dispatch; any image dtype)
        "dag":   R and A on one stream, M on a side stream with exactly the edges the buffers need
        "join":  three graph branches forked and joined in every step
        "auto":  "am" for float32 images of >= 4 MB, else "fused" when eligible (float32 images), else "am".
    Steps are replayed as HIP graphs over static buffers; the per-step maps and attention maps are double buffered.

    ``images`` / ``rows`` are either one static buffer each (the caller copies every batch in) or RINGS of n buffers
    (lists of equal length): batch k lives in ``images[k % n]`` / ``rows[k % n]`` and is warped into ``outs[k % n]``,
    so a producer can fill slot (k+1) % n while slot k % n is being read, and a measurement over a ring larger than the
    Infinity Cache streams every batch from HBM.

        ow = OverlappedWarp(images, rows, starts)      # allocates outs, captures lazily
        rows[0] <- attention of batch 0;  ow.prime()   # reduce + maps of batch 0 (serial)
        rows[1 % n] <- attention of batch 1;  ow.prime2()   # reduce of batch 1 (serial)
        for k in 0 .. N-1:
            images[k % n] <- batch k;  rows[(k+2) % n] <- attention of batch k+2 (if any)
            out = ow.step()                            # R(k) || M(k+1) || A(k+2)   -> outs[k % n]
    i.e. the attention runs two batches ahead of the images (``ow.flush()`` = R alone, for a tail).  Every step is
    bit-identical to ``warp_from_attention_stack`` on its batch (same kernels, same arguments)."""

    def __init__(self, images, rows, starts: torch.Tensor, out_size=None, channels_last: bool = False,
                 mode: str = "cv2", pattern: str = "auto"):
        if pattern not in ("auto", "fused", "am", "dag", "join"):
            raise ValueError("OverlappedWarp: pattern must be 'auto', 'fused', 'am', 'dag' or 'join'")
        self.pattern = pattern
        self.images = _ring(images, "OverlappedWarp", "images", None, 4, mismatch=ValueError, strided=ValueError)
        self.rows = _ring(rows, "OverlappedWarp", "attention rows [T,B,heads,kv]", _ATTENTION_DTYPES, 4, strided=ValueError)
        if len(self.images) != len(self.rows) or self.images[0].shape[0] != self.rows[0].shape[1]:
            raise ValueError("OverlappedWarp: images and rows must be rings of the same length, of batches of the same size")
        dev = require_gpu(*self.images, *self.rows, starts)
        if not starts.is_contiguous():
            raise ValueError("OverlappedWarp: starts must be contiguous (the graphs hold raw pointers)")
        self.n = len(self.images)
        self.starts = starts.clone()         # own copy: set_starts() writes into it
        self.channels_last, self.mode = channels_last, mode
        img0 = self.images[0]
        B, H, W, C = img0.shape if channels_last else (img0.shape[0], img0.shape[2], img0.shape[3], img0.shape[1])
        Ho, Wo = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
        self.B, self.C, self.H, self.W, self.Ho, self.Wo = B, C, H, W, Ho, Wo
        self.size_hw = (H, W)
        self.out_size = out_size
        self._T, _, self._heads, self._kv = self.rows[0].shape
        self.starts_tiled = starts.repeat(self._T).contiguous()
        shape = (B, Ho, Wo, C) if channels_last else (B, C, Ho, Wo)
        self.outs = [torch.empty(shape, device=dev, dtype=img0.dtype) for _ in range(self.n)]
        self.cur = 0                 # which (steps, maps) buffer set the next resample reads
        self.k = 0                   # ring position of the next resample
        self._dev = dev
        self._sideM = torch.cuda.Stream(device=dev)
        self._sideA = torch.cuda.Stream(device=dev)
        self._init_graphs(dev)
        # both buffer sets, filled once outside capture (allocations, lazily built tables)
        self.steps = [attention_step_maps(self.rows[0], self.starts, ae.NUM_IMAGE_TOKENS, self.starts_tiled) for _ in (0, 1)]
        self.maps = [axis_maps_from_attention_steps(self.steps[i], self.size_hw, self.out_size) for i in (0, 1)]
        cu.remap_separable(self.images[0], *self.maps[0], mode=self.mode, channels_last=self.channels_last, out=self.outs[0])
        torch.cuda.synchronize(dev)
        self._inv = (_tables.right_inverse_inv(GRID, W, 1e-8, dev), _tables.right_inverse_inv(GRID, H, 1e-8, dev))
        if self.pattern == "auto" and img0.dtype == torch.float32 and img0[0].numel() * 4 >= (4 << 20):
            # large images (>= 4 MB each): the resample is > 90 % of a step and keeps its own launch (inside the fused launch it runs 2 %
            # slower); the reduce and the latency-bound map construction share one (attwarp_attn_reduce_and_maps)
            self.pattern = "am"
        if self.pattern in ("auto", "fused"):
            # one launch per step (attwarp_warp_step_fused) when the shapes are eligible: float32 images on the staged
            # resample, attention rows in any of the three dtypes
            try:
                if img0.dtype != torch.float32:
                    raise _lib.AttWarpError("fused step: float32 images only")
                self._fused_step(0, 0)
                torch.cuda.synchronize(dev)
                self.pattern = "fused"
            except _lib.AttWarpError:
                if self.pattern == "fused":
                    raise
                # measured (uint8 images): "am" 0.040 / 0.124 ms per step at B=64 / 256 336x336
                # against 0.048 / 0.131 ("dag") and 0.048 / 0.125 ("join")
                self.pattern = "am"
            # the trial step overwrote maps[1] / steps[1] with what they held anyway (same inputs)

    def _fused_step(self, c, k):
        """R(k) | M(k+1) | A(k+2) as ONE launch (block ranges of one grid)."""
        img, out = self.images[k % self.n], self.outs[k % self.n]
        rows = self.rows[(k + 2) % self.n]
        T, B = self._T, self.B
        mx, my = self.maps[c]
        nx, ny = self.maps[1 - c]
        with torch.cuda.device(self._dev):
            call("attwarp_warp_step_fused", ptr(img), ptr(out), _lib.HWC if self.channels_last else _lib.CHW, B, self.C, self.H,
                 self.W, self.Ho, self.Wo, ptr(mx), ptr(my), _lib.MODE_IDS[self.mode],
                 _lib.dtype_id(rows), ptr(self.steps[c]), T, GRID, ptr(self._inv[0]), ptr(self._inv[1]), ptr(nx), ptr(ny),
                 ptr(rows), T * B, self._heads, self._kv, ptr(self.starts_tiled), T * B, ae.NUM_IMAGE_TOKENS,
                 ptr(self.steps[1 - c]), stream_ptr(self._dev))

    @property
    def out(self) -> torch.Tensor:
        """Output buffer of the most recent step."""
        return self.outs[(self.k - 1) % self.n]

    def _am_step(self, c, k):
        """A(k+2) + M(k+1) as one launch, then R(k)."""
        self._am_launch(c, k)
        self._resample(c, k % self.n)

    def _am_launch(self, c, k):
        """A(k+2): rows[k+2] -> steps[1-c]  and  M(k+1): steps[c] -> maps[1-c]  as ONE launch."""
        rows = self.rows[(k + 2) % self.n]
        T, B = self._T, self.B
        nx, ny = self.maps[1 - c]
        with torch.cuda.device(self._dev):
            call("attwarp_attn_reduce_and_maps", _lib.dtype_id(rows), ptr(rows), T * B, self._heads, self._kv,
                 ptr(self.starts_tiled), T * B, ae.NUM_IMAGE_TOKENS, ptr(self.steps[1 - c]), ptr(self.steps[c]), T, B, GRID,
                 self.W, self.H, self.Wo, self.Ho, ptr(self._inv[0]), ptr(self._inv[1]), ptr(nx), ptr(ny), stream_ptr(self._dev))

    def _reduce(self, i, r):
        """A: rows[r] -> steps[i]"""
        n_rows = self._T * self.B
        ae.attn_reduce_step(self.rows[r].view(n_rows, self._heads, 1, self._kv), self.starts_tiled, ae.NUM_IMAGE_TOKENS,
                            out=self.steps[i].view(n_rows, ae.NUM_IMAGE_TOKENS))

    def _maps(self, i_steps, i_maps):
        """M: steps[i_steps] -> maps[i_maps]"""
        axis_maps_from_attention_steps(self.steps[i_steps], self.size_hw, self.out_size, maps_out=self.maps[i_maps])

    def _resample(self, i, r):
        cu.remap_separable(self.images[r], *self.maps[i], mode=self.mode, channels_last=self.channels_last,
                           out=self.outs[r])

    def _graph_step(self, k, main):
        """One step inside a capture on ``main``, with the buffer set the stream has reached at ring position k.  It launches
        R(k): resample images[k] with maps[c] | M(k+1): steps[c] -> maps[1-c] | A(k+2): rows[k+2] -> steps[1-c].
        pattern "dag": R and A alternate on ONE stream (both are bandwidth-bound: side by side they would only share
        the same HBM), the latency-bound M runs on a side stream with exactly the edges the buffers need -- M(k+1) after
        A(k+1) and R(k-1) (which read maps[1-c]), R(k+1) after M(k+1), A(k+3) after M(k+1) (which read steps[c]) -- so the
        main stream never waits for a kernel that has not long finished.  pattern "join": three branches forked and
        joined in every step."""
        c = self.cur ^ ((k - self.k) & 1)                    # (cur and k stand still while their graph is captured)
        if self.pattern == "fused":
            self._fused_step(c, k)
        elif self.pattern == "am":
            self._am_step(c, k)
        elif self.pattern == "dag":
            # main so far: ..., A(k+1), R(k-1) [previous step: R then A]; side: ..., M(k)
            self._sideM.wait_stream(main)                # M(k+1) after A(k+1) and R(k-1)
            with torch.cuda.stream(self._sideM):
                self._maps(c, 1 - c)
            self._resample(c, k % self.n)                # R(k) needs M(k): joined at the end of step u-1
            self._reduce(1 - c, (k + 2) % self.n)        # A(k+2) overwrites steps[1-c], read by M(k): done
            main.wait_stream(self._sideM)                # next R needs M(k+1); next A overwrites steps[c]
        else:
            self._sideM.wait_stream(main)                # fork
            self._sideA.wait_stream(main)
            with torch.cuda.stream(self._sideA):
                self._reduce(1 - c, (k + 2) % self.n)
            with torch.cuda.stream(self._sideM):
                self._maps(c, 1 - c)
            self._resample(c, k % self.n)
            main.wait_stream(self._sideM)                # join
            main.wait_stream(self._sideA)

    def _graph_start(self):
        return (self.cur, self.k % self.n), self.k           # cur is not the parity of k: flush() advances k alone

    def _advance(self, m):
        self.cur ^= m & 1
        self.k += m

    @staticmethod
    def round_unroll(unroll: int, n: int) -> int:
        """The graph length run() uses: even, and for a ring of n > 1 buffers a multiple of lcm(2, n) (at least one), so
        that a graph returns to the state it started from and is re-used; 0 (single steps only) below 2."""
        unroll -= unroll % 2
        if unroll >= 2 and n > 1:
            period = math.lcm(2, n)
            unroll = max(period, unroll - unroll % period)
        return unroll if unroll >= 2 else 0

    def run(self, n: int, unroll: int = 8) -> torch.Tensor:
        """n steps on the buffers as they are (steady-state measurement / a producer that stays ahead of the ring):
        graphs of ``unroll`` steps (one host call per ``unroll`` steps), then single steps for the remainder.  With a
        ring of n buffers a graph of lcm(2, n)-multiple length returns to the state it started from and is re-used."""
        self._run(n, self.round_unroll(unroll, self.n))
        return self.out

    def set_starts(self, starts: torch.Tensor):
        """New first-image-token positions ([B] int32) for the batches reduced from now on: copied into the static
        buffer the captured graphs read (stream ordered; the attention runs two batches ahead of the images, so a
        stream whose prompts change per batch calls this before the step that reduces that batch)."""
        if starts.shape != self.starts.shape or starts.dtype != self.starts.dtype or starts.device != self.starts.device:
            raise ValueError("OverlappedWarp.set_starts: same shape, dtype and device as the starts given at construction")
        self.starts.copy_(starts)
        self.starts_tiled.copy_(starts.repeat(self.rows[0].shape[0]))

    def reset(self):
        """Back to ring position 0 / buffer set 0 (a new stream on the same static buffers; prime() again)."""
        self.cur = 0
        self.k = 0

    def prime(self):
        """Reduce + maps of the batch at the current ring position into the current buffer set (serial, no graph)."""
        self._reduce(self.cur, self.k % self.n)
        self._maps(self.cur, self.cur)

    def prime2(self):
        """Reduce of the batch after it into the current steps buffer (its maps are built by the first step)."""
        self._reduce(self.cur, (self.k + 1) % self.n)

    def step(self) -> torch.Tensor:
        self._play(1)
        return self.out

    def flush(self) -> torch.Tensor:
        """Resample of the batch at the current ring position with the current maps alone, then advance (tail of a
        stream: no further attention to reduce)."""
        self._resample(self.cur, self.k % self.n)
        self.k += 1
        return self.out

    def tail(self) -> torch.Tensor:
        """The last two batches of a stream that ends: R(N-2) + M(N-1), then R(N-1)."""
        self._resample(self.cur, self.k % self.n)
        self._maps(self.cur, 1 - self.cur)
        self.cur ^= 1
        self.k += 1
        return self.flush()


_StepSlot = _lib.StepSlot


class PairedStepWarp(_StepGraphs):
    """``OverlappedWarp`` pattern "fused" with TWO batches of the stream per piece and launch
    (attwarp_warp_step_fused_slots):

        launch p:   R(2p), R(2p+1)  |  M(2p+2), M(2p+3)  |  A(2p+4), A(2p+5)

    Every dependency is on an earlier launch, and the launch's ramp and tail -- about 8 us of a 60 us step at B=64
    336x336 -- are paid once per two batches.  Per-step maps and step-map buffers exist four times (batch j uses set
    j % 4); ``images`` / ``rows`` are rings of n >= 2 static buffers (even n), batch k in slot k % n, output in
    ``outs[k % n]``.  float32 images on the staged resample, attention rows float32 / float16 / bfloat16.

        pw = PairedStepWarp(images, rows, starts)
        rows[0..3] <- attention of batches 0..3;  pw.prime()         # reduce of 0..3, maps of 0, 1 (serial launches)
        for p in 0 .. N/2 - 1:
            images[2p % n], images[(2p+1) % n] <- batches 2p, 2p+1;  rows[(2p+4) % n], rows[(2p+5) % n] <- attention ahead
            pw.step()                                                  # -> outs[2p % n], outs[(2p+1) % n]
        pw.tail()                                                      # the last four batches without further attention

    Bit-identical, batch by batch, to ``warp_from_attention_stack`` (same kernels bodies, same arguments)."""

    def __init__(self, images, rows, starts: torch.Tensor, out_size=None, channels_last: bool = False, mode: str = "cv2"):
        self.images = _ring(images, "PairedStepWarp", "images", (torch.float32,), 4)
        self.rows = _ring(rows, "PairedStepWarp", "attention rows [T,B,heads,kv]", _ATTENTION_DTYPES, 4)
        img0, r0 = self.images[0], self.rows[0]
        if len(self.images) != len(self.rows) or len(self.images) % 2 or img0.shape[0] != r0.shape[1]:
            raise ValueError("PairedStepWarp: images and rows must be rings of the same even length >= 2, of batches of the "
                             "same size")
        dev = require_gpu(*self.images, *self.rows, starts)
        self.n = len(self.images)
        self.channels_last, self.mode, self._dev = channels_last, mode, dev
        H, W = (img0.shape[1], img0.shape[2]) if channels_last else (img0.shape[2], img0.shape[3])
        self.C = img0.shape[3] if channels_last else img0.shape[1]
        self.B, self.H, self.W = img0.shape[0], H, W
        self.Ho, self.Wo = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
        self._T, _, self._heads, self._kv = r0.shape
        T = self._T
        self.starts = starts.clone()
        self.starts_tiled = starts.repeat(T).contiguous()
        shape = (self.B, self.Ho, self.Wo, self.C) if channels_last else (self.B, self.C, self.Ho, self.Wo)
        self.outs = [torch.empty(shape, device=dev, dtype=torch.float32) for _ in range(self.n)]
        self.steps = [torch.empty(T, self.B, ae.NUM_IMAGE_TOKENS, device=dev, dtype=r0.dtype) for _ in range(4)]
        self.maps = [(torch.empty(self.B, self.Wo, device=dev, dtype=torch.float32),
                      torch.empty(self.B, self.Ho, device=dev, dtype=torch.float32)) for _ in range(4)]
        self.g = GRID
        self._inv = (_tables.right_inverse_inv(GRID, W, 1e-8, dev), _tables.right_inverse_inv(GRID, H, 1e-8, dev))
        self.k = 0
        self._init_graphs(dev)
        self._launch(0)                        # eligibility (raises AttWarpError) + lazy module loading, outside any capture
        torch.cuda.synchronize(dev)

    def _launch(self, k):
        """R(k), R(k+1) | M(k+2), M(k+3) | A(k+4), A(k+5)"""
        T, B = self._T, self.B
        slots = (_StepSlot * 2)()
        for s in (0, 1):
            j = k + s
            mx, my = self.maps[j % 4]
            nx, ny = self.maps[(j + 2) % 4]
            slots[s] = _StepSlot(ptr(self.images[j % self.n]), ptr(self.outs[j % self.n]), ptr(mx), ptr(my),
                                 ptr(self.steps[(j + 2) % 4]), ptr(nx), ptr(ny),
                                 ptr(self.rows[(j + 4) % self.n]), ptr(self.starts_tiled), ptr(self.steps[j % 4]))
        with torch.cuda.device(self._dev):
            call("attwarp_warp_step_fused_slots", ctypes.cast(slots, ctypes.c_void_p), 2,
                 _lib.HWC if self.channels_last else _lib.CHW, B, self.C, self.H, self.W, self.Ho, self.Wo, _lib.MODE_IDS[self.mode],
                 _lib.dtype_id(self.rows[0]), T, self.g, ptr(self._inv[0]), ptr(self._inv[1]), T * B, self._heads, self._kv, T * B,
                 ae.NUM_IMAGE_TOKENS, stream_ptr(self._dev))

    def _reduce(self, j):
        n_rows = self._T * self.B
        ae.attn_reduce_step(self.rows[j % self.n].view(n_rows, self._heads, 1, self._kv), self.starts_tiled,
                            ae.NUM_IMAGE_TOKENS, out=self.steps[j % 4].view(n_rows, ae.NUM_IMAGE_TOKENS))

    def _maps(self, j):
        axis_maps_from_attention_steps(self.steps[j % 4], (self.H, self.W), (self.Ho, self.Wo), maps_out=self.maps[j % 4])

    def _resample(self, j):
        cu.remap_separable(self.images[j % self.n], *self.maps[j % 4], mode=self.mode, channels_last=self.channels_last,
                           out=self.outs[j % self.n])

    def reset(self):
        self.k = 0

    def prime(self):
        k = self.k
        for j in range(k, k + 4):
            self._reduce(j)
        self._maps(k); self._maps(k + 1)

    # a graph step is one launch = two batches (k stays even); its buffer indices depend on k mod 4 (maps) and k mod n (ring)
    def _graph_step(self, p, main):
        self._launch(2 * p)

    def _graph_start(self):
        return self.k % math.lcm(4, self.n), self.k // 2

    def _advance(self, pairs):
        self.k += 2 * pairs

    def step(self):
        """One launch = two batches."""
        self._play(1)

    def run(self, n_batches: int, unroll_pairs: int = 4):
        """n_batches (even) batches: graphs of ``unroll_pairs`` launches, then single launches."""
        if n_batches % 2:
            raise ValueError("PairedStepWarp.run: an even number of batches")
        self._run(n_batches // 2, unroll_pairs)

    def tail(self):
        """The last four batches of a stream that ends: R(k), R(k+1), M + R of k+2, k+3 (their reduce is done)."""
        k = self.k
        self._resample(k); self._resample(k + 1)
        self._maps(k + 2); self._maps(k + 3)
        self._resample(k + 2); self._resample(k + 3)
        self.k += 4


def pair_slots(ring):
    """Views of a ring of equally shaped [B, ...] buffers as a ring of half the length of [2B, ...] buffers: slot i = the
    batches 2i and 2i+1 as ONE batch, for running two batches of a stream per launch (``MaskChainStream(pair_slots(images),
    pair_slots(masks), ...)``: a launch's ramp and tail, and at small batches its unfilled machine, are then paid once per
    two batches; the reference's BATCH_SIZE = 32 is a memory choice of the LLaVA pass, the warp is free to take two).
    Needs an even number of slots with slot 2i+1 directly behind slot 2i in memory, e.g. ``ring = list(torch.empty(n, B,
    ...))``.  The outputs of such a stream are [2B, ...] too: ``out[:B]`` / ``out[B:]``."""
    ring = list(ring)
    if len(ring) % 2:
        raise ValueError("pair_slots: an even number of slots expected")
    out = []
    for a, b in zip(ring[0::2], ring[1::2]):
        if (a.shape != b.shape or a.dtype != b.dtype or a.device != b.device or not (a.is_contiguous() and b.is_contiguous())
                or b.data_ptr() != a.data_ptr() + a.numel() * a.element_size()
                or a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()):
            raise ValueError("pair_slots: slot 2i+1 must lie directly behind slot 2i in the same allocation "
                             "(allocate the ring as one tensor [n, B, ...])")
        out.append(torch.as_strided(a, (2 * a.shape[0],) + tuple(a.shape[1:]), a.stride(), a.storage_offset()))
    return out


class MaskChainStream(_StepGraphs):
    """Steady-state form of :func:`warp_from_masks` -- the chain ``main_batched.py:243-287`` runs per image -- for a STREAM
    of equally shaped batches.  The stages of the chain belong to different batches and are independent:

        V(j)  revise_mask            masks[j] [B,24,24] float32       -> rev               llava.py:223-238
        L(j)  x255, PIL LANCZOS      rev                              -> mota [B,H,W] u8   llava.py:192-196,243,253
        P(j)  float64 marginals      mota                             -> axis sums         new_method.py:206-226
        F(j)  cumsum / np.interp     axis sums                        -> maps              new_method.py:228-265
        R(j)  uint8 cv2.remap        images[j] [B,H,W,3] + maps       -> outs[j]           new_method.py:268-271

    V, L, P, F are bound by instruction issue (integer multiply-adds, float64 adds in numpy's orders) and by dependent
    latency chains; R is the one that streams HBM.  Run back to back for every batch (``pattern="serial"``, the launches
    of ``warp_from_masks`` on static buffers) nothing overlaps.  ``pattern``:

        "branches": R(k) | P(k+1) -> F(k+1) | V(k+2) -> L(k+2) as three branches of one HIP graph, forked and joined every
                    step (existing kernels, the hardware schedules workgroups of the branches side by side)
        "fused":    R(k) | F(k+1) | P(k+2) | L(k+3) | V(k+4) as block ranges of ONE launch per step
                    (attwarp_mask_chain_step), replayed as graphs of ``unroll`` steps
        "ragged":   the same one launch per step through attwarp_mask_chain_ragged (every image described by a table entry):
                    equally sized images whose shape the uniform step refuses -- a width that is not a multiple of 4
        "auto":     "fused" when the shapes are eligible, else "ragged" when the ragged kernel takes them, else "branches"

    ``images`` / ``masks`` are rings of n static buffers (lists of equal length; a single tensor = a ring of one): batch k
    lives in slot k % n and is warped into ``outs[k % n]``.  Usage (d = pipeline depth: 2 for "branches", 4 for "fused"):

        mc = MaskChainStream(images, masks, out_size=(500, 500))
        masks[0 .. d-1] <- the first d batches;  mc.prime()
        for k in 0 .. N-1:
            images[k % n] <- batch k;  masks[(k + d) % n] <- mask of batch k + d (if any)
            out = mc.step()                                   # -> outs[k % n]

    Every step is bit-identical to ``warp_from_masks`` on its batch (same arithmetic per stage; the parity tests compare
    both with the oracle)."""

    PATTERNS = ("auto", "serial", "branches", "fused", "ragged")

    def __init__(self, images, masks, out_size=(500, 500), enhance_coe=10, kernel_size=3, transform="identity",
                 exp_scale=1.0, exp_divisor=1.0, apply_inverse=False, mode: str = "cv2", pattern: str = "auto"):
        if pattern not in self.PATTERNS:
            raise ValueError(f"MaskChainStream: pattern must be one of {self.PATTERNS}")
        self.images = _ring(images, "MaskChainStream", "images [B,H,W,C]", (torch.uint8,), 4)
        self.masks = _ring(masks, "MaskChainStream", "masks [B,n,n]", (torch.float32,), 3)
        if len(self.images) != len(self.masks):
            raise ValueError("MaskChainStream: images and masks must be rings of the same length")
        dev = require_gpu(*self.images, *self.masks)
        img0, m0 = self.images[0], self.masks[0]
        B, H, W, C = img0.shape
        if m0.shape[0] != B or m0.shape[1] != m0.shape[2]:
            raise ValueError("MaskChainStream: masks [B,n,n] must match the image batch")
        if kernel_size % 2 != 1:
            raise ValueError("MaskChainStream: kernel_size must be odd")
        self.n = len(self.images)
        self.B, self.H, self.W, self.C, self.g = B, H, W, C, int(m0.shape[1])
        self.Ho, self.Wo = int(out_size[0]), int(out_size[1])
        self.mode = mode
        self.enhance_coe, self.kernel_size = float(enhance_coe), int(kernel_size)
        xf = _transform_args(transform, exp_scale, exp_divisor, apply_inverse)
        self.transform, self.exp_scale, self.exp_divisor, self.apply_inverse = xf
        self._xf = dict(zip(_TRANSFORM_KW, xf))
        self._dev = dev
        lib = _lib.load()
        self.outs = [torch.empty(B, self.Ho, self.Wo, C, device=dev, dtype=torch.uint8) for _ in range(self.n)]
        self.k = 0
        self._init_graphs(dev)
        self._side = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        self.pattern = pattern
        # the table of the transformed byte values the one-launch steps read for sqrt / exp / log (a constant of the stream)
        self._lut = _tables.attention_transform_lut(self.transform, self.exp_scale, self.exp_divisor, dev)
        if pattern == "ragged":               # (the uniform path's intermediates are not needed: every batch brings its own)
            if not (self.mode == "cv2" and ragged_eligible(H, W, C, self.g) and self.Wo * C <= RAGGED_MAX_ROW_BYTES):
                raise _lib.AttWarpError("MaskChainStream: this shape / these options do not run on the ragged chain kernel")
            self._build_ragged()
        else:
            # parity-indexed intermediates (batch j uses slot j % 2 of each)
            self.rev = [torch.empty(B, self.g, self.g, device=dev, dtype=torch.float32) for _ in (0, 1)]
            self.mota = [torch.empty(B, H, W, device=dev, dtype=torch.uint8) for _ in (0, 1)]
            self.ws = [torch.empty(lib.attwarp_axis_sums_workspace_bytes(B, H, W), device=dev, dtype=torch.uint8) for _ in (0, 1)]
            self.maps = [(torch.empty(B, self.Wo, device=dev, dtype=torch.float32),
                          torch.empty(B, self.Ho, device=dev, dtype=torch.float32)) for _ in (0, 1)]
            self._tmp = torch.empty(B, self.g, W, device=dev, dtype=torch.uint8)       # two-pass Lanczos forms only
            self._tx = _tables.lanczos_tables(self.g, W, dev) if W != self.g else (None, None, 0)
            self._ty = _tables.lanczos_tables(self.g, H, dev) if H != self.g else (None, None, 0)
            if pattern in ("auto", "fused"):
                try:
                    self._fused_launch(0, dry=True)
                    self.pattern = "fused"
                except (_lib.AttWarpError, AttributeError):
                    if pattern == "fused":
                        raise
                    self.pattern = "branches"
            if pattern == "auto" and self.pattern == "branches":
                if self.mode == "cv2" and ragged_eligible(H, W, C, self.g) and self.Wo * C <= RAGGED_MAX_ROW_BYTES:
                    self.pattern = "ragged"
                    del self.rev, self.mota, self.ws, self.maps, self._tmp
                    self._build_ragged()
        self.depth = {"serial": 0, "branches": 2, "fused": 4, "ragged": 4}[self.pattern]

    def _build_ragged(self):
        """Every (ring slot, batch parity) RaggedBatch of the stream, built HERE -- before any capture: building one plans
        a table on the host and uploads it, which must never become a node of a HIP graph (it would be re-executed, from a
        staging buffer that has been reused since, on every replay).  Batch j of the stream lives in ring slot j % n and
        uses the intermediates of parity j & 1: one RaggedBatch per (slot, parity) that occurs -- n for an even ring, 2 n for
        an odd one -- each with its own table (the table names the slot's images), all batches of one parity SHARING one set
        of intermediates (rev / mota / sums / maps: two sets in all, as the uniform step)."""
        self._rb = {}
        first = {}
        for j in range(math.lcm(2, self.n)):
            key = (j % self.n, j & 1)
            img = self.images[key[0]]
            rb = RaggedBatch([img[b] for b in range(self.B)], (self.Ho, self.Wo), self.g, out=self.outs[key[0]],
                             share=first.get(key[1]))
            rb.masks = self.masks[key[0]]
            first.setdefault(key[1], rb)
            self._rb[key] = rb

    # ---- the stages on static buffers (same entry points as warp_from_masks) ----
    def _V(self, j):
        with torch.cuda.device(self._dev):
            call("attwarp_mask_postproc", ptr(self.masks[j % self.n]), self.B, self.g, self.kernel_size, self.enhance_coe,
                 ptr(self.rev[j & 1]), stream_ptr(self._dev))

    def _L(self, j):
        (bx, kx, ksx), (by, ky, ksy) = self._tx, self._ty
        with torch.cuda.device(self._dev):
            call("attwarp_mask_upsample_lanczos", ptr(self.rev[j & 1]), None, self.B, self.g, self.g, self.H, self.W,
                 ptr(bx), ptr(kx), ksx, ptr(by), ptr(ky), ksy, ptr(self._tmp), ptr(self.mota[j & 1]), stream_ptr(self._dev))

    def _PF(self, j):
        mx, my = self.maps[j & 1]
        with torch.cuda.device(self._dev):
            call("attwarp_axis_maps_from_attention", ptr(self.mota[j & 1]), _lib.U8, self.B, self.H, self.W, self.Wo, self.Ho,
                 _lib.TRANSFORM_IDS[self.transform], self.exp_scale, self.exp_divisor, int(self.apply_inverse), ptr(mx),
                 ptr(my), ptr(self.ws[j & 1]), stream_ptr(self._dev))

    def _R(self, j):
        cu.remap_separable(self.images[j % self.n], *self.maps[j & 1], mode=self.mode, channels_last=True,
                           out=self.outs[j % self.n])

    def _fused_launch(self, k, dry=False):
        """R(k) | F(k+1) | P(k+2) | L(k+3) | V(k+4) as ONE launch (attwarp_mask_chain_step).  ``dry``: the eligibility
        trial of the constructor -- the stages write the buffers of the parities they would write in step k, from whatever
        the inputs hold; prime() overwrites all of it."""
        if self.mode != "cv2":
            raise _lib.AttWarpError("mask chain step: cv2 mode only (the integer uint8 resample; what both reference drivers compute)")
        (bx, kx, ksx), (by, ky, ksy) = self._tx, self._ty
        if bx is None or by is None:
            raise _lib.AttWarpError("mask chain step: the mask must be up-sampled on both axes")
        p, q = k & 1, (k + 1) & 1
        mx, my = self.maps[p]
        nx, ny = self.maps[q]
        with torch.cuda.device(self._dev):
            call("attwarp_mask_chain_step", ptr(self.images[k % self.n]), ptr(self.outs[k % self.n]), self.B, self.C, self.H,
                 self.W, self.Ho, self.Wo, ptr(mx), ptr(my),
                 ptr(self.ws[q]), ptr(nx), ptr(ny),                      # F(k+1)
                 ptr(self.mota[p]), ptr(self.ws[p]),                      # P(k+2)
                 ptr(self.rev[q]), ptr(bx), ptr(kx), ksx, ptr(by), ptr(ky), ksy, ptr(self.mota[q]),   # L(k+3)
                 ptr(self.masks[(k + 4) % self.n]), self.g, self.kernel_size, self.enhance_coe, ptr(self.rev[p]),   # V(k+4)
                 _lib.TRANSFORM_IDS[self.transform], self.exp_scale, self.exp_divisor, int(self.apply_inverse), ptr(self._lut),
                 stream_ptr(self._dev))

    def _ragged(self, j):
        """Batch j of the stream: the RaggedBatch of slot j % n (its images, masks and output buffer) with the
        intermediates of parity j & 1 (all built by the constructor)."""
        return self._rb[(j % self.n, j & 1)]

    def ragged_batch(self, j: int) -> RaggedBatch:
        """The RaggedBatch that carries batch j of a ``pattern="ragged"`` stream (e.g. for :func:`heatmap_overlay_ragged`:
        its masks are valid from step j - 3 on and overwritten by step j - 1, see there)."""
        if self.pattern != "ragged":
            raise ValueError("MaskChainStream.ragged_batch: the stream does not run the ragged pattern")
        return self._ragged(j)

    def _ragged_launch(self, **stages):
        ragged_chain_launch(**{s: self._ragged(j) for s, j in stages.items()}, enhance_coe=self.enhance_coe, kernel_size=self.kernel_size,
                            **self._xf)

    # ---- driving ----
    def prime(self):
        """Everything the first step expects to find done for the batches at ring positions k .. k+depth-1 (serial)."""
        k = self.k
        if self.pattern == "ragged":
            _ragged_serial(_RAGGED_FILL, k, lambda st, j: self._ragged_launch(**{st: j}))
            return
        if self.pattern == "branches":      # step k runs R(k) | PF(k+1) | VL(k+2)
            self._V(k); self._L(k); self._PF(k)
            self._V(k + 1); self._L(k + 1)
        elif self.pattern == "fused":       # step k runs R(k) | F(k+1) | P(k+2) | L(k+3) | V(k+4)
            for j in (k, k + 1, k + 2):
                self._V(j); self._L(j)
                if j <= k + 1:
                    self._PF(j)             # (P(k+1) included: its F runs again inside step k, same result)
            self._V(k + 3)

    def _one(self, k):
        if self.pattern == "serial":
            self._V(k); self._L(k); self._PF(k); self._R(k)
        elif self.pattern == "fused":
            self._fused_launch(k)
        elif self.pattern == "ragged":
            self._ragged_launch(R=k, F=k + 1, P=k + 2, L=k + 3, V=k + 4)
        else:
            raise RuntimeError("branches are only defined inside a capture")

    def _graph_step(self, k, main):
        """Step k inside a capture on ``main``."""
        if self.pattern == "branches":
            s1, s2 = self._side
            s1.wait_stream(main); s2.wait_stream(main)          # fork
            with torch.cuda.stream(s1):
                self._PF(k + 1)
            with torch.cuda.stream(s2):
                self._V(k + 2); self._L(k + 2)
            self._R(k)
            main.wait_stream(s1); main.wait_stream(s2)          # join
        else:
            self._one(k)

    def _graph_start(self):
        return self.k % math.lcm(2, self.n), self.k          # the buffer indices of a step depend on k mod n and k mod 2

    def _advance(self, m):
        self.k += m

    @property
    def out(self) -> torch.Tensor:
        """Output buffer of the most recent step."""
        return self.outs[(self.k - 1) % self.n]

    def step(self) -> torch.Tensor:
        self._play(1)
        return self.out

    @staticmethod
    def round_unroll(unroll: int) -> int:
        """The graph length run() uses: even (a graph returns to the parity it started from), at least 2."""
        return max(2, unroll - unroll % 2)

    def run(self, n: int, unroll: int = 8) -> torch.Tensor:
        """n steps on the buffers as they are (steady-state measurement / a producer that stays ahead of the ring): graphs
        of ``unroll`` steps (one host call each), then single steps.  A graph is keyed by the ring position it starts at
        (mod lcm(2, ring length)), so a stream that is reset() and run again replays the graphs of the first pass."""
        self._run(n, self.round_unroll(unroll))
        return self.out

    def reset(self):
        self.k = 0

    def drain(self) -> torch.Tensor:
        """The last ``depth`` batches of a stream that ends (no further masks): the remaining stages, serially."""
        k = self.k
        if self.pattern == "ragged":
            _ragged_serial(_RAGGED_DRAIN, k, lambda st, j: self._ragged_launch(**{st: j}))
        elif self.pattern == "branches":
            self._R(k); self._PF(k + 1); self._R(k + 1)
        elif self.pattern == "fused":
            self._R(k)
            self._PF(k + 1); self._R(k + 1)
            self._PF(k + 2); self._R(k + 2)
            self._L(k + 3); self._PF(k + 3); self._R(k + 3)
        self.k += self.depth
        return self.out


# ---- the main_batched chain for batches of DIFFERENTLY sized images -------------------------------------------------------
RAGGED_MAX_ROW_BYTES = 4096          # attwarp_ragged_plan: rows of the integer cv2 resample
RAGGED_MAX_SIDE = 8192


# the ends of the one-launch-per-step pipeline R(k) | F(k+1) | P(k+2) | L(k+3) | V(k+4), stage by stage: (batch behind k, its
# stages in launch order).  The fill leaves the four batches ahead of step k where that step expects them; the drain finishes
# the four batches in flight behind the last step.
_RAGGED_FILL = ((0, "VLPF"), (1, "VLP"), (2, "VL"), (3, "V"))
_RAGGED_DRAIN = ((0, "R"), (1, "FR"), (2, "PFR"), (3, "LPFR"))


def _ragged_serial(schedule, k: int, launch):
    """``launch(stage, j)`` -- one stage of batch j alone -- for every entry of a fill / drain schedule at position k."""
    for d, stages in schedule:
        for st in stages:
            launch(st, k + d)


def ragged_eligible(h: int, w: int, c: int, g: int = GRID) -> bool:
    """Does an [h,w,c] uint8 image run on the ragged chain kernel (attwarp.h: limits of attwarp_ragged_plan)?"""
    return 4 <= w * c <= RAGGED_MAX_ROW_BYTES and h > g and w > g and max(h, w) <= RAGGED_MAX_SIDE and c <= 4


_RAGGED_IMAGE_DTYPE = np.dtype(_lib.RaggedImage)       # attwarp_ragged_image as a record array: one column per field
_RaggedImageDev = _lib.RaggedImageDev
_AXIS_TABLES: dict = {}
_AXIS_TABLES_LOCK = threading.Lock()     # (host threads share the cache: insert + evict under one lock)


_AXIS_TABLES_MAX = 4096              # distinct (device, g, size) entries kept (40 KB of device memory each at size 1024)


def _axis_tables(g: int, n: int, dev: torch.device):
    """(bounds pointer, coefficient pointer, ksize, bounds tensor, coefficient tensor) of Pillow's g -> n LANCZOS tables on
    `dev`, cached per size (bounded: the oldest entries go first; a RaggedBatch keeps the tensors it points to alive)."""
    key = (dev.index, g, n)
    t = _AXIS_TABLES.get(key)
    if t is None:
        b, k, ks = _tables.lanczos_tables(g, n, dev)
        t = (b.data_ptr(), k.data_ptr(), ks, b, k)
        with _AXIS_TABLES_LOCK:
            while len(_AXIS_TABLES) >= _AXIS_TABLES_MAX:
                _AXIS_TABLES.pop(next(iter(_AXIS_TABLES)), None)
            _AXIS_TABLES[key] = t
    return t


class RaggedBatch:
    """One batch of differently sized uint8 images [H_i,W_i,C] on the GPU, planned for ``attwarp_mask_chain_ragged``:
    the table (host copy in pinned memory + device copy), and the batch's own intermediates and outputs --
    ``rev`` [B,g,g], ``mota`` (the up-sampled masks, packed), ``sums`` (axis sums), ``maps`` and ``out`` [B,H_out,W_out,C].
    The images are referenced, not copied: keep them alive and unchanged until the batch's resample has run."""

    def __init__(self, images, out_size=(500, 500), g: int = GRID, out: Optional[torch.Tensor] = None,
                 share: Optional["RaggedBatch"] = None):
        """``share``: a RaggedBatch of the SAME image sizes whose intermediates (rev / mota / sums / maps) this batch adopts
        instead of allocating its own -- the batches of one parity of a stream never have two stages in flight at once."""
        images = list(images)
        if not images:
            raise ValueError("RaggedBatch: empty batch")
        dev = require_gpu(*images)
        C = int(images[0].shape[2]) if images[0].dim() == 3 else -1
        for im in images:
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != C or not im.is_contiguous():
                raise TypeError("RaggedBatch: images must be contiguous uint8 [H,W,C] tensors with one channel count")
        self.images = images
        self.B, self.C, self.g = len(images), C, int(g)
        self.Ho, self.Wo = int(out_size[0]), int(out_size[1])
        self._dev = dev
        # the caller-side records (attwarp_ragged_image) as one structured array: pointers and sizes column by column
        rec = np.zeros(self.B, dtype=_RAGGED_IMAGE_DTYPE)
        rec["image"] = [im.data_ptr() for im in images]
        rec["H"] = hs = [int(im.shape[0]) for im in images]
        rec["W"] = ws = [int(im.shape[1]) for im in images]
        tx = [_axis_tables(self.g, w, dev) for w in ws]
        ty = [_axis_tables(self.g, h, dev) for h in hs]
        if any(t[2] != 8 for t in ty):
            raise _lib.AttWarpError("RaggedBatch: an image is too low for the 8-tap vertical mask up-sampling (H < 24)")
        rec["bounds_x"] = [t[0] for t in tx]; rec["kk_x"] = [t[1] for t in tx]; rec["ksize_x"] = [t[2] for t in tx]
        rec["bounds_y"] = [t[0] for t in ty]; rec["kk_y"] = [t[1] for t in ty]
        self._keep = [t[3:] for t in tx] + [t[3:] for t in ty]      # the coefficient tensors the table points to
        rp = ctypes.c_void_p(rec.ctypes.data)
        # host copy: a plain buffer this batch keeps (the entry point reads the header from it at every launch); the upload
        # goes through a pooled pinned staging buffer (allocating pinned memory per batch costs more than the five launches)
        shape = (rp, self.B, C, self.g, self.Ho, self.Wo)
        self.table_host, self.header = planned_table(("attwarp_ragged_table_bytes",) + shape, ("attwarp_ragged_plan",) + shape + (TABLE,),
                                                     _lib.RaggedHeader, _lib.AttWarpError, "attwarp_ragged_table_bytes: ")
        self.table_dev = uploaded(self.table_host, dev)
        h = self.header
        if share is not None:
            if (share.B, share.g, share.Ho, share.Wo, int(share.header.mota_bytes), int(share.header.sums_bytes)) != \
                    (self.B, self.g, self.Ho, self.Wo, int(h.mota_bytes), int(h.sums_bytes)) or share._dev != dev:
                raise ValueError("RaggedBatch: `share` must be a batch of the same image sizes on the same device")
            self.rev, self.mota, self.sums, self.map_x, self.map_y = share.rev, share.mota, share.sums, share.map_x, share.map_y
        else:
            self.rev = torch.empty(self.B, self.g, self.g, device=dev, dtype=torch.float32)
            self.mota = torch.empty(int(h.mota_bytes), device=dev, dtype=torch.uint8)
            self.sums = torch.empty(int(h.sums_bytes) // 8, device=dev, dtype=torch.float64)
            self.map_x = torch.empty(self.B, self.Wo, device=dev, dtype=torch.float32)
            self.map_y = torch.empty(self.B, self.Ho, device=dev, dtype=torch.float32)
        if out is None:
            out = torch.empty(self.B, self.Ho, self.Wo, C, device=dev, dtype=torch.uint8)
        elif tuple(out.shape) != (self.B, self.Ho, self.Wo, C) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
            raise ValueError("RaggedBatch: out must be a dense uint8 [B,H_out,W_out,C] tensor on the images' device")
        self.out = out
        self.masks = None                   # [B,g,g] float32: set by the caller before V runs

    @property
    def algorithmic_bytes(self) -> int:
        """Chain-level bytes of this batch: mask written + read (2 H W), image read (C H W), output written."""
        px = sum(int(i.shape[0]) * int(i.shape[1]) for i in self.images)
        return px * (2 + self.C) + self.B * self.Ho * self.Wo * self.C

    def mota_of(self, b: int) -> torch.Tensor:
        """The up-sampled uint8 mask [H_b,W_b] of image b (what blend_mask returns as ``mota_mask``, llava.py:253)."""
        rec = (_RaggedImageDev * self.B).from_address(self.table_host.ctypes.data + int(self.header.off_images))
        H, W = int(self.images[b].shape[0]), int(self.images[b].shape[1])
        off = int(rec[b].mota_off)
        return self.mota[off:off + H * W].view(H, W)


def upload_images(images, device=None):
    """A batch of host images as the reference's driver holds them (`b_images`: PIL images or uint8 [H,W,C] arrays of
    different sizes, main_batched.py:246) -> list of uint8 [H_i,W_i,C] GPU tensors: packed back to back into ONE staging
    buffer and copied with ONE host-to-device transfer (the ragged kernels take images at any byte address, so the views
    need no padding).  PIL images are taken as RGB; the warp does not depend on the channel order."""
    dev = torch.device(device) if device is not None else _lib.default_device()
    arrs = []
    for im in images:
        a = np.asarray(im.convert("RGB")) if hasattr(im, "convert") else np.asarray(im)
        if a.dtype != np.uint8 or a.ndim not in (2, 3):
            raise TypeError("upload_images: uint8 [H,W] / [H,W,C] arrays or PIL images expected")
        arrs.append(a[:, :, None] if a.ndim == 2 else a)
    sizes = [a.size for a in arrs]
    total = int(sum(sizes))
    host = np.empty(total, dtype=np.uint8)
    off = 0
    for a, n in zip(arrs, sizes):
        host[off:off + n] = a.reshape(-1)
        off += n
    return packed_views(uploaded(host, dev), [a.shape for a in arrs])


def upload_png_files(files_or_paths, device=None, all_formats=False, inflate="lane"):
    """:func:`upload_images` for a batch still in its PNG files (bytes-like or paths; the warped, overlay and attention-map
    files the drivers wrote, or anyone's 8-bit non-interlaced PNG): the COMPRESSED bytes go up in one transfer and are decoded
    on the GPU (attwarp_amd.png.decode_png) -> list of uint8 [H_i,W_i,3] RGB GPU tensors, views into one packed buffer, as
    ``Image.open(f).convert("RGB")`` gives them.  OSError for a broken file, ValueError for an unsupported one.
    ``all_formats=True`` also takes palette, 1- / 2- / 4- / 16-bit and Adam7-interlaced files (png.PngFiles: document scans and
    web graphics; 16-bit grey saturates as Pillow's does); without it they raise ValueError.
    ``inflate="wave"`` inflates every one-stream file (anything another encoder wrote) with a whole wave instead of one lane
    (png.PngFiles); the pixels do not depend on it."""
    return png.decode_png(files_or_paths, "RGB", "rgb", device, all_formats, inflate)


def upload_jpeg_files(files_or_paths, device=None, substreams="auto", progressive=False, all_layouts=False, all_scans=False,
                      scan_substreams=False, segment_bytes=None):
    """:func:`upload_images` for a batch still in its JPEG files (bytes-like or paths; the TextVQA / GQA images the drivers and
    the MarginalNet loader open, or anyone's baseline JPEG): the COMPRESSED bytes go up in one transfer and are decoded on
    the GPU (attwarp_amd.jpeg.decode_jpeg) -> list of uint8 [H_i,W_i,3] RGB GPU tensors, views into one packed buffer, as
    ``Image.open(f).convert("RGB")`` gives them.  OSError for a broken file, ValueError for an unsupported one.
    ``substreams``: marker-less files as self-synchronising sub-streams (jpeg.plan); the pixels do not depend on it.
    ``progressive=True`` also takes progressive files (jpeg.JpegFiles); without it they raise ValueError.
    ``all_layouts=True`` also takes CMYK / YCCK files, RGB-coded files and every sampling layout libjpeg decodes (4:4:0,
    4:1:1 ...; jpeg.JpegFiles); without it they raise ValueError.
    ``all_scans=True`` is the one switch for a folder somebody else made: both keywords, and also progressive files of those
    layouts (what web optimisers write from CMYK and rotated camera pictures) and sequential files of several scans.
    ``scan_substreams="auto"`` / True (opt-in) cuts the marker-less scans of plain progressive files into ``segment_bytes``
    decoded by one lane each (jpeg.plan); pixels and statuses do not depend on it."""
    return jpeg.decode_jpeg(files_or_paths, "RGB", "rgb", device, substreams, progressive, all_layouts, all_scans, scan_substreams,
                            segment_bytes)


def upload_image_files(files_or_paths, device=None, substreams="auto", progressive=False, all_formats=False, all_layouts=False,
                       all_scans=False, inflate="lane", scan_substreams=False, segment_bytes=None):
    """A batch of image files of either kind (bytes-like or paths), each sent by its signature to the PNG or the JPEG decoder
    (:func:`upload_png_files`, :func:`upload_jpeg_files`): one transfer and one decode per kind -> the uint8 [H_i,W_i,3] RGB
    GPU tensors in input order.  ValueError for a file that is neither.  ``progressive``, ``all_layouts``, ``all_scans``: see
    :func:`upload_jpeg_files`; ``all_formats``, ``inflate``: see :func:`upload_png_files`; ``scan_substreams``, ``segment_bytes``: see
    :func:`upload_jpeg_files`."""
    files = [file_bytes(f) for f in files_or_paths]
    kinds = []
    for i, f in enumerate(files):
        head = bytes(memoryview(f).cast("B")[:8])
        if head == b"\x89PNG\r\n\x1a\n":
            kinds.append("png")
        elif head[:2] == b"\xff\xd8":
            kinds.append("jpeg")
        else:
            raise ValueError(f"upload_image_files: file {i} is neither a PNG nor a JPEG file")
    decode = {"png": lambda f, d: upload_png_files(f, d, all_formats, inflate), "jpeg": lambda f, d: upload_jpeg_files(f, d, substreams, progressive, all_layouts, all_scans, scan_substreams, segment_bytes)}
    return per_kind(files, kinds, ("png", "jpeg"), lambda kind, group: decode[kind](group, device))


def ragged_chain_launch(R: Optional[RaggedBatch] = None, F: Optional[RaggedBatch] = None, P: Optional[RaggedBatch] = None,
                        L: Optional[RaggedBatch] = None, V: Optional[RaggedBatch] = None, enhance_coe=10, kernel_size=3,
                        transform="identity", exp_scale=1.0, exp_divisor=1.0, apply_inverse=False):
    """ONE launch of ``attwarp_mask_chain_ragged``: the resample of batch R, the map construction of F, the marginals of P,
    the mask up-sampling of L and revise_mask of V (``V.masks`` [B,g,g] float32) -- five different batches of a stream, or
    any subset (one batch alone: five launches, V -> L -> P -> F -> R).  ``transform`` .. ``apply_inverse``:
    save_warped_image's keyword arguments (new_method.py:405-411), used by P and F; unknown names mean identity (:400-403)."""
    some = next(b for b in (R, F, P, L, V) if b is not None)
    dev = some._dev
    transform, exp_scale, exp_divisor, apply_inverse = _transform_args(transform, exp_scale, exp_divisor, apply_inverse)
    lut = _tables.attention_transform_lut(transform, exp_scale, exp_divisor, dev) if P is not None else None
    def tab(b):
        return (None, None) if b is None else (b.table_host.ctypes.data, ptr(b.table_dev))
    if V is not None and (V.masks is None or V.masks.dtype != torch.float32 or tuple(V.masks.shape) != (V.B, V.g, V.g)
                          or not V.masks.is_contiguous() or V.masks.device != dev):
        raise ValueError("ragged_chain_launch: V.masks must be a dense float32 [B,g,g] tensor on the batch's device")
    with torch.cuda.device(dev):
        call("attwarp_mask_chain_ragged",
             *tab(R), ptr(R.out) if R else None, ptr(R.map_x) if R else None, ptr(R.map_y) if R else None,
             *tab(F), ptr(F.sums) if F else None, ptr(F.map_x) if F else None, ptr(F.map_y) if F else None,
             *tab(P), ptr(P.mota) if P else None, ptr(P.sums) if P else None,
             *tab(L), ptr(L.rev) if L else None, ptr(L.mota) if L else None,
             ptr(V.masks) if V else None, V.B if V else 0, some.g, int(kernel_size), float(enhance_coe), ptr(V.rev) if V else None,
             _lib.TRANSFORM_IDS[transform], exp_scale, exp_divisor, int(apply_inverse), ptr(lut),
             stream_ptr(dev))


def warp_from_masks_ragged(images, attn24: torch.Tensor, out_size=(500, 500), enhance_coe=10, kernel_size=3,
                           transform="identity", exp_scale=1.0, exp_divisor=1.0, apply_inverse=False, mode: str = "cv2",
                           return_batch: bool = False):
    """The ``main_batched.py:243-287`` chain for a batch of DIFFERENTLY sized images, as that driver holds them:
    ``images``: list of uint8 [H_i,W_i,C] GPU tensors (any sizes, any width -- 683 x 1024 like 1024 x 768); ``attn24``
    [B,24,24] -> dense uint8 [B,H_out,W_out,C].  Five launches for the whole batch (revise_mask, LANCZOS up-sampling to
    every image's own size, float64 marginals, CDF / np.interp maps, cv2 resample), each over all images at once.
    ``transform`` / ``exp_scale`` / ``exp_divisor`` / ``apply_inverse``: save_warped_image's own keyword arguments
    (new_method.py:405-411; the driver passes "identity", 1.0, 1.0, False); same signature as :func:`warp_from_masks`.
    Images outside the ragged kernel's limits (rows wider than 4096 bytes, sides <= 24 or > 8192) and ``mode="exact"``
    (the ragged resample is the integer cv2 one) run through :func:`warp_from_masks` one by one."""
    images = list(images)
    B = len(images)
    if B == 0:
        raise ValueError("warp_from_masks_ragged: empty batch")
    if attn24.dim() != 3 or attn24.shape[0] != B or attn24.shape[1] != attn24.shape[2]:
        raise ValueError("warp_from_masks_ragged: one square [g,g] map per image expected ([B,g,g])")
    dev = require_gpu(attn24, *images)
    if any(i.dim() != 3 or i.dtype != torch.uint8 for i in images):
        raise TypeError("warp_from_masks_ragged: images must be uint8 [H,W,C] tensors")
    C = int(images[0].shape[2])
    if any(int(i.shape[2]) != C for i in images):
        raise ValueError("warp_from_masks_ragged: the images of one batch must share their channel count "
                         f"(got {sorted({int(i.shape[2]) for i in images})}): the output is one dense [B,H_out,W_out,C] tensor")
    if mode not in ("cv2", "exact"):
        raise ValueError(f"warp_from_masks_ragged: unknown mode {mode!r}")
    g = int(attn24.shape[-1])
    Ho, Wo = int(out_size[0]), int(out_size[1])
    xf = dict(transform=transform, exp_scale=exp_scale, exp_divisor=exp_divisor, apply_inverse=apply_inverse)
    ok = [mode == "cv2" and ragged_eligible(int(i.shape[0]), int(i.shape[1]), C, g) for i in images]
    if Wo * C > RAGGED_MAX_ROW_BYTES:
        ok = [False] * B
    masks = attn24.float().contiguous()
    rb = None
    if all(ok):
        try:
            rb = RaggedBatch(images, out_size, g)
        except _lib.AttWarpError:          # a limit ragged_eligible does not model (e.g. the LDS of a very long axis): per image
            ok = [False] * B
    if rb is not None:
        rb.masks = masks
        for stage in "VLPFR":
            ragged_chain_launch(**{stage: rb}, enhance_coe=enhance_coe, kernel_size=kernel_size, **xf)
        return (rb.out, rb) if return_batch else rb.out
    out = torch.empty(B, Ho, Wo, C, device=dev, dtype=torch.uint8)
    idx = [b for b in range(B) if ok[b]]
    if idx:
        sub = warp_from_masks_ragged([images[b] for b in idx], masks[idx], out_size, enhance_coe, kernel_size, **xf)
        out[idx] = sub
    for b in range(B):
        if not ok[b]:
            out[b] = warp_from_masks(images[b][None], masks[b:b + 1], out_size, enhance_coe, kernel_size, mode=mode, **xf)[0]
    return (out, None) if return_batch else out


class RaggedMaskChainStream(_StepGraphs):
    """A stream of ragged batches, one launch per batch: R(k) | F(k+1) | P(k+2) | L(k+3) | V(k+4) of
    ``attwarp_mask_chain_ragged`` (the ragged twin of :class:`MaskChainStream`).

        st = RaggedMaskChainStream(out_size=(500, 500))
        for images, attn24 in batches:                 # lists of uint8 [H_i,W_i,3] GPU tensors, [B,24,24]
            done = st.push(images, attn24)             # -> the RaggedBatch whose resample was just enqueued (4 pushes back)
            if done is not None: use(done.out)
        for done in st.flush(): use(done.out)

    Every output equals :func:`warp_from_masks_ragged` on its batch, bit for bit (same stage bodies).  For steady-state
    measurements ``ring`` + ``run`` replay one launch per batch over prebuilt batches (optionally as HIP graphs)."""

    DEPTH = 4

    def __init__(self, out_size=(500, 500), enhance_coe=10, kernel_size=3, g: int = GRID, transform="identity", exp_scale=1.0,
                 exp_divisor=1.0, apply_inverse=False):
        self.out_size = (int(out_size[0]), int(out_size[1]))
        self.enhance_coe, self.kernel_size, self.g = float(enhance_coe), int(kernel_size), int(g)
        # save_warped_image's keyword arguments (new_method.py:405-411), constants of the stream
        self._xf = dict(zip(_TRANSFORM_KW, _transform_args(transform, exp_scale, exp_divisor, apply_inverse)))
        self._q = []                       # the batches in flight, oldest first: [k-4 .. k]

    def _stages(self, **stages):
        ragged_chain_launch(**stages, enhance_coe=self.enhance_coe, kernel_size=self.kernel_size, **self._xf)

    def _launch(self, q):
        """q: the five batches [R, F, P, L, V] of this step (None where the stream has none)."""
        if any(b is not None for b in q):
            self._stages(R=q[0], F=q[1], P=q[2], L=q[3], V=q[4])

    def _window(self):
        """The five [R, F, P, L, V] slots of a launch that takes the youngest batch in flight as V (None: no batch)."""
        return ([None] * (self.DEPTH + 1) + self._q)[-(self.DEPTH + 1):]

    def push(self, images, attn24: torch.Tensor, out: Optional[torch.Tensor] = None):
        rb = RaggedBatch(images, self.out_size, self.g, out=out)
        rb.masks = attn24.float().contiguous()
        self._q.append(rb)
        self._launch(self._window())
        if len(self._q) > self.DEPTH:
            return self._q.pop(0)
        return None

    def flush(self):
        """The launches that finish the batches still in flight; returns them oldest first."""
        done = []
        # the youngest batch in flight has had V only, the one before it V and L, ...: one launch moves every batch one
        # stage on ([R, F, P, L, V] slots, oldest first)
        q = self._window()[1:] + [None]
        while any(b is not None for b in q):
            self._launch(q)
            if q[0] is not None:
                done.append(q[0])
            q = q[1:] + [None]
        self._q = []
        return done

    # ---- steady state over prebuilt batches (measurement, or a producer that stays ahead of the ring) ----
    def ring(self, batches):
        """Adopt n >= 5 prebuilt RaggedBatch objects (tables on the device, ``masks`` set) as a ring: step k runs
        R(k) | F(k+1) | P(k+2) | L(k+3) | V(k+4) on slots k % n .. (k+4) % n."""
        self._ring = list(batches)
        if len(self._ring) < self.DEPTH + 1:
            raise ValueError("RaggedMaskChainStream.ring: at least 5 batches")
        self.k = 0
        self._init_graphs(self._ring[0]._dev)          # (the graphs belong to this ring: a new ring starts without any)

    def prime(self):
        """Run V..F of the first four ring slots serially, so that step 0 finds what it expects."""
        r = self._ring
        _ragged_serial(_RAGGED_FILL, 0, lambda st, j: self._stages(**{st: r[j]}))

    def _step(self, k, main=None):
        r, n = self._ring, len(self._ring)
        self._launch([r[(k + i) % n] for i in range(self.DEPTH + 1)])

    _graph_step = _step

    def _graph_start(self):
        return self.k % len(self._ring), self.k              # the batches of a step depend on k mod n

    def _advance(self, m):
        self.k += m

    @staticmethod
    def round_unroll(unroll: int, n: int) -> int:
        """The graph length run() uses over a ring of n batches: whole turns of the ring (at least one); 0: no graphs."""
        return n * max(1, unroll // n) if unroll > 0 else 0

    def run(self, n_steps: int, unroll: int = 0):
        """n_steps launches over the ring; unroll > 0: replayed as HIP graphs of ``unroll`` steps (one host call each)."""
        for _ in range(self._run_graphs(n_steps, self.round_unroll(unroll, len(self._ring)))):
            self._step(self.k)
            self.k += 1

    def drain_ring(self):
        """Finish the four batches in flight behind the last step, serially (their outputs then equal the stream's)."""
        r, n = self._ring, len(self._ring)
        _ragged_serial(_RAGGED_DRAIN, self.k, lambda st, j: self._stages(**{st: r[j % n]}))
        self.k += self.DEPTH


# ---- Jet heat-map overlays (blend_mask's merged image, save_warped_image's masked overlay) ----
_OVERLAY_IMAGE_DTYPE = np.dtype(_lib.OverlayImage)     # attwarp_overlay_image as a record array
OVERLAY_STYLES = {"blend_mask": _lib.OVERLAY_BLEND_MASK, "save_warped": _lib.OVERLAY_SAVE_WARPED}
_CHANNEL_ORDERS = {"rgb": _lib.RGB, "bgr": _lib.BGR}


def _overlay_launch(images, maps, outs, alpha, style, order, out_order):
    """ONE attwarp_heatmap_overlay call: lists of uint8 [H,W,3] images, [H,W] maps (one dtype: uint8 / float32 / float64)
    and uint8 [H,W,3] outputs, any sizes.  The records go to the device through the pooled pinned staging buffer."""
    if style not in OVERLAY_STYLES:
        raise ValueError(f"heatmap_overlay: style must be one of {sorted(OVERLAY_STYLES)}")
    out_order = order if out_order is None else out_order
    if order not in _CHANNEL_ORDERS or out_order not in _CHANNEL_ORDERS:
        raise ValueError("heatmap_overlay: channel orders are 'rgb' or 'bgr'")
    B = len(images)
    if B == 0 or len(maps) != B or len(outs) != B:
        raise ValueError("heatmap_overlay: one map and one output per image, at least one image")
    dev = require_gpu(*images, *maps, *outs)
    mdt = maps[0].dtype
    if mdt not in (torch.uint8, torch.float32, torch.float64) or any(m.dtype != mdt for m in maps):
        raise TypeError("heatmap_overlay: the maps of one call share one dtype: uint8, float32 or float64")
    for im, m, o in zip(images, maps, outs):
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_contiguous():
            raise TypeError("heatmap_overlay: images must be contiguous uint8 [H,W,3] tensors")
        if m.dim() != 2 or tuple(m.shape) != tuple(im.shape[:2]) or not m.is_contiguous():
            raise ValueError(f"heatmap_overlay: map {tuple(m.shape)} must be a contiguous [H,W] tensor of the image's size "
                             f"{tuple(im.shape[:2])}")
        if o.dtype != torch.uint8 or o.shape != im.shape or not o.is_contiguous():
            raise ValueError("heatmap_overlay: outputs must be contiguous uint8 tensors of the images' shapes")
    rec = np.zeros(B, dtype=_OVERLAY_IMAGE_DTYPE)
    rec["image"] = [t.data_ptr() for t in images]
    rec["map"] = [t.data_ptr() for t in maps]
    rec["out"] = [t.data_ptr() for t in outs]
    rec["H"] = [int(t.shape[0]) for t in images]
    rec["W"] = [int(t.shape[1]) for t in images]
    _overlay_call(rec, dev, _lib.dtype_id(maps[0]), style, alpha, order, out_order)


def _overlay_call(rec: np.ndarray, dev: torch.device, map_dtype: int, style, alpha, order, out_order):
    """attwarp_heatmap_overlay on host records (attwarp_overlay_image); the device copy goes through the pooled pinned
    staging buffer, the workspace comes from the caching allocator (both stream ordered)."""
    B = int(rec.shape[0])
    lib = _lib.load()
    with torch.cuda.device(dev):
        rec_dev = uploaded(rec, dev)
        ws = torch.empty(lib.attwarp_overlay_workspace_bytes(B), device=dev, dtype=torch.uint8)
        call("attwarp_heatmap_overlay", rec.ctypes.data, ptr(rec_dev), B, map_dtype, OVERLAY_STYLES[style],
             float(alpha), _CHANNEL_ORDERS[order], _CHANNEL_ORDERS[out_order], ptr(ws), stream_ptr(dev))


def heatmap_overlay(images, maps, alpha: float = 0.5, style: str = "blend_mask", order: str = "rgb",
                    out_order: Optional[str] = None):
    """Jet heat-map overlays of a batch in one call (two launches), on the GPU:

        style="blend_mask"   blend_mask's merged image (llava.py:254-269): cv2.normalize(NORM_MINMAX) of the uint8 mask,
                             COLORMAP_JET, addWeighted(image, 1 - alpha, heat, alpha, 0)      -- uint8 maps only
        style="save_warped"  save_warped_image's masked overlay (new_method.py:455-475): min-max in the map's dtype with
                             EPSILON = 1e-9, COLORMAP_JET, addWeighted(heat, alpha, image, 1 - alpha, 0)

    ``images``: uint8 [B,H,W,3] with ``maps`` [B,H,W] (dense batch -> dense [B,H,W,3]), or lists of uint8 [H_i,W_i,3] and
    [H_i,W_i] GPU tensors of any sizes (-> list of [H_i,W_i,3]).  Maps: uint8, float32 or float64, one dtype per call, at the
    images' sizes.  ``order`` / ``out_order``: channel order of the images / of the result ("rgb" or "bgr"; the result
    defaults to the images' order).  Arithmetic: DESIGN.md "Heat-map overlay" (bit-exact with the numpy restatement of
    tests/overlay_ref.py; OpenCV itself is pinned where it is installed, exact at alpha = 0.5)."""
    if isinstance(images, torch.Tensor):
        if images.dim() != 4 or not isinstance(maps, torch.Tensor) or maps.dim() != 3 or maps.shape[0] != images.shape[0]:
            raise ValueError("heatmap_overlay: a dense batch is images [B,H,W,3] with maps [B,H,W]")
        images, maps = images.contiguous(), maps.contiguous()
        out = torch.empty_like(images)
        _overlay_launch([images[b] for b in range(images.shape[0])], [maps[b] for b in range(maps.shape[0])],
                        [out[b] for b in range(out.shape[0])], alpha, style, order, out_order)
        return out
    images, maps = list(images), list(maps)
    outs = [torch.empty_like(im) for im in images]
    _overlay_launch(images, maps, outs, alpha, style, order, out_order)
    return outs


def heatmap_overlay_ragged(rb: RaggedBatch, alpha: float = 0.5, order: str = "rgb", out_order: Optional[str] = None):
    """blend_mask's merged images for every image of a ragged batch, from the up-sampled masks the chain already holds
    (``rb.mota``, read in place through :meth:`RaggedBatch.mota_of`: no copy) -> ``(packed, views)``: one uint8 buffer
    and the [H_i,W_i,3] view of each image in it (images at 16-byte aligned offsets).  ``alpha``: blend_mask's alpha (0.5
    for both reference drivers).  ``order``: channel order of ``rb.images`` (upload_images gives RGB).

    When to enqueue it: after the launch that ran the batch's L stage (mask up-sampling) and before anything overwrites
    ``rb.mota``.  A batch of :func:`warp_from_masks_ragged` (``return_batch=True``) or one returned by
    :meth:`RaggedMaskChainStream.push` / ``flush`` owns its masks: any time later on the same stream.  The batches of one
    parity of ``MaskChainStream(pattern="ragged")`` SHARE one mask buffer (``RaggedBatch(share=...)``): batch j's mask is
    written by step j - 3 (L(j)) and overwritten by step j - 1 (L(j + 2)), so its overlay goes right after step j - 3 or
    step j - 2, with batch j's images already in their ring slot."""
    B = rb.B
    if rb.C != 3:
        raise ValueError("heatmap_overlay_ragged: three-channel images only")
    out_order = order if out_order is None else out_order
    if order not in _CHANNEL_ORDERS or out_order not in _CHANNEL_ORDERS:
        raise ValueError("heatmap_overlay_ragged: channel orders are 'rgb' or 'bgr'")
    # the records straight from the batch's table (mota_off of every image): no per-image tensor on the launch path
    tab = (_RaggedImageDev * B).from_address(rb.table_host.ctypes.data + int(rb.header.off_images))
    rec = np.zeros(B, dtype=_OVERLAY_IMAGE_DTYPE)
    rec["image"] = [im.data_ptr() for im in rb.images]
    rec["H"] = [int(t.H) for t in tab]
    rec["W"] = [int(t.W) for t in tab]
    npx = rec["H"].astype(np.int64) * rec["W"]
    rec["map"] = rb.mota.data_ptr() + np.array([int(t.mota_off) for t in tab], dtype=np.int64)
    sizes = (3 * npx + 15) // 16 * 16                    # outputs at 16-byte aligned offsets
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    packed = torch.empty(int(sizes.sum()), device=rb._dev, dtype=torch.uint8)
    rec["out"] = packed.data_ptr() + offs
    _overlay_call(rec, rb._dev, _lib.U8, "blend_mask", alpha, order, out_order)
    views = [packed[o:o + 3 * n].view(h, w, 3) for o, n, h, w in zip(offs.tolist(), npx.tolist(), rec["H"].tolist(), rec["W"].tolist())]
    return packed, views


def _ragged_images_to_save(rb: RaggedBatch, paths, what: str, order: str, who: str):
    """What ``save_png_ragged`` / ``save_jpeg_ragged`` (``who``) write: ``(paths, images, their channel order)``."""
    paths = list(paths)
    if len(paths) != rb.B:
        raise ValueError(f"{who}: {len(paths)} paths for a batch of {rb.B}")
    if what == "warped":
        if rb.C not in (1, 3):
            raise ValueError(f"{who}: one- or three-channel images only")
        return paths, rb.out, order
    if what == "mota":
        return paths, [rb.mota_of(b) for b in range(rb.B)], "rgb"
    raise ValueError(f"{who}: what is 'warped' or 'mota'")


def save_png_ragged(rb: RaggedBatch, paths, what: str = "warped", filter: str = "sub", order: str = "rgb", match="rle"):
    """The file-writing leg of the driver loop (main_batched.py:243-303) for a whole ragged batch: the warped images
    (``what="warped"``: ``rb.out``) or the up-sampled masks (``what="mota"``: :meth:`RaggedBatch.mota_of`, grey files) of
    ``rb`` as PNG files, encoded on the GPU in one :class:`attwarp_amd.png.PngBatch` -- only compressed bytes are copied
    to the host.  Enqueue it after the launches that produced what it saves; ``order``: channel order of ``rb.images``;
    ``match``: "rle" / "lz", one value or one per image (:class:`attwarp_amd.png.PngBatch`)."""
    paths, images, order = _ragged_images_to_save(rb, paths, what, order, "save_png_ragged")
    png.write_png(paths, images, filter=filter, order=order, match=match)


def save_jpeg_ragged(rb: RaggedBatch, paths, what: str = "warped", quality=75, subsampling="4:2:0", restart_rows=0,
                     order: str = "rgb", optimize=False, progressive=False):
    """:func:`save_png_ragged` for JPEG files: the warped images (``what="warped"``) or the up-sampled masks (``what="mota"``,
    grey files) of ``rb``, encoded on the GPU in one :class:`attwarp_amd.jpeg.JpegBatch` with the bytes ``Image.save`` would
    write (Pillow's defaults; ``restart_rows=1`` is what this project's reader decodes fastest).  ``order``: channel order
    of ``rb.images``.  ``optimize``: the images' own Huffman tables, the files of ``Image.save(..., optimize=True)``;
    ``progressive``: those of ``Image.save(..., progressive=True)``."""
    paths, images, order = _ragged_images_to_save(rb, paths, what, order, "save_jpeg_ragged")
    jpeg.write_jpeg(paths, images, quality, subsampling, restart_rows, order, optimize, progressive)
