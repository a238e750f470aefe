"""The trainer's debug and validation panels, built on the GPU (csrc/panel.hip): the visual debug block of
the training step (MN/trainer.py:283-337) and its twin in validation (:455-517).  ONE launch normalises and up-samples the
attention heat on the fly, converts floats to bytes as ``(x * 255).byte()`` does and lays the first ``n`` samples of every
row out as ``torchvision.utils.make_grid`` does, straight into one uint8 canvas; the grid file and every per-sample file are
then encoded from that one buffer by one :class:`attwarp_amd.png.PngBatch` (the per-sample files are views into the grid).
Only compressed bytes cross to the host.

Values: the byte is torch's wherever ``(t).byte()`` is defined (``-1 < t < 256``).  Outside that range torch's float to
uint8 cast is undefined (and differs between its CPU and GPU kernels); here ``t <= -1`` gives 0, ``t >= 256`` gives 255
and NaN gives 0, so a heat image whose maximum is NaN or +inf is all zeros.  float32 and uint8 sources only (the trainer's
tensors at this point are float32): anything else raises TypeError.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from ._lib import call, stream_ptr

PANEL_MAX_SRC = _lib.PANEL_MAX_SRC          # row sources of one call at most
PANEL_MAX_HEAT = _lib.PANEL_MAX_HEAT        # h * w of a heat source at most (one float32 tile in LDS)
_LAYOUTS = {"hwc": _lib.HWC, "chw": _lib.CHW}


class Heat:
    """Marks a low-resolution float32 ``[N, 1, h, w]`` tensor as a heat source: per image ``A / (A.amax() + 1e-6)``,
    up-sampled (or down-sampled) to the cell size with torch's bilinear, ``align_corners=False``; ``h * w`` is at most
    :data:`PANEL_MAX_HEAT`."""

    def __init__(self, A: torch.Tensor):
        self.A = A


def grid_geometry(K: int, H: int, W: int, nrow: int, padding: int = 2, right_margin: int = 0):
    """``make_grid``'s geometry for K cells of H x W -> (xmaps, ymaps, padding used, Hg, Wg + right_margin).  A single
    cell is returned bare (padding 0), as ``make_grid`` returns a single image."""
    pad = 0 if K == 1 else padding
    xmaps = min(nrow, K)
    ymaps = -(-K // xmaps)
    return xmaps, ymaps, pad, ymaps * (H + pad) + pad, xmaps * (W + pad) + pad + right_margin


def _source(row, clamp: bool):
    """One row -> (PanelSource fields, (H, W) or None for a heat row, the tensor)."""
    heat = isinstance(row, Heat)
    t = row.A if heat else row
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"panels: a row is a tensor or Heat(tensor), got {type(row).__name__}")
    if t.dtype != torch.float32 and (heat or t.dtype != torch.uint8):
        raise TypeError(f"panels: {'a heat row is float32' if heat else 'rows are float32 or uint8'}, got {t.dtype}")
    if t.dim() != 4 or (heat and t.shape[1] != 1) or t.shape[1] not in (1, 3):
        raise ValueError(f"panels: rows are [N,3,H,W] / [N,1,H,W], heat rows [N,1,h,w]; got {tuple(t.shape)}")
    N, C, H, W = (int(v) for v in t.shape)
    if min(N, H, W) < 1:
        raise ValueError(f"panels: zero size in {tuple(t.shape)}")
    if not t[0].is_contiguous():
        raise ValueError(f"panels: the planes of an image must be dense (strides {t.stride()} for {tuple(t.shape)})")
    kind = _lib.PANEL_HEAT if heat else (_lib.PANEL_U8 if t.dtype == torch.uint8 else _lib.PANEL_F32)
    stride = int(t.stride(0)) if N > 1 else C * H * W
    if stride < C * H * W:
        raise ValueError(f"panels: batch stride {stride} below the {C * H * W} elements of an image")
    rec = dict(data=t.data_ptr(), batch_stride=stride, kind=kind, C=C, N=N, h=H if heat else 0, w=W if heat else 0,
               clamp=int(bool(clamp)) if kind == _lib.PANEL_F32 else 0)
    return rec, (None if heat else (H, W)), t


def make_grid_u8(rows: Sequence[Union[torch.Tensor, Heat]], n: Optional[int] = None, nrow: Optional[int] = None,
                 padding: int = 2, pad_value: int = 0, layout: str = "hwc", clamp: Union[bool, Sequence[bool]] = False,
                 right_margin: int = 0, out: Optional[torch.Tensor] = None, size: Optional[Tuple[int, int]] = None,
                 for_png: bool = False) -> torch.Tensor:
    """``make_grid((torch.cat([row[:n] for row in rows]) * 255).byte(), nrow, padding, pad_value)`` in one launch ->
    uint8 ``[Hg, Wg + right_margin, 3]`` (``layout="hwc"``: what ``Image.fromarray(grid.permute(1, 2, 0))`` holds and what
    ``PngBatch`` reads) or ``[3, Hg, Wg + right_margin]`` (``"chw"``: what ``make_grid`` returns).

    ``rows``: float32 or uint8 ``[N,3,H,W]`` / ``[N,1,H,W]`` tensors (one channel fills all three; uint8 is copied; a
    slice of a larger batch is read where it lies) and :class:`Heat` rows; at most :data:`PANEL_MAX_SRC`.  ``n``: images
    taken from every row (default: the smallest N); ``nrow``: cells per grid row (default ``n``).  ``clamp``: clamp float
    values to [0, 1] first, one flag or one per row.  ``right_margin``: extra columns of ``pad_value`` (room for the
    validation panel's text: paste a uint8 image there with ``copy_``).  ``size``: the cell size when every row is a heat
    row.  ``out``: a dense uint8 tensor of the result's shape.  ``for_png``: also refuse a canvas too wide for the PNG
    encoder.  Out-of-range values saturate and NaN gives 0 (module docstring).  Limits raise before any launch; no
    argument depends on device data, so a call can be captured in a graph."""
    rows = list(rows)
    if not rows:
        raise ValueError("make_grid_u8: no rows")
    if layout not in _LAYOUTS:
        raise ValueError(f"make_grid_u8: layout must be one of {sorted(_LAYOUTS)}")
    clamps = [clamp] * len(rows) if isinstance(clamp, bool) else list(clamp)
    if len(clamps) != len(rows):
        raise ValueError(f"make_grid_u8: {len(clamps)} clamp flags for {len(rows)} rows")
    parsed = [_source(r, c) for r, c in zip(rows, clamps)]
    sizes = {hw for _, hw, _ in parsed if hw is not None}
    if size is not None:
        sizes.add((int(size[0]), int(size[1])))
    if len(sizes) != 1:
        raise ValueError(f"make_grid_u8: one cell size is needed, got {sorted(sizes)} (size= names it when every row is a heat row)")
    H, W = sizes.pop()
    dev = _lib.require_gpu(*[t for _, _, t in parsed])
    if n is None:
        n = min(rec["N"] for rec, _, _ in parsed)
    n = int(n)
    nrow = n if nrow is None else int(nrow)
    recs = (_lib.PanelSource * len(parsed))(*[_lib.PanelSource(**rec) for rec, _, _ in parsed])
    if n >= 1 and nrow >= 1 and padding >= 0 and right_margin >= 0:
        _, _, _, Hg, Wt = grid_geometry(len(parsed) * n, H, W, nrow, int(padding), int(right_margin))
    else:
        Hg = Wt = 1                        # (the entry point refuses these; nothing is written)
    shape = (Hg, Wt, 3) if layout == "hwc" else (3, Hg, Wt)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(shape, device=dev, dtype=torch.uint8)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"make_grid_u8: out must be a dense uint8 tensor of shape {shape} on the rows' device")
        call("attwarp_panel_grid", recs, len(parsed), n, H, W, nrow, int(padding), int(pad_value), _LAYOUTS[layout],
             int(right_margin), _lib.PANEL_FOR_PNG if for_png else 0, _lib.ptr(out), stream_ptr(dev))
    return out


def trainer_debug_grid(img: torch.Tensor, A: torch.Tensor, warps: Sequence[torch.Tensor], num_vis: int = 4,
                       right_margin: int = 0, for_png: bool = False):
    """The panel of MN/trainer.py:301-307 (two warps: ``Wimg``, ``Wimg_gt``) and :484-517 (three: ``Wimg_gt_orig`` too) ->
    ``(grid, cells)``: ``grid`` is the uint8 HWC canvas of rows ``[img, Heat(A), *warps]``, ``n = min(num_vis, B)`` cells
    each, and ``cells[r][i]`` the ``[H, W, 3]`` strided view of cell ``(r, i)`` in it.

    Everything is sliced ``[:n]`` before anything is computed: the heat of the other samples is never built.  Do the same
    at the call site -- ``warp_from_cdf_torch(img[:n], Fx[:n], Fy[:n])`` -- the reference's whole-batch warps are the
    larger half of what its block wastes.  The warps may hold just those ``n`` samples or the whole batch.  The warp rows
    are clamped to [0, 1] as the trainer clamps them (for the bytes that is what the value policy does anyway)."""
    warps = list(warps)
    n = min(int(num_vis), int(img.shape[0]))
    if n < 1:
        raise ValueError("trainer_debug_grid: empty batch or num_vis < 1")
    rows = [img[:n], Heat(A[:n])] + [w[:n] for w in warps]
    grid = make_grid_u8(rows, n=n, nrow=n, layout="hwc", clamp=[False, False] + [True] * len(warps),
                        right_margin=right_margin, for_png=for_png)
    H, W = int(img.shape[-2]), int(img.shape[-1])
    _, _, pad, _, _ = grid_geometry(len(rows) * n, H, W, n)
    cells = [[grid[r * (H + pad) + pad: r * (H + pad) + pad + H, i * (W + pad) + pad: i * (W + pad) + pad + W]
              for i in range(n)] for r in range(len(rows))]
    return grid, cells


def write_trainer_debug(grid_path, sample_paths, img: torch.Tensor, A: torch.Tensor, warps: Sequence[torch.Tensor],
                        num_vis: int = 4, filter: str = "sub", match="rle") -> List:
    """The files of MN/trainer.py:305-325: the grid (``grid_path``) and, per sample ``i < min(num_vis, B)``, the cells of
    ``warps[0]`` (``Wimg``) and ``warps[1]`` (``Wimg_gt``) -- ``sample_paths[i] = (pred_path, gt_path)``; they hold
    ``(W[i].clamp(0, 1) * 255).byte()``.  One panel launch, then ONE ``PngBatch`` over the grid and its cell views; only
    compressed bytes are downloaded (``match``: :class:`attwarp_amd.png.PngBatch`, one value or one per file, the grid's
    first).  Returns the paths written, the grid's first.  Slice the warps at the call site:
    ``warp_from_cdf_torch(img[:n], Fx[:n], Fy[:n])`` (see :func:`trainer_debug_grid`)."""
    from . import png
    warps = list(warps)
    if len(warps) < 2:
        raise ValueError("write_trainer_debug: warps = (Wimg, Wimg_gt, ...) -- the per-sample files are cells of the first two")
    n = min(int(num_vis), int(img.shape[0]))
    sample_paths = [tuple(p) for p in sample_paths]
    if len(sample_paths) < n or any(len(p) != 2 for p in sample_paths):
        raise ValueError(f"write_trainer_debug: {n} (pred_path, gt_path) pairs are needed")
    grid, cells = trainer_debug_grid(img, A, warps, num_vis, for_png=True)
    images, paths = [grid], [grid_path]
    for i in range(n):
        images += [cells[2][i], cells[3][i]]
        paths += list(sample_paths[i])
    files = png.download(*png.PngBatch(images, filter, match=match).run())
    for p, f in zip(paths, files):
        with open(p, "wb") as fh:
            fh.write(f)
    return paths
