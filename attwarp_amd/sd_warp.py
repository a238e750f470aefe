"""Drop-in for the compute of ``Ablations/Stable_diffusion_based_warp.py`` (the Stable-Diffusion warp ablation): token
importance and the token-selected attention map from captured UNet cross-attention (:310-402), ``cv2.resize(...,
INTER_CUBIC)`` / ``cv2.GaussianBlur`` / min-max of the map (:159-160, :396-401, :407-413) and the iterated warp (:142-172,
:445-456), on the GPU.

* :func:`reduce_captured_maps` reads every captured tensor ``[B,heads,H,W,tokens]`` ONCE (one ``attwarp_xattn_reduce`` call
  per dtype over the whole dict): the per-token sums of every tensor, and for the requested layers ``hw_tok`` =
  ``attn.sum(0).sum(0)`` (``B * heads`` times smaller than the tensor), from which any token selection follows:
  ``attn[..., idx].sum(0).sum(0).sum(-1) == hw_tok[..., idx].sum(-1)``.  :func:`compute_token_importance` and
  :func:`aggregate_attention_map_for_tokens` keep the reference's signatures and also accept that result, so a run reads the
  captured tensors once.  The host math on the ``[tokens]`` vectors is the reference's numpy, line for line.
* :func:`resize_cubic`, :func:`minmax_normalize`, :func:`blur5_normalize`: the map arithmetic for ragged batches of float32
  device maps (OpenCV's published algorithms restated; bit-exact with tests/sdwarp_ref.py).
* :func:`iterative_warp`: ``run``'s loop (:445-456) for a batch of differently sized images without leaving the device.
* ``set_transform_function``, ``resize_image_to_match_attmap``, ``warp_image_by_attention``, ``save_warped_image``,
  ``save_warped_image_original``, ``upsample_attention_map``: the ablation's numpy / file facing names (the module's default
  transform is identity, unlike ``new_method``).  Image I/O reuses ``new_method``'s helpers (Pillow, BGR in memory).

Not here: ``load_pipeline``, ``encode_image``, ``get_text_embeddings``, ``truncated_ddim_inversion``,
``forward_and_capture`` and ``run`` drive ``diffusers`` and the external ``attention_map_diffusers`` package; keep the
reference's own.  There is no CPU path: captured tensors and maps must be GPU tensors.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, _tables
from . import new_method as _nm
from ._lib import call, ptr, require_gpu, stream_ptr
from .grounding import _packed, _upload_records

EPSILON = 1e-9
BASE_ATTENTION = 1e-9
ATTENTION_TRANSFORM = "identity"      # reference default (:59)
EXP_SCALE = 1.0
EXP_DIVISOR = 1.0
APPLY_INVERSE_TO_MARGINALS = False

_KNOWN = ("identity", "square", "sqrt", "exp", "log")
_MAX_RECORDS, _MAX_SIDE, _MAX_TOKENS = 65535, 1 << 15, 256

_XATTN_DTYPE = np.dtype([("attn", "<u8"), ("token_sums", "<u8"), ("hw_tok", "<u8"), ("B", "<i4"), ("heads", "<i4"),
                         ("HW", "<i4"), ("pad", "<i4")])
_CUBIC_DTYPE = np.dtype([("src", "<u8"), ("out", "<u8"), ("ofs_x", "<u8"), ("coef_x", "<u8"), ("ofs_y", "<u8"),
                         ("coef_y", "<u8"), ("h", "<i4"), ("w", "<i4"), ("H", "<i4"), ("W", "<i4")])
_F32MAP_DTYPE = np.dtype([("src", "<u8"), ("out", "<u8"), ("H", "<i4"), ("W", "<i4")])
assert _XATTN_DTYPE.itemsize == 40 and _CUBIC_DTYPE.itemsize == 64 and _F32MAP_DTYPE.itemsize == 24


def set_transform_function(transform_name, exp_scale=1.0, exp_divisor=1.0, apply_inverse=False):
    """Reference :61-80: select the attention transform; unknown names fall back to identity (the NAME is returned as
    given, as in the reference)."""
    global ATTENTION_TRANSFORM, EXP_SCALE, EXP_DIVISOR, APPLY_INVERSE_TO_MARGINALS
    EXP_SCALE = exp_scale
    EXP_DIVISOR = exp_divisor
    APPLY_INVERSE_TO_MARGINALS = apply_inverse
    ATTENTION_TRANSFORM = transform_name if transform_name in _KNOWN else "identity"
    return transform_name


def resize_image_to_match_attmap(image, att_map):
    """Reference :82-91 (``cv2.resize(image, (aw, ah), INTER_LINEAR)``; a copy when the sizes match)."""
    return _nm.resize_image_to_match_attmap(image, att_map, "cv2")


def warp_image_by_attention(image, att_map, new_width, new_height):
    """Reference :93-140 with the module state set by :func:`set_transform_function`: image [h,w,3] uint8, att_map [h,w]
    (uint8 / float32 / float64) -> warped [new_height,new_width,3]."""
    if image is None or att_map is None:
        return None
    dev = _lib.default_device()
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise TypeError(f"warp_image_by_attention: a uint8 [h,w,c] image is expected, got {img.dtype} {img.shape}")
    att = _nm._att_to_device(att_map, dev)
    if att.dim() != 2 or tuple(att.shape) != img.shape[:2]:
        raise ValueError(f"attention map {tuple(att.shape)} must match image {img.shape[:2]}")
    mx, my = _axis_maps(att.unsqueeze(0), int(new_width), int(new_height), ATTENTION_TRANSFORM, EXP_SCALE, EXP_DIVISOR,
                        APPLY_INVERSE_TO_MARGINALS)
    out = _nm.remap_hwc(torch.from_numpy(np.ascontiguousarray(img)).to(dev).unsqueeze(0), mx, my, "cv2")[0]
    return out.cpu().numpy()


# ---- the captured cross-attention, read once -------------------------------------------------------------------------
def xattn_chunk(tokens: int) -> int:
    """Positions of HW one workgroup of ``attwarp_xattn_reduce`` owns (fixes the summation order of ``token_sums``)."""
    c = _lib.load().attwarp_xattn_chunk(int(tokens))
    if c <= 0:
        raise ValueError(f"xattn_chunk: tokens={tokens} outside 1 .. {_MAX_TOKENS}")
    return c


def xattn_reduce(tensors: Sequence[torch.Tensor], want_hw_tok: Sequence[bool]):
    """``attwarp_xattn_reduce`` on tensors ``[B,heads,HW,tokens]`` (or ``[B,heads,H,W,tokens]``) of ONE dtype (float32,
    float16, bfloat16) and one ``tokens``: -> (token_sums [M,tokens] device tensor in the dtype, list of hw_tok [HW,tokens]
    device tensors or None).  Dense tensors only (element alignment is enough: a view at an odd element offset is fine)."""
    tensors = list(tensors)
    want = [bool(w) for w in want_hw_tok]
    M = len(tensors)
    if len(want) != M:
        raise ValueError(f"xattn_reduce: {len(want)} hw_tok flags for {M} tensors")
    if not 0 < M <= _MAX_RECORDS:
        raise ValueError(f"xattn_reduce: 1 .. {_MAX_RECORDS} tensors per call, got {M}")
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("xattn_reduce: captured maps must be GPU tensors (there is no CPU path)")
    dev = require_gpu(*tensors)
    dt, tokens = tensors[0].dtype, int(tensors[0].shape[-1])
    if dt not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"xattn_reduce: float32, float16 or bfloat16 tensors expected, got {dt}")
    if not 1 <= tokens <= _MAX_TOKENS:
        raise ValueError(f"xattn_reduce: tokens={tokens} outside 1 .. {_MAX_TOKENS}")
    rec = np.zeros(M, dtype=_XATTN_DTYPE)
    keep = []
    for m, t in enumerate(tensors):
        if t.dtype != dt or t.dim() not in (4, 5) or int(t.shape[-1]) != tokens:
            raise ValueError(f"xattn_reduce: tensor {m}: {t.dtype} {tuple(t.shape)}; one dtype and one token count per call, "
                             f"[B,heads,HW,tokens] or [B,heads,H,W,tokens]")
        if t.numel() == 0:
            raise ValueError(f"xattn_reduce: tensor {m} is empty")
        t = t.detach()
        if not t.is_contiguous():
            t = t.contiguous()
        keep.append(t)
        rec["attn"][m] = t.data_ptr()
        rec["B"][m], rec["heads"][m] = t.shape[0], t.shape[1]
        rec["HW"][m] = int(np.prod(t.shape[2:-1]))
    es = keep[0].element_size()
    sums = torch.empty(M, tokens, device=dev, dtype=dt)
    rec["token_sums"] = sums.data_ptr() + es * tokens * np.arange(M, dtype=np.int64)
    n_hw = np.where(want, rec["HW"].astype(np.int64) * tokens, 0)
    offs = np.concatenate([[0], np.cumsum(n_hw)[:-1]]).astype(np.int64)
    buf = torch.empty(int(n_hw.sum()), device=dev, dtype=dt)
    rec["hw_tok"] = np.where(want, buf.data_ptr() + es * offs, 0)
    hw = [buf[o:o + n].view(int(r["HW"]), tokens) if w else None for o, n, w, r in zip(offs.tolist(), n_hw.tolist(), want, rec)]
    lib = _lib.load()
    with torch.cuda.device(dev):
        rec_dev = _upload_records(rec, dev)
        ws = torch.empty(max(16, lib.attwarp_xattn_reduce_workspace_bytes(rec.ctypes.data, M, tokens)), device=dev, dtype=torch.uint8)
        call("attwarp_xattn_reduce", rec.ctypes.data, ptr(rec_dev), M, _lib.dtype_id(keep[0]), tokens, ptr(ws), stream_ptr(dev))
    del keep
    return sums, hw


@dataclass
class ReducedMaps:
    """What one pass over a captured dict leaves: ``token_sums[(step, key)]`` -- numpy [tokens] in the tensor's dtype
    (``attn.sum(dim=(0,1,2,3)).cpu().numpy()``), ``hw_tok[(step, key)]`` -- device tensor [H,W,tokens] in the dtype
    (``attn.sum(0).sum(0)``) for the kept keys, and the dict's key structure ``keys[step]`` in insertion order."""
    token_sums: Dict[tuple, np.ndarray] = field(default_factory=dict)
    hw_tok: Dict[tuple, torch.Tensor] = field(default_factory=dict)
    keys: Dict[object, list] = field(default_factory=dict)


def reduce_captured_maps(captured_maps, keep_hw_tok=1) -> ReducedMaps:
    """One ``attwarp_xattn_reduce`` call per dtype over ALL tensors of ``captured_maps`` (dict[step -> dict[layer_key ->
    Tensor[B,heads,H,W,tokens]]]).  ``keep_hw_tok``: an int n -- keep ``hw_tok`` of the last n layers (sorted keys) of
    every step, what ``aggregate_attention_map_for_tokens(num_last_layers=n)`` reads; "all"; or a collection of
    (step, key) pairs.  The per-token sums of every tensor come back in ONE device tensor per dtype, copied to the host
    once."""
    res = ReducedMaps()
    items = []
    for step, layer_dict in captured_maps.items():
        res.keys[step] = list(layer_dict.keys())
        skeys = sorted(layer_dict.keys())
        if keep_hw_tok == "all":
            kept = set(skeys)
        elif isinstance(keep_hw_tok, (int, np.integer)):
            kept = set(skeys[-int(keep_hw_tok):]) if keep_hw_tok > 0 else set()
        else:
            kept = {k for (s, k) in keep_hw_tok if s == step}
        for k, t in layer_dict.items():
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError("reduce_captured_maps: captured maps must be GPU tensors (there is no CPU path)")
            if t.dim() != 5:
                raise ValueError(f"reduce_captured_maps: [B,heads,H,W,tokens] tensors expected, got {tuple(t.shape)}")
            items.append(((step, k), t, k in kept))
    groups: Dict[tuple, list] = {}
    for it in items:
        groups.setdefault((it[1].dtype, int(it[1].shape[-1])), []).append(it)
    for group in groups.values():
        for i in range(0, len(group), _MAX_RECORDS):
            part = group[i:i + _MAX_RECORDS]
            sums, hw = xattn_reduce([t for (_, t, _) in part], [w for (_, _, w) in part])
            host = sums.float().cpu().numpy() if sums.dtype == torch.bfloat16 else sums.cpu().numpy()
            for j, (name, t, w) in enumerate(part):
                res.token_sums[name] = host[j]
                if w:
                    res.hw_tok[name] = hw[j].view(t.shape[2], t.shape[3], t.shape[4])
    return res


def _reduced(captured_maps, keep_hw_tok) -> ReducedMaps:
    return captured_maps if isinstance(captured_maps, ReducedMaps) else reduce_captured_maps(captured_maps, keep_hw_tok)


def compute_token_importance(captured_maps, inference_step_selection=None, num_layers=None, last_timestep=False):
    """Reference :310-360.  ``captured_maps``: the captured dict (GPU tensors) or a :class:`ReducedMaps`."""
    red = _reduced(captured_maps, 0)
    if last_timestep:
        t = max(red.keys.keys())
        k = max(red.keys[t])
        return red.token_sums[(t, k)]
    timesteps = ([t for t in red.keys if t in inference_step_selection] if inference_step_selection is not None
                 else list(red.keys.keys()))
    token_scores = []
    for t in timesteps:
        keys = sorted(red.keys[t])
        if num_layers is not None:
            keys = keys[-num_layers:]
        for k in keys:
            token_scores.append(red.token_sums[(t, k)])
    if not token_scores:
        raise ValueError("No attention maps to compute token importance")
    return np.mean(token_scores, axis=0)


def token_maps(hw_tok: torch.Tensor, token_indices) -> torch.Tensor:
    """``attn[..., token_indices].sum(0).sum(0).sum(-1)`` from ``hw_tok`` = ``attn.sum(0).sum(0)`` [H,W,tokens]: the third
    rounding of the reference (``sum(-1)`` in the tensor's dtype), then ``astype(float32)`` -> float32 [H,W] (device)."""
    require_gpu(hw_tok)
    idx = torch.as_tensor(np.asarray(list(token_indices), dtype=np.int64), device=hw_tok.device)
    return hw_tok[..., idx].sum(dim=-1).float()


def aggregate_attention_map_for_tokens(captured_maps, token_indices, inference_step_selection=None, num_last_layers=1):
    """Reference :365-402 -> float32 numpy [max_h,max_w].  ``captured_maps``: the captured dict (GPU tensors) or a
    :class:`ReducedMaps` that kept ``hw_tok`` of the layers read here."""
    red = _reduced(captured_maps, num_last_layers)
    all_steps = sorted(list(red.keys.keys()))
    steps_to_use = ([s for s in all_steps if s in inference_step_selection] if inference_step_selection is not None
                    else all_steps)
    maps_2d = []
    for step in steps_to_use:
        for key in sorted(list(red.keys[step]))[-num_last_layers:]:
            if (step, key) not in red.hw_tok:
                raise KeyError(f"aggregate_attention_map_for_tokens: hw_tok of {(step, key)} was not kept by "
                               f"reduce_captured_maps (keep_hw_tok)")
            maps_2d.append(token_maps(red.hw_tok[(step, key)], token_indices))
    if not maps_2d:
        raise ValueError("No attention maps to aggregate")
    max_h, max_w = max(m.shape[0] for m in maps_2d), max(m.shape[1] for m in maps_2d)
    small = [i for i, m in enumerate(maps_2d) if tuple(m.shape) != (max_h, max_w)]
    if small:
        for i, r in zip(small, resize_cubic([maps_2d[i] for i in small], [(max_w, max_h)] * len(small))):
            maps_2d[i] = r
    acc = maps_2d[0].clone()                      # np.stack(...).mean(axis=0): sequential float32 adds, then / n
    for m in maps_2d[1:]:
        acc += m
    # (torch divides by a scalar as a multiplication by its reciprocal; the quotient of a float32 by a small integer is never
    # within 2^-24 / n of a float32 rounding boundary unless it is exact, so float64 and one rounding gives numpy's bits)
    acc = (acc.double() / float(len(maps_2d))).float()
    return minmax_normalize([acc], in_place=True)[0].cpu().numpy()


# ---- float32 maps: cubic resize, blur, min-max --------------------------------------------------------------------------
def _check_maps(maps, who: str) -> Tuple[list, torch.device]:
    maps = list(maps)
    if not 0 < len(maps) <= _MAX_RECORDS:
        raise ValueError(f"{who}: 1 .. {_MAX_RECORDS} maps per call, got {len(maps)}")
    for m in maps:
        if not isinstance(m, torch.Tensor) or not m.is_cuda:
            raise RuntimeError(f"{who}: maps must be GPU tensors (there is no CPU path)")
        if m.dtype != torch.float32 or m.dim() != 2 or not m.is_contiguous() or m.numel() == 0:
            raise ValueError(f"{who}: maps must be contiguous float32 [H,W] tensors, got {m.dtype} {tuple(m.shape)}")
        if max(m.shape) > _MAX_SIDE:
            raise ValueError(f"{who}: map {tuple(m.shape)} has a side beyond {_MAX_SIDE}")
    return maps, require_gpu(*maps)


def resize_cubic(maps: Sequence[torch.Tensor], sizes_wh) -> List[torch.Tensor]:
    """``cv2.resize(m, (W, H), interpolation=cv2.INTER_CUBIC)`` for a ragged batch of float32 device maps [h_i,w_i] of any
    size in one launch; ``sizes_wh``: one (W, H) per map, cv2's order -> list of [H_i,W_i] views into one buffer."""
    maps, dev = _check_maps(maps, "resize_cubic")
    sizes = [(int(s[0]), int(s[1])) for s in sizes_wh]
    if len(sizes) != len(maps) or any(not (0 < W <= _MAX_SIDE and 0 < H <= _MAX_SIDE) for (W, H) in sizes):
        raise ValueError(f"resize_cubic: one (W, H) within 1 .. {_MAX_SIDE} per map")
    M = len(maps)
    buf, offs, views = _packed(sizes, dev)
    rec = np.zeros(M, dtype=_CUBIC_DTYPE)
    rec["src"] = [m.data_ptr() for m in maps]
    rec["out"] = buf.data_ptr() + 4 * offs
    rec["h"], rec["w"] = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    rec["W"], rec["H"] = [s[0] for s in sizes], [s[1] for s in sizes]
    keep = []
    for i, (m, (W, H)) in enumerate(zip(maps, sizes)):
        if (H, W) == tuple(m.shape):
            continue
        tx, ty = _tables.cubic_tables(int(m.shape[1]), W, dev), _tables.cubic_tables(int(m.shape[0]), H, dev)
        keep += [tx, ty]
        rec["ofs_x"][i], rec["coef_x"][i] = tx[0].data_ptr(), tx[1].data_ptr()
        rec["ofs_y"][i], rec["coef_y"][i] = ty[0].data_ptr(), ty[1].data_ptr()
    with torch.cuda.device(dev):
        rec_dev = _upload_records(rec, dev)
        call("attwarp_resize_cubic", rec.ctypes.data, ptr(rec_dev), M, stream_ptr(dev))
    del keep
    return views


def _blur_minmax(maps, outs, blur: bool, normalize_from, dev):
    """blur5_minmax on maps -> outs (blur) or partials of maps alone, then minmax_normalize of `normalize_from` in place /
    into outs."""
    M = len(maps)
    rec = np.zeros(M, dtype=_F32MAP_DTYPE)
    rec["src"] = [m.data_ptr() for m in maps]
    rec["out"] = [o.data_ptr() for o in outs] if blur else 0
    rec["H"], rec["W"] = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    rec2 = rec.copy()
    rec2["src"] = [m.data_ptr() for m in normalize_from]
    rec2["out"] = [o.data_ptr() for o in outs]
    lib = _lib.load()
    with torch.cuda.device(dev):
        both = np.concatenate([rec, rec2])
        both_dev = _upload_records(both, dev)
        ws = torch.empty(lib.attwarp_blur5_minmax_workspace_bytes(rec.ctypes.data, M), device=dev, dtype=torch.uint8)
        call("attwarp_blur5_minmax", rec.ctypes.data, both_dev.data_ptr(), M, 1 if blur else 0, ptr(ws), stream_ptr(dev))
        call("attwarp_minmax_normalize", rec2.ctypes.data, both_dev.data_ptr() + rec.nbytes, M, ptr(ws), stream_ptr(dev))


def minmax_normalize(maps: Sequence[torch.Tensor], in_place: bool = False) -> List[torch.Tensor]:
    """numpy's ``a -= a.min(); a /= (a.max() + 1e-9)`` in float32 (:160, :400-401) for a ragged batch of device maps."""
    maps, dev = _check_maps(maps, "minmax_normalize")
    outs = maps if in_place else [torch.empty_like(m) for m in maps]
    _blur_minmax(maps, outs, False, maps, dev)
    return outs


def blur5_normalize(maps: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """``cv2.GaussianBlur(m, (5, 5), sigmaX=1.0)`` followed by the in-place min-max (:410-412) for a ragged batch."""
    maps, dev = _check_maps(maps, "blur5_normalize")
    outs = [torch.empty_like(m) for m in maps]
    _blur_minmax(maps, outs, True, outs, dev)
    return outs


def blur5(maps: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """``cv2.GaussianBlur(m, (5, 5), sigmaX=1.0)`` alone (float32, BORDER_REFLECT_101)."""
    maps, dev = _check_maps(maps, "blur5")
    outs = [torch.empty_like(m) for m in maps]
    M = len(maps)
    rec = np.zeros(M, dtype=_F32MAP_DTYPE)
    rec["src"], rec["out"] = [m.data_ptr() for m in maps], [o.data_ptr() for o in outs]
    rec["H"], rec["W"] = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    with torch.cuda.device(dev):
        rec_dev = _upload_records(rec, dev)
        call("attwarp_blur5_minmax", rec.ctypes.data, ptr(rec_dev), M, 1, None, stream_ptr(dev))
    return outs


def _map_to_device(att_map, dev) -> torch.Tensor:
    a = np.asarray(att_map)
    if a.dtype != np.float32 or a.ndim != 2:
        raise TypeError(f"a float32 [h,w] attention map is expected (cv2.resize of other depths is not restated), got "
                        f"{a.dtype} {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def upsample_attention_map(att_map_lr, target_size):
    """Reference :407-413: cubic resize to ``target_size`` = (H, W), 5 x 5 Gaussian blur, min-max -> float32 numpy."""
    H, W = target_size
    dev = _lib.default_device()
    full = resize_cubic([_map_to_device(att_map_lr, dev)], [(int(W), int(H))])
    return blur5_normalize(full)[0].cpu().numpy()


# ---- the iterated warp -------------------------------------------------------------------------------------------------
def _uniform_axis_map(n: int, n_out: int, dev) -> torch.Tensor:
    """The map of one axis under the ablation's near-zero fallback (:119-133): uniform profile with total n."""
    key = ("sd_uniform", n, n_out, str(dev))
    t = _tables._DEV_CACHE.get(key)
    if t is None:
        c = np.concatenate(([0], np.cumsum(np.ones(n, np.float64)) / float(n))) * n_out
        c[-1] = n_out
        m = np.interp(np.arange(n_out), c, np.concatenate(([0], np.arange(n) + 1))).astype(np.float32)
        t = _tables._cache_put(key, torch.from_numpy(m).to(dev))
    return t


def _fallback_flags(att: torch.Tensor, transform, exp_scale, exp_divisor, apply_inverse) -> Optional[torch.Tensor]:
    """[B] bool (device): does the ablation's ``sx < EPSILON or sy < EPSILON`` (:117-123) hold?  There the ablation takes
    uniform profiles with their own totals, while new_method -- whose grid construction ``attwarp_axis_maps_from_attention``
    computes -- keeps ``mean(biased) * h * w`` clamped to EPSILON; everywhere else the two are one code.  Only a transform
    with negative values can get there: log (and exp's inverse); None for the others.  The totals are float64 sums of the
    same values in torch's order; no host synchronisation."""
    if not (transform == "log" or (transform == "exp" and apply_inverse)):
        return None
    h, w = att.shape[-2:]
    a = att.double().clamp_min(0)
    t = torch.log(a + 1e-5) if transform == "log" else torch.exp(exp_scale * a) / exp_divisor
    biased = t + BASE_ATTENTION
    px, py = biased.sum(dim=-2), biased.sum(dim=-1)
    if apply_inverse:
        if transform == "log":
            inv = lambda x: torch.exp(x) - 1e-5                                           # noqa: E731
        else:
            inv = lambda x: torch.log((x * exp_divisor).clamp_min(1e-9)) / exp_scale      # noqa: E731
        px = inv(px - BASE_ATTENTION * h) + BASE_ATTENTION * h
        py = inv(py - BASE_ATTENTION * w) + BASE_ATTENTION * w
    return (px.sum(dim=-1) < EPSILON) | (py.sum(dim=-1) < EPSILON)


def _axis_maps(att: torch.Tensor, width, height, transform, exp_scale, exp_divisor, apply_inverse):
    """att [B,h,w] float32 -> the ablation's (map_x [B,width], map_y [B,height])."""
    mx, my = _nm.attention_axis_maps(att, width, height, transform, exp_scale, exp_divisor, apply_inverse)
    flags = _fallback_flags(att, transform, exp_scale, exp_divisor, apply_inverse)
    if flags is not None:
        h, w = att.shape[-2:]
        mx = torch.where(flags[:, None], _uniform_axis_map(w, width, att.device)[None], mx)
        my = torch.where(flags[:, None], _uniform_axis_map(h, height, att.device)[None], my)
    return mx, my


def _warp_pass(images, att_maps, out_size, transform, exp_scale, exp_divisor, apply_inverse) -> torch.Tensor:
    """One ``save_warped_image`` (:142-172) for every image: map -> cubic resize to the image's size -> min-max -> axis maps
    -> cv2.remap.  -> uint8 [B,height,width,C]."""
    from .checkpoint_utils import remap_separable
    width, height = out_size
    full = resize_cubic(att_maps, [(int(im.shape[1]), int(im.shape[0])) for im in images])
    minmax_normalize(full, in_place=True)
    out = torch.empty(len(images), height, width, images[0].shape[2], device=images[0].device, dtype=torch.uint8)
    if isinstance(images, torch.Tensor):              # one size (every pass after the first): one batched call each
        mx, my = _axis_maps(torch.stack(full), width, height, transform, exp_scale, exp_divisor, apply_inverse)
        remap_separable(images, mx, my, mode="cv2", channels_last=True, out=out)
        return out
    for b, (im, a) in enumerate(zip(images, full)):
        mx, my = _axis_maps(a.unsqueeze(0), width, height, transform, exp_scale, exp_divisor, apply_inverse)
        remap_separable(im.unsqueeze(0), mx, my, mode="cv2", channels_last=True, out=out[b:b + 1])
    return out


def iterative_warp(images_u8: Sequence[torch.Tensor], att_maps: Sequence[torch.Tensor], iterations: int = 1,
                   out_size=(500, 500), transform: str = "identity", exp_scale: float = 1.0, exp_divisor: float = 1.0,
                   apply_inverse: bool = False) -> List[torch.Tensor]:
    """``run``'s warping loop (:445-456) for a batch: ``images_u8`` -- uint8 [H_i,W_i,3] device images of any sizes,
    ``att_maps`` -- their float32 device maps (any sizes), ``out_size`` = (width, height).  Every pass re-resizes each map
    from its original size to the current image size, normalises it and warps with ``exp_scale / max(1, iterations)``;
    pass i + 1 reads pass i's output (the reference's PNG round trip is lossless).  Nothing leaves the device.
    -> the batch of every pass, uint8 [B,height,width,3] each (the reference writes them as ``_it{i}.png`` and the last as
    the result)."""
    images = list(images_u8)
    att_maps, dev = _check_maps(att_maps, "iterative_warp")
    if len(images) != len(att_maps):
        raise ValueError(f"iterative_warp: {len(images)} images for {len(att_maps)} maps")
    for im in images:
        if not isinstance(im, torch.Tensor) or not im.is_cuda:
            raise RuntimeError("iterative_warp: images must be GPU tensors (there is no CPU path)")
        if im.dtype != torch.uint8 or im.dim() != 3 or not im.is_contiguous():
            raise ValueError(f"iterative_warp: contiguous uint8 [H,W,C] images expected, got {im.dtype} {tuple(im.shape)}")
    if transform not in _KNOWN:
        transform = "identity"
    step_scale = exp_scale / max(1, iterations)
    passes = []
    cur = images
    for _ in range(int(iterations)):
        out = _warp_pass(cur, att_maps, (int(out_size[0]), int(out_size[1])), transform, step_scale, exp_divisor, apply_inverse)
        passes.append(out)
        cur = out
    return passes


def _imread_bgr(image_path) -> np.ndarray:
    """``cv2.imread``: BGR uint8 [H,W,3]; FileNotFoundError when the file cannot be read (:148-150)."""
    from PIL import Image
    try:
        return np.ascontiguousarray(np.array(Image.open(image_path).convert("RGB"))[:, :, ::-1])
    except Exception:
        raise FileNotFoundError(f"Could not load {image_path}") from None


def save_warped_image(image_path, att_map, output_path, width=500, height=500, transform="identity", exp_scale=1.0,
                      exp_divisor=1.0, apply_inverse=False, skip_map_resize=False):
    """Reference :142-172: the map is cubic-resized to the image's size and min-max normalised, the image warped and
    written to ``output_path``.  Sets the module's transform state like the reference."""
    img = _imread_bgr(image_path)
    set_transform_function(transform, exp_scale, exp_divisor, apply_inverse)
    dev = _lib.default_device()
    out = iterative_warp([torch.from_numpy(img).to(dev)], [_map_to_device(att_map, dev)], 1, (width, height),
                         ATTENTION_TRANSFORM, exp_scale, exp_divisor, apply_inverse)[0][0]
    _nm._imwrite(output_path, out.cpu().numpy())
    return True


def save_warped_image_original(image_path, att_map, output_path, width=500, height=500, transform="identity",
                               exp_scale=1.0, exp_divisor=1.0, apply_inverse=False, skip_map_resize=False):
    """Reference :175-200: the IMAGE is resized to the map (INTER_LINEAR), then warped by the map as it is."""
    img = _imread_bgr(image_path)
    img_resized = resize_image_to_match_attmap(img, att_map)
    set_transform_function(transform, exp_scale, exp_divisor, apply_inverse)
    warped = warp_image_by_attention(img_resized, att_map, width, height)
    if warped is None:
        return False
    _nm._imwrite(output_path, warped)
    return True
