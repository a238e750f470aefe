"""The reference's layer-selection study on the GPU: ``Ablations/uncertainty_attn_maps_llava.py`` (last-query attention over
the image tokens for several decoder layers, absolute and relative maps, ``cv2.resize(..., INTER_LANCZOS4)`` to the image
size and to 18 x 27) and the box metrics of ``Ablations/attention_redistribution/metrics.py`` (``top1``, ``am_all``).

The study runs HF eager attention with ``output_attentions=True`` on every layer at batch 1, then 36 LANCZOS4 resizes
and numpy reductions per image on the host.  Here:

* :class:`LayerSweepProbe` captures the raw head-mean row of every swept layer during ONE (batched) prefill, with the
  layers left on their fast attention (``attwarp_attn_probe_head_mean``: nothing of size q x kv is materialised);
* :func:`layer_sweep` forms the absolute and relative grids and scores every (layer, type, sample) against its box in one
  fused launch that evaluates the LANCZOS4 value of each full-resolution pixel on the fly -- the full maps are never
  written -- and resizes the 18 x 27 maps in a second launch;
* :func:`resize_lanczos4`, :func:`box_metrics` and :func:`grid_box_metrics` (the fused form) are the pieces on their
  own (OpenCV's arithmetic restated: DESIGN.md "Layer sweep"; bit-exact with tests/grounding_ref.py).

There is no CPU path: inputs must be GPU tensors.
"""
from __future__ import annotations

import copy
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib, _tables
from ._batch import uploaded as _upload_records
from ._lib import call, ptr, require_gpu, stream_ptr
from .attention_extraction import NUM_IMAGE_TOKENS, kv_begin_from_mask, probe_head_mean

# ---- metrics.py, name for name ---------------------------------------------------------------------------------------
BBOX_METHODS: List[str] = ["xywh", "xyxy"]


def interpret_bbox(b, method: str):
    """metrics.py:6-12: a raw box as (x, y, w, h) ints under "xywh" or "xyxy"."""
    if method == "xywh":
        x, y, w, h = b
        return int(x), int(y), int(w), int(h)
    x1, y1, x2, y2 = b
    return int(x1), int(y1), int(x2 - x1), int(y2 - y1)


def select_box(b_raw):
    """The study's box choice (uncertainty_attn_maps_llava.py:146-151): the first interpretation of BBOX_METHODS with a
    positive width and height, or None (the study skips that sample)."""
    for m in BBOX_METHODS:
        b = interpret_bbox(b_raw, m)
        if b[2] > 0 and b[3] > 0:
            return b
    return None


def box_slice(box, H: int, W: int):
    """The ranges ``a[y0:y0+h, x0:x0+w]`` of am_all covers in an [H,W] map, by numpy's slice rules (a negative start counts
    from the end, stops are clipped, an empty slice stays empty): (r0, r1, c0, c1) with r0 <= r1, c0 <= c1."""
    x0, y0, w, h = (int(v) for v in box)
    r0, r1, _ = slice(y0, y0 + h).indices(H)
    c0, c1, _ = slice(x0, x0 + w).indices(W)
    return r0, max(r0, r1), c0, max(c0, c1)


def top1(attention_map: torch.Tensor, box) -> int:
    """metrics.py:15-19 on a float32 [H,W] GPU map: 1 if np.argmax of the map falls inside the box."""
    return int(box_metrics([attention_map], [box]).top1[0].item())


def am_all(attention_map: torch.Tensor, box) -> float:
    """metrics.py:22-25 on a float32 [H,W] GPU map: box mass / (total mass + 1e-12), both sums in float64."""
    return float(box_metrics([attention_map], [box]).am[0].item())


# ---- records of attwarp_grid_map -------------------------------------------------------------------------------------
_GRID_MAP_DTYPE = np.dtype([("src", "<u8"), ("out", "<u8"), ("ofs_x", "<u8"), ("coef_x", "<u8"), ("ofs_y", "<u8"),
                            ("coef_y", "<u8"), ("H", "<i4"), ("W", "<i4"), ("box_x", "<i8"), ("box_y", "<i8"),
                            ("box_w", "<i8"), ("box_h", "<i8"), ("r0", "<i4"), ("r1", "<i4"), ("c0", "<i4"),
                            ("c1", "<i4")])
assert _GRID_MAP_DTYPE.itemsize == 104
_MAX_GRID, _MAX_SIDE, _MAX_MAPS, _BOX_LIM = 64, 1 << 15, 65535, 1 << 40


def _sizes(sizes_wh, M: int, who: str):
    """(W, H) for every map: one pair for all, or one per map."""
    s = list(sizes_wh)
    if len(s) == 2 and all(isinstance(v, (int, np.integer)) for v in s):
        s = [tuple(s)] * M
    if len(s) != M:
        raise ValueError(f"{who}: {len(s)} sizes for {M} maps")
    out = []
    for wh in s:
        W, H = int(wh[0]), int(wh[1])
        if not (0 < W <= _MAX_SIDE and 0 < H <= _MAX_SIDE):
            raise ValueError(f"{who}: size (W={W}, H={H}) outside 1 .. {_MAX_SIDE}")
        out.append((W, H))
    return out


def _check_grids(grids: torch.Tensor, who: str):
    if not isinstance(grids, torch.Tensor) or not grids.is_cuda:
        raise ValueError(f"{who}: grids must be a GPU tensor (there is no CPU path)")
    if grids.dtype != torch.float32 or grids.dim() != 3:
        raise ValueError(f"{who}: grids must be float32 [M,h,w], got {grids.dtype} {tuple(grids.shape)}")
    M, h, w = grids.shape
    if not (0 < M <= _MAX_MAPS and 0 < h <= _MAX_GRID and 0 < w <= _MAX_GRID):
        raise ValueError(f"{who}: {M} grids of {h} x {w} (1 .. {_MAX_MAPS} grids of at most {_MAX_GRID} x {_MAX_GRID})")
    return grids.contiguous()


def _table_columns(rec, h: int, w: int, sizes, dev):
    """ofs_x / coef_x / ofs_y / coef_y of every record from the per-size device tables (cached per distinct size)."""
    keep = []
    for col, n_in, idx in (("x", w, 0), ("y", h, 1)):
        ptrs = {}
        for n in {s[idx] for s in sizes}:
            ofs, coef = _tables.lanczos4_tables(n_in, n, dev)
            keep += [ofs, coef]
            ptrs[n] = (ofs.data_ptr(), coef.data_ptr())
        rec["ofs_" + col] = [ptrs[s[idx]][0] for s in sizes]
        rec["coef_" + col] = [ptrs[s[idx]][1] for s in sizes]
    return keep


def _boxes(rec, boxes, sizes, who: str):
    if len(boxes) != len(sizes):
        raise ValueError(f"{who}: {len(boxes)} boxes for {len(sizes)} maps")
    b = np.array([[int(v) for v in box] for box in boxes], dtype=object).reshape(len(boxes), 4) if len(boxes) else None
    if b is None or np.any(np.abs(b.astype(float)) >= _BOX_LIM):
        raise ValueError(f"{who}: boxes must be (x, y, w, h) integers below 2^40 in magnitude")
    b = b.astype(np.int64)
    rec["box_x"], rec["box_y"], rec["box_w"], rec["box_h"] = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    sl = np.array([box_slice(box, H, W) for box, (W, H) in zip(b.tolist(), sizes)], dtype=np.int32)
    rec["r0"], rec["r1"], rec["c0"], rec["c1"] = sl[:, 0], sl[:, 1], sl[:, 2], sl[:, 3]


def _packed(sizes, dev):
    """One float32 buffer holding [H_i,W_i] maps back to back (16-byte aligned offsets) and the views into it."""
    n = np.array([W * H for (W, H) in sizes], dtype=np.int64)
    span = (n + 3) // 4 * 4
    offs = np.concatenate([[0], np.cumsum(span)[:-1]]).astype(np.int64)
    buf = torch.empty(int(span.sum()), device=dev, dtype=torch.float32)
    views = [buf[o:o + W * H].view(H, W) for o, (W, H) in zip(offs.tolist(), sizes)]
    return buf, offs, views


def _resize_into(grids: torch.Tensor, sizes, out_ptrs, dev):
    M, h, w = grids.shape
    rec = np.zeros(M, dtype=_GRID_MAP_DTYPE)
    rec["src"] = grids.data_ptr() + 4 * h * w * np.arange(M, dtype=np.int64)
    rec["out"] = out_ptrs
    rec["W"] = [s[0] for s in sizes]
    rec["H"] = [s[1] for s in sizes]
    keep = _table_columns(rec, h, w, sizes, dev)
    with torch.cuda.device(dev):
        rec_dev = _upload_records(rec, dev)
        call("attwarp_resize_lanczos4", rec.ctypes.data, ptr(rec_dev), M, h, w, stream_ptr(dev))
    del keep


def resize_lanczos4(grids: torch.Tensor, sizes_wh):
    """``cv2.resize(grid, (W, H), interpolation=cv2.INTER_LANCZOS4)`` for a batch of float32 grids [M,h,w] (h, w <= 64) on
    the GPU, OpenCV's generic-path arithmetic (uncertainty_attn_maps_llava.py:63-64).  ``sizes_wh``: one (W, H) -- in cv2's
    order -- for every grid (-> [M,H,W]), or a list of M pairs (-> list of [H_i,W_i] views into one buffer).  A [h,w] grid
    with one size gives [H,W]."""
    single = isinstance(grids, torch.Tensor) and grids.dim() == 2
    g = _check_grids(grids.unsqueeze(0) if single else grids, "resize_lanczos4")
    M = g.shape[0]
    one = len(sizes_wh) == 2 and all(isinstance(v, (int, np.integer)) for v in sizes_wh)
    sizes = _sizes(sizes_wh, M, "resize_lanczos4")
    dev = g.device
    if one:
        W, H = sizes[0]
        out = torch.empty(M, H, W, device=dev, dtype=torch.float32)
        _resize_into(g, sizes, out.data_ptr() + 4 * H * W * np.arange(M, dtype=np.int64), dev)
        return out[0] if single else out
    buf, offs, views = _packed(sizes, dev)
    _resize_into(g, sizes, buf.data_ptr() + 4 * offs, dev)
    return views


@dataclass
class BoxMetrics:
    """Per map: ``argmax`` int64 (row-major np.argmax), ``top1`` int32, ``am`` float64 -- GPU tensors [M]."""
    argmax: torch.Tensor
    top1: torch.Tensor
    am: torch.Tensor


def _metrics(rec: np.ndarray, dev, fused: bool, h: int, w: int) -> BoxMetrics:
    M = int(rec.shape[0])
    lib = _lib.load()
    with torch.cuda.device(dev):
        rec_dev = _upload_records(rec, dev)
        ws = torch.empty(lib.attwarp_box_metrics_workspace_bytes(rec.ctypes.data, M), device=dev, dtype=torch.uint8)
        res = BoxMetrics(torch.empty(M, device=dev, dtype=torch.int64), torch.empty(M, device=dev, dtype=torch.int32),
                         torch.empty(M, device=dev, dtype=torch.float64))
        call("attwarp_box_metrics", rec.ctypes.data, ptr(rec_dev), M, 1 if fused else 0, h, w, ptr(res.argmax), ptr(res.top1),
             ptr(res.am), ptr(ws), stream_ptr(dev))
    return res


def box_metrics(maps, boxes) -> BoxMetrics:
    """``top1`` / ``am_all`` (metrics.py:15-25) of float32 maps in GPU memory: a tensor [M,H,W] or a list of [H_i,W_i]
    tensors, one (x, y, w, h) box per map as :func:`interpret_bbox` gives it.  One call for the whole batch."""
    if isinstance(maps, torch.Tensor):
        if maps.dim() != 3:
            raise ValueError(f"box_metrics: maps must be [M,H,W] or a list of [H,W] tensors, got {tuple(maps.shape)}")
        maps = list(maps.contiguous())
    maps = list(maps)
    M = len(maps)
    if not 0 < M <= _MAX_MAPS:
        raise ValueError(f"box_metrics: 1 .. {_MAX_MAPS} maps per call, got {M}")
    for m in maps:
        if not isinstance(m, torch.Tensor) or not m.is_cuda:
            raise ValueError("box_metrics: maps must be GPU tensors (there is no CPU path)")
        if m.dtype != torch.float32 or m.dim() != 2 or not m.is_contiguous():
            raise ValueError(f"box_metrics: maps must be contiguous float32 [H,W] tensors, got {m.dtype} {tuple(m.shape)}")
    dev = require_gpu(*maps)
    sizes = _sizes([(int(m.shape[1]), int(m.shape[0])) for m in maps], M, "box_metrics")
    rec = np.zeros(M, dtype=_GRID_MAP_DTYPE)
    rec["src"] = [m.data_ptr() for m in maps]
    rec["W"] = [s[0] for s in sizes]
    rec["H"] = [s[1] for s in sizes]
    _boxes(rec, list(boxes), sizes, "box_metrics")
    return _metrics(rec, dev, False, 0, 0)


def grid_box_metrics(grids: torch.Tensor, sizes_wh, boxes) -> BoxMetrics:
    """:func:`box_metrics` of ``resize_lanczos4(grids, sizes_wh)`` without writing the resized maps: the LANCZOS4 value of
    every pixel is computed on the fly (one launch plus a small combining one).  Identical bits to resizing first and then
    calling :func:`box_metrics`.  grids float32 [M,h,w] (h, w <= 64); sizes_wh one (W, H) or M of them; M boxes."""
    g = _check_grids(grids, "grid_box_metrics")
    M, h, w = g.shape
    sizes = _sizes(sizes_wh, M, "grid_box_metrics")
    rec = np.zeros(M, dtype=_GRID_MAP_DTYPE)
    rec["src"] = g.data_ptr() + 4 * h * w * np.arange(M, dtype=np.int64)
    rec["W"] = [s[0] for s in sizes]
    rec["H"] = [s[1] for s in sizes]
    keep = _table_columns(rec, h, w, sizes, g.device)
    _boxes(rec, list(boxes), sizes, "grid_box_metrics")
    res = _metrics(rec, g.device, True, h, w)
    del keep
    return res


# ---- the sweep -------------------------------------------------------------------------------------------------------
TYPES = ("absolute", "relative")


@dataclass
class SweepResult:
    """Per (layer, type, sample), types ordered ("absolute", "relative"): ``top1`` int32 and ``am`` float64 [nL,2,B],
    ``argmax`` int64 [nL,2,B] (row-major in the full map), ``small`` float32 [nL,2,B,27,18] (the 18 x 27 maps the study
    colours), ``maps`` (with return_maps=True: nested lists [l][t][b] of full-size [H_b,W_b] maps, else None) and
    ``layers`` (the labels of the first axis)."""
    top1: torch.Tensor
    am: torch.Tensor
    argmax: torch.Tensor
    small: torch.Tensor
    maps: Optional[list]
    layers: List[int]

    def summary(self):
        """The study's summary table (uncertainty_attn_maps_llava.py:182-185): [(layer, type, mean top1, mean am)] for every
        layer, absolute before relative, means over the batch."""
        t = self.top1.double().mean(dim=-1).cpu().numpy()
        a = self.am.mean(dim=-1).cpu().numpy()
        return [(self.layers[l], typ, float(t[l, k]), float(a[l, k])) for l in range(len(self.layers))
                for k, typ in enumerate(TYPES)]


def layer_sweep(abs_rows: torch.Tensor, gen_rows: torch.Tensor, sizes_wh, boxes, small_wh=(18, 27),
                return_maps: bool = False, layers: Optional[Sequence[int]] = None) -> SweepResult:
    """The study's per-image work (uncertainty_attn_maps_llava.py:54-66, 161-166) for a whole batch in two launches.

    ``abs_rows`` / ``gen_rows``: [nL,B,ntok] raw head-mean rows of the question prompt and of the generic prompt (e.g.
    :meth:`LayerSweepProbe.rows` of the two prefills), ntok = g*g; ``sizes_wh``: B image sizes (W, H) as PIL reports
    them; ``boxes``: B boxes (x, y, w, h) -- :func:`select_box` of the raw annotation (the study skips samples without
    one); ``small_wh``: cv2's (W, H) of the small maps; ``layers``: labels of the first axis for :meth:`summary`
    (default 0 .. nL-1).

    abs = rows.float(), rel = abs / (gen + 1e-8) in float32 (numpy's float32 expression, :58-60); full maps: the fused
    LANCZOS4 + metrics launch (the maps are materialised only with return_maps=True)."""
    if not (isinstance(abs_rows, torch.Tensor) and isinstance(gen_rows, torch.Tensor)) or not (abs_rows.is_cuda and gen_rows.is_cuda):
        raise ValueError("layer_sweep: abs_rows and gen_rows must be GPU tensors (there is no CPU path)")
    if abs_rows.dim() != 3 or abs_rows.shape != gen_rows.shape:
        raise ValueError(f"layer_sweep: abs_rows and gen_rows must be [nL,B,ntok] of one shape, got {tuple(abs_rows.shape)} "
                         f"and {tuple(gen_rows.shape)}")
    nL, B, ntok = abs_rows.shape
    g = int(round(ntok ** 0.5))
    if g * g != ntok or g > _MAX_GRID:
        raise ValueError(f"layer_sweep: ntok={ntok} is not the square of a grid side <= {_MAX_GRID}")
    if 2 * nL * B > _MAX_MAPS:
        raise ValueError(f"layer_sweep: 2 * nL * B = {2 * nL * B} maps (> {_MAX_MAPS})")
    sizes = _sizes(sizes_wh, B, "layer_sweep")
    boxes = list(boxes)
    if len(boxes) != B or any(b is None for b in boxes):
        raise ValueError(f"layer_sweep: one (x, y, w, h) box per sample ({B}); drop samples whose select_box is None")
    small = _sizes([tuple(small_wh)], 1, "layer_sweep")[0]
    labels = list(range(nL)) if layers is None else [int(v) for v in layers]
    if len(labels) != nL:
        raise ValueError(f"layer_sweep: {len(labels)} layer labels for {nL} layers")
    require_gpu(abs_rows, gen_rows)

    a = abs_rows.float()
    grids = torch.stack([a, a / (gen_rows.float() + 1e-8)], dim=1).reshape(nL * 2 * B, g, g).contiguous()
    msizes = sizes * (2 * nL)                                       # map m = (l * 2 + t) * B + b
    res = grid_box_metrics(grids, msizes, boxes * (2 * nL))
    sm = resize_lanczos4(grids, small)
    maps = None
    if return_maps:
        full = resize_lanczos4(grids, msizes)
        maps = [[full[(l * 2 + t) * B:(l * 2 + t + 1) * B] for t in range(2)] for l in range(nL)]
    return SweepResult(res.top1.view(nL, 2, B), res.am.view(nL, 2, B), res.argmax.view(nL, 2, B),
                       sm.view(nL, 2, B, small[1], small[0]), maps, labels)


# ---- the multi-layer probe -------------------------------------------------------------------------------------------
def decoder_layers(model):
    """The decoder layers of a causal LM or a LLaVA model: ``model.get_decoder().layers``, else ``model.model.layers``
    (LlamaForCausalLM, LLaVA's own class, HF's LlavaForConditionalGeneration).  Found by name, not by structure: the CLIP
    tower's layers own a ``self_attn`` too."""
    dec = model.get_decoder() if hasattr(model, "get_decoder") else None
    layers = getattr(dec, "layers", None)
    if layers is None:
        layers = getattr(getattr(model, "model", None), "layers", None)
    if layers is None:
        raise ValueError(f"LayerSweepProbe: cannot find the decoder layers of {type(model).__name__}")
    return layers


class LayerSweepProbe:
    """Raw head-mean last-query rows of several decoder layers from ONE prefill, every layer left on its fast attention.

    ``layers`` are 0-based decoder indices, as ``BatchMaskHookLogger(layer_index=...)``.  The study's ``L`` reads
    ``out.attentions[L-1]`` (uncertainty_attn_maps_llava.py:55), so its sweep ``LAYERS = [4, 8, ..., 24]`` is
    ``[L - 1 for L in LAYERS]`` here.  Every target layer gets a private config whose attention implementation (registered
    through transformers' ``AttentionInterface``) computes ``probe_head_mean`` from the post-RoPE query and key and then
    delegates to the model's own implementation; every other layer is untouched.  ``remove()`` (or leaving the ``with``
    block) restores the model exactly.

    Use: ``set_image_token_starts(starts)`` (first image token per sample), run the prefill, ``rows()`` -> [nL,B,ntok] in
    the model dtype (the last captured row of each layer; :meth:`clear` forgets them).

    A batched, LEFT-padded prefill must pass ``position_ids`` derived from the attention mask (e.g.
    ``(attention_mask.cumsum(-1) - 1).clamp_min(0)``): without them padded samples see shifted RoPE positions and their rows
    differ from a batch-1 run.  The reference itself runs at batch 1."""

    def __init__(self, model, layers: Sequence[int], ntok: int = NUM_IMAGE_TOKENS):
        try:
            from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS, AttentionInterface
        except ImportError as e:   # fail loudly: there is no silent fallback to the eager path
            raise RuntimeError("LayerSweepProbe needs transformers' AttentionInterface (>= 4.48)") from e
        self.model = model
        self.layers = [int(v) for v in layers]
        self.ntok = int(ntok)
        dec = decoder_layers(model)
        if not self.layers or len(set(self.layers)) != len(self.layers) or any(not 0 <= v < len(dec) for v in self.layers):
            raise ValueError(f"LayerSweepProbe: layers {self.layers} must be distinct indices in 0 .. {len(dec) - 1}")
        self._starts: Optional[List[int]] = None
        self._starts_dev: Optional[torch.Tensor] = None
        self._rows: List[Optional[torch.Tensor]] = [None] * len(self.layers)
        self._saved = []
        try:
            for slot, li in enumerate(self.layers):
                attn = dec[li].self_attn
                base = attn.config._attn_implementation
                eager = getattr(sys.modules[type(attn).__module__], "eager_attention_forward", None)
                base_fn = ALL_ATTENTION_FUNCTIONS.get_interface(base, eager)
                if base_fn is None:
                    raise RuntimeError(f"LayerSweepProbe: cannot resolve the attention implementation '{base}'")
                name = f"attwarp_sweep_{id(self):x}_{li}"
                AttentionInterface.register(name, self._wrap(slot, base_fn))
                self._saved.append((attn, attn.config, name))
                private = copy.copy(attn.config)
                private._attn_implementation = name
                attn.config = private
        except Exception:
            self.remove()
            raise

    def _wrap(self, slot: int, base_fn):
        probe = self

        def probed(module, query, key, value, attention_mask, **kwargs):
            if probe._starts is not None:
                probe._capture(slot, query, key, attention_mask, kwargs.get("scaling"))
            return base_fn(module, query, key, value, attention_mask, **kwargs)
        return probed

    @torch.no_grad()
    def _capture(self, slot: int, query, key, attention_mask, scaling):
        B, kv = key.shape[0], key.shape[2]
        if len(self._starts) < B:
            raise RuntimeError(f"LayerSweepProbe: {len(self._starts)} image-token starts for a batch of {B}")
        for b, st in enumerate(self._starts[:B]):
            if st < 0 or st + self.ntok > kv:
                raise ValueError(f"LayerSweepProbe: image-token range [{st}, {st + self.ntok}) of sample {b} is outside the "
                                 f"attention row of {kv} keys")
        if self._starts_dev is None or self._starts_dev.device != key.device or self._starts_dev.numel() < B:
            self._starts_dev = torch.tensor(self._starts, dtype=torch.int32, device=key.device)
        self._rows[slot] = probe_head_mean(query, key, self._starts_dev[:B], self.ntok, kv_begin_from_mask(attention_mask, kv),
                                           scaling)

    def set_image_token_starts(self, starts: Sequence[int]):
        """First image token of every sample (e.g. ``input_ids[b].tolist().index(image_token_index)`` plus its left
        padding); the span is ``ntok`` tokens from there."""
        self._starts = [int(s) for s in starts]
        self._starts_dev = None

    def rows(self) -> torch.Tensor:
        """[nL,B,ntok] in the model dtype, layers in the order given."""
        if any(r is None for r in self._rows):
            missing = [li for li, r in zip(self.layers, self._rows) if r is None]
            raise RuntimeError(f"LayerSweepProbe: no row captured for layers {missing} (set_image_token_starts, then run a "
                               f"forward pass)")
        return torch.stack(self._rows, dim=0)

    def clear(self):
        self._rows = [None] * len(self.layers)

    def remove(self):
        """Give every probed layer its own config back and unregister the wrappers."""
        try:
            from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
        except ImportError:
            ALL_ATTENTION_FUNCTIONS = None
        for attn, config, name in reversed(self._saved):
            attn.config = config
            if ALL_ATTENTION_FUNCTIONS is not None:
                ALL_ATTENTION_FUNCTIONS._global_mapping.pop(name, None)
        self._saved = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.remove()
        return False
