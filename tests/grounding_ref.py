"""numpy restatement of the layer-selection study's arithmetic (the kernels of csrc/grounding.hip and
attwarp_attn_probe_head_mean are bit-exact against it):

* ``head_mean_rows``: the raw head-mean row of uncertainty_attn_maps_llava.py:56 -- ``oracle.warp_oracle.attn_probe_last_row``
  (HF eager attention's last query row at its dtype transitions) followed by a float64 mean over heads and ONE rounding;
  bfloat16 (no numpy dtype) through the same steps with an explicit round-to-nearest-even;
* ``lanczos4_coeffs`` / ``resize_lanczos4``: OpenCV 4.x ``resizeGeneric_`` with ``HResizeLanczos4`` / ``VResizeLanczos4``
  for one float32 channel (imgproc/src/resize.cpp), taps in ascending order, no FMA; ``dsize == ssize`` copies;
* ``box_metrics``: metrics.py:15-25 -- np.argmax, top1's inequalities, am with float64 sums and numpy slicing;
* ``layer_sweep``: the study's per-image loop (:54-66, :161-166) on float32 grids.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import warp_oracle as O

F32, F64 = np.float32, np.float64


# ---- bfloat16 without a numpy dtype: float32 arrays holding bf16 values -----------------------------------------------
def to_bf16(x) -> np.ndarray:
    """Round float64 / float32 values to bfloat16 ONCE (round to nearest even); float32 array of the rounded values.
    float64 input goes through float32 with round-to-odd first, which keeps the single rounding."""
    x = np.asarray(x)
    f = x
    if x.dtype == F64:
        f = x.astype(F32)
        u = f.view(np.uint32).copy()
        inexact = np.isfinite(x) & (f.astype(F64) != x)
        u[inexact & (np.abs(f.astype(F64)) > np.abs(x))] -= np.uint32(1)
        u[inexact] |= np.uint32(1)
        f = u.view(F32)
    f = np.asarray(f, dtype=F32)
    u = f.view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)
    r = np.where(np.isnan(f), np.uint32(0x7FC00000), r)
    return r.view(F32)


def _probe_rows_bf16(q, k, scaling, kv_begin=None):
    """attn_probe_last_row for bfloat16 q, k (float32 arrays of bf16 values): the oracle's steps with bf16 roundings."""
    B, H, D = q.shape
    Hkv, kv = k.shape[1], k.shape[2]
    kk = np.repeat(k, H // Hkv, axis=1)
    w = to_bf16(np.einsum("bhd,bhjd->bhj", q.astype(F64), kk.astype(F64)))
    x = to_bf16(w * F32(scaling))
    out = np.zeros((B, H, kv), dtype=F32)
    for b in range(B):
        kb = 0 if kv_begin is None else int(kv_begin[b])
        xv = x[b, :, kb:]
        m = xv.max(axis=-1, keepdims=True)
        e = np.exp((xv - m).astype(F32).astype(F64)).astype(F32)
        den = e.astype(F64).sum(axis=-1, keepdims=True).astype(F32)
        out[b, :, kb:] = to_bf16(e / den)
    return out


def head_mean_rows(q, k, starts, ntok, scaling, kv_begin=None, bf16=False):
    """[B,ntok]: mean over heads of the last query row's probabilities p[b, h, st:st+ntok], no renormalisation; the head
    sum in float64 in head order, divided by heads, rounded once to the model dtype (q's dtype, or bf16 values)."""
    p = _probe_rows_bf16(q, k, scaling, kv_begin) if bf16 else O.attn_probe_last_row(q, k, scaling, kv_begin)
    B, H = p.shape[:2]
    out = np.empty((B, ntok), dtype=F32 if bf16 else p.dtype)
    for b in range(B):
        st = min(max(int(starts[b]), 0), p.shape[2] - ntok)
        s = p[b, 0, st:st + ntok].astype(F64)
        for h in range(1, H):
            s = s + p[b, h, st:st + ntok].astype(F64)
        m = s / H
        out[b] = to_bf16(m) if bf16 else m.astype(p.dtype)
    return out


# ---- OpenCV INTER_LANCZOS4 ----------------------------------------------------------------------------------------------
_S45 = 0.70710678118654752440084436210485
_CS = [(1, 0), (-_S45, -_S45), (0, 1), (_S45, -_S45), (-1, 0), (_S45, _S45), (0, -1), (-_S45, _S45)]
CV_PI = 3.1415926535897932384626433832795


def interpolate_lanczos4(x: np.float32) -> np.ndarray:
    """OpenCV's interpolateLanczos4(float x, float* coeffs), operation by operation (math.sin / math.cos = libm's)."""
    x = F32(x)
    xs = F32(x + F32(3))
    y0 = -float(xs) * CV_PI * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    c = np.zeros(8, dtype=F32)
    total = F32(0)
    for i in range(8):
        y0_ = F32(xs - F32(i))
        if abs(y0_) >= F32(1e-6):
            y = -float(y0_) * CV_PI * 0.25
            c[i] = F32((_CS[i][0] * s0 + _CS[i][1] * c0) / (y * y))
        else:
            c[i] = F32(1e30)
        total = F32(total + c[i])
    inv = F32(F32(1) / total)
    return (c * inv).astype(F32)


def lanczos4_coeffs(n_in: int, n_out: int):
    """resizeGeneric_'s tables for one axis: (ofs int32 [n_out], coeffs float32 [n_out,8])."""
    scale = 1.0 / (float(n_out) / n_in)
    ofs = np.zeros(n_out, dtype=np.int32)
    co = np.zeros((n_out, 8), dtype=F32)
    for d in range(n_out):
        f = F32((d + 0.5) * scale - 0.5)
        s = math.floor(f)
        f = F32(f - F32(s))
        ofs[d] = s
        co[d] = interpolate_lanczos4(f)
    return ofs, co


def _taps(ofs, n_src):
    return np.clip(ofs[:, None].astype(np.int64) - 3 + np.arange(8), 0, n_src - 1)


def resize_lanczos4(grid: np.ndarray, W: int, H: int, tables=None) -> np.ndarray:
    """cv2.resize(grid, (W, H), interpolation=cv2.INTER_LANCZOS4) for a float32 [h,w] grid: horizontal pass, vertical
    pass, float32 products and sums, taps in ascending order from the first product.  Leading axes are a batch of grids
    resized to one size ([...,h,w] -> [...,H,W]): the same operations element by element."""
    g = np.asarray(grid, dtype=F32)
    h, w = g.shape[-2:]
    if (H, W) == (h, w):
        return g.copy()
    (ox, cx), (oy, cy) = tables if tables is not None else (lanczos4_coeffs(w, W), lanczos4_coeffs(h, H))
    tx = _taps(ox, w)
    hrow = g[..., tx[:, 0]] * cx[:, 0]
    for j in range(1, 8):
        hrow = (hrow + (g[..., tx[:, j]] * cx[:, j]).astype(F32)).astype(F32)
    ty = _taps(oy, h)
    out = hrow[..., ty[:, 0], :] * cy[:, 0:1]
    for k in range(1, 8):
        out = (out + (hrow[..., ty[:, k], :] * cy[:, k:k + 1]).astype(F32)).astype(F32)
    return out.astype(F32)


# ---- metrics.py --------------------------------------------------------------------------------------------------------
def box_slice(box, H, W):
    """numpy's slice a[y0:y0+h, x0:x0+w] of an [H,W] map as (r0, r1, c0, c1) (range slicing follows the same rules)."""
    x0, y0, w, h = (int(v) for v in box)
    r = range(H)[y0:y0 + h]
    c = range(W)[x0:x0 + w]
    r0 = r.start if len(r) else 0
    c0 = c.start if len(c) else 0
    return r0, r0 + len(r), c0, c0 + len(c)


def box_metrics(att: np.ndarray, box):
    """(argmax, top1, am): np.argmax (first NaN / first maximum), metrics.py:19's inequalities, am with float64 sums over
    numpy's slice a[y0:y0+h, x0:x0+w]."""
    x0, y0, w, h = (int(v) for v in box)
    i = int(np.argmax(att))
    r, c = np.unravel_index(i, att.shape)
    t = 1 if (x0 <= c < x0 + w and y0 <= r < y0 + h) else 0
    a64 = att.astype(F64)
    with np.errstate(invalid="ignore"):
        am = a64[y0:y0 + h, x0:x0 + w].sum() / (a64.sum() + 1e-12)
    return i, t, float(am)


def layer_sweep(abs_rows, gen_rows, sizes_wh, boxes, small_wh=(18, 27)):
    """The study's loop on [nL,B,ntok] float32 rows (model-dtype values): -> top1, am, argmax [nL,2,B], small
    [nL,2,B,sh,sw]."""
    abs_rows = np.asarray(abs_rows, dtype=F32)
    gen_rows = np.asarray(gen_rows, dtype=F32)
    nL, B, ntok = abs_rows.shape
    g = int(round(ntok ** 0.5))
    top1 = np.zeros((nL, 2, B), np.int32)
    am = np.zeros((nL, 2, B), F64)
    arg = np.zeros((nL, 2, B), np.int64)
    small = np.zeros((nL, 2, B, small_wh[1], small_wh[0]), F32)
    tabs = {}

    def tables(W, H):
        key = (W, H)
        if key not in tabs:
            tabs[key] = (lanczos4_coeffs(g, W), lanczos4_coeffs(g, H))
        return tabs[key]

    for l in range(nL):
        for b in range(B):
            a = abs_rows[l, b].reshape(g, g)
            rel = a / (gen_rows[l, b].reshape(g, g) + 1e-8)
            for t, grid in enumerate((a, rel)):
                W, H = sizes_wh[b]
                full = resize_lanczos4(grid, W, H, tables(W, H))
                arg[l, t, b], top1[l, t, b], am[l, t, b] = box_metrics(full, boxes[b])
                small[l, t, b] = resize_lanczos4(grid, small_wh[0], small_wh[1], tables(*small_wh))
    return top1, am, arg, small
