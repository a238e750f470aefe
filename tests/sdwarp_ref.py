"""numpy restatement of the Stable-Diffusion warp ablation's arithmetic (the kernels of csrc/sdwarp.hip are bit-exact
against it):

* ``xattn_reduce``: ``token_sums`` / ``hw_tok`` of one captured tensor [B,heads,HW,tokens] in the documented summation order
  (DESIGN.md 3.9): float64 over B, over heads, over the positions of a chunk, over chunks -- each ascending from 0.0 / from
  the first term as written below -- and the reference's roundings to the tensor's dtype.  bfloat16 (no numpy dtype) as
  float32 arrays of bf16 values with an explicit round-to-nearest-even (tests/grounding_ref.to_bf16);
* ``cubic_coeffs`` / ``resize_cubic``: OpenCV 4.x ``resizeGeneric_`` with ``interpolateCubic`` (A = -0.75f) and the scalar
  ``HResizeCubic`` / ``VResizeCubic`` for one float32 channel, taps ascending from the first product, no FMA;
* ``gaussian5_taps`` / ``blur5``: ``getGaussianKernel(5, 1.0)`` and the separable symmetric 5-tap filter with
  BORDER_REFLECT_101; ``minmax_normalize``: numpy's own in-place expressions of the reference;
* ``iterative_warp``: ``run``'s loop (Stable_diffusion_based_warp.py:445-456) on top of the oracle's axis maps and uint8
  resample.
"""
from __future__ import annotations

import math

import numpy as np

from grounding_ref import to_bf16

F32, F64 = np.float32, np.float64
XA_ELEMS = 2048


def xattn_chunk(tokens: int) -> int:
    return max(1, XA_ELEMS // tokens)


def _round_to(x64: np.ndarray, dtype: str) -> np.ndarray:
    """float64 -> the tensor's dtype, one rounding; bf16 values are carried in float32."""
    if dtype == "bf16":
        return to_bf16(x64)
    with np.errstate(over="ignore"):
        return x64.astype(np.float16 if dtype == "f16" else F32)


def xattn_reduce(attn: np.ndarray, dtype: str):
    """attn [B,heads,HW,tokens] (float32 / float16 arrays, or float32 holding bf16 values with dtype="bf16") ->
    (token_sums [tokens], hw_tok [HW,tokens]) in the tensor's dtype (bf16: float32 arrays of bf16 values)."""
    B, heads, HW, tokens = attn.shape
    tot = np.zeros((HW, tokens), F64)
    acc_h = np.zeros((HW, tokens), F64)
    for h in range(heads):
        acc_b = np.zeros((HW, tokens), F64)
        for b in range(B):
            acc_b = acc_b + attn[b, h].astype(F64)
        tot = tot + acc_b
        acc_h = acc_h + _round_to(acc_b, dtype).astype(F64)
    hw_tok = _round_to(acc_h, dtype)
    chunk = xattn_chunk(tokens)
    total = None
    for p0 in range(0, HW, chunk):
        part = tot[p0].copy()
        for p in range(p0 + 1, min(HW, p0 + chunk)):
            part = part + tot[p]
        total = part if total is None else total + part
    return _round_to(total, dtype), hw_tok


# ---- OpenCV INTER_CUBIC -------------------------------------------------------------------------------------------------
def interpolate_cubic(x) -> np.ndarray:
    """OpenCV's interpolateCubic(float x, float* coeffs), operation by operation in float32."""
    x = F32(x)
    A = F32(-0.75)
    one = F32(1)
    x1 = F32(x + one)
    c = np.zeros(4, F32)
    c[0] = F32(F32(F32(F32(F32(F32(A * x1) - F32(F32(5) * A)) * x1) + F32(F32(8) * A)) * x1) - F32(F32(4) * A))
    c[1] = F32(F32(F32(F32(F32(F32(A + F32(2)) * x) - F32(A + F32(3))) * x) * x) + one)
    xm = F32(one - x)
    c[2] = F32(F32(F32(F32(F32(F32(A + F32(2)) * xm) - F32(A + F32(3))) * xm) * xm) + one)
    c[3] = F32(F32(F32(one - c[0]) - c[1]) - c[2])
    return c


def cubic_coeffs(n_in: int, n_out: int):
    """resizeGeneric_'s tables for one axis: (ofs int32 [n_out], coeffs float32 [n_out,4])."""
    scale = 1.0 / (float(n_out) / n_in)
    ofs = np.zeros(n_out, dtype=np.int32)
    co = np.zeros((n_out, 4), dtype=F32)
    for d in range(n_out):
        f = F32((d + 0.5) * scale - 0.5)
        s = math.floor(f)
        f = F32(f - F32(s))
        ofs[d] = s
        co[d] = interpolate_cubic(f)
    return ofs, co


def _taps(ofs, n_src):
    return np.clip(ofs[:, None].astype(np.int64) - 1 + np.arange(4), 0, n_src - 1)


def resize_cubic(src: np.ndarray, W: int, H: int, tables=None) -> np.ndarray:
    """cv2.resize(src, (W, H), interpolation=cv2.INTER_CUBIC) for a float32 [h,w] map; leading axes are a batch of maps
    resized to one size (the same operations element by element)."""
    g = np.asarray(src, dtype=F32)
    h, w = g.shape[-2:]
    if (H, W) == (h, w):
        return g.copy()
    (ox, cx), (oy, cy) = tables if tables is not None else (cubic_coeffs(w, W), cubic_coeffs(h, H))
    with np.errstate(invalid="ignore", over="ignore"):
        tx = _taps(ox, w)
        ty = _taps(oy, h)
        rows = np.unique(ty)                     # only the source rows the output needs (a large source, few outputs)
        pos = np.searchsorted(rows, ty)
        gr = g[..., rows, :]
        hrow = gr[..., tx[:, 0]] * cx[:, 0]
        for j in range(1, 4):
            hrow = (hrow + (gr[..., tx[:, j]] * cx[:, j]).astype(F32)).astype(F32)
        out = hrow[..., pos[:, 0], :] * cy[:, 0:1]
        for k in range(1, 4):
            out = (out + (hrow[..., pos[:, k], :] * cy[:, k:k + 1]).astype(F32)).astype(F32)
    return out.astype(F32)


# ---- GaussianBlur(5 x 5, sigma 1) and the min-max ---------------------------------------------------------------------------
def gaussian5_taps(sigma: float = 1.0) -> np.ndarray:
    """getGaussianKernel(5, sigma) as float32: exp(-x^2 / (2 sigma^2)) normalised in double, each tap rounded."""
    scale2x = -0.5 / (sigma * sigma)
    t = [math.exp(scale2x * (i - 2.0) * (i - 2.0)) for i in range(5)]
    s = 0.0
    for v in t:
        s += v
    s = 1.0 / s
    return np.array([v * s for v in t], dtype=F64).astype(F32)


def reflect101(p: np.ndarray, n: int) -> np.ndarray:
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101)."""
    p = np.array(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def _sym5(k, a, b, c, d, e):
    return ((k[2] * c + (k[1] * (b + d).astype(F32)).astype(F32)).astype(F32) + (k[0] * (a + e).astype(F32)).astype(F32)).astype(F32)


def blur5(src: np.ndarray) -> np.ndarray:
    """cv2.GaussianBlur(src, (5, 5), sigmaX=1.0) for a float32 [H,W] map: row pass, column pass, each in the symmetric
    form k0*s0 + k1*(s-1 + s1) + k2*(s-2 + s2), every operation rounded."""
    a = np.asarray(src, dtype=F32)
    H, W = a.shape
    k = gaussian5_taps(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        xs = [reflect101(np.arange(W) + o, W) for o in (-2, -1, 0, 1, 2)]
        r = _sym5(k, *[a[:, x] for x in xs])
        ys = [reflect101(np.arange(H) + o, H) for o in (-2, -1, 0, 1, 2)]
        return _sym5(k, *[r[y, :] for y in ys])


def minmax_normalize(a: np.ndarray) -> np.ndarray:
    """The reference's own lines (:160, :400-401, :411-412) on a float32 copy."""
    a = np.array(a, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a -= a.min()
        a /= (a.max() + 1e-9)
    return a


def upsample_attention_map(att_map_lr, target_size):
    H, W = target_size
    return minmax_normalize(blur5(resize_cubic(att_map_lr, W, H)))


# ---- the aggregated map and the iterated warp --------------------------------------------------------------------------------
def token_maps(hw_tok, token_indices, dtype: str) -> np.ndarray:
    """hw_tok[..., idx].sum(-1) in the tensor's dtype, then astype(float32) (:383-385): the sum in float64, rounded once
    (torch's own order on the device may differ by the float32 summation bound; the tests compare within it)."""
    s = hw_tok[..., list(token_indices)].astype(F64).sum(axis=-1)
    return _round_to(s, dtype).astype(F32)


def aggregate_from_maps(maps) -> np.ndarray:
    """aggregate_attention_map_for_tokens after the per-layer maps exist (:390-402): cubic resize to the largest, np.mean
    over the stack, min-max."""
    mh, mw = max(m.shape[0] for m in maps), max(m.shape[1] for m in maps)
    maps = [m if m.shape == (mh, mw) else resize_cubic(m, mw, mh) for m in maps]
    return minmax_normalize(np.stack(maps, axis=0).mean(axis=0))


def aggregate_from_hw_tok(hw_toks, token_indices, dtype: str) -> np.ndarray:
    """aggregate_attention_map_for_tokens (:380-402) from hw_tok arrays [H,W,tokens] in the tensor's dtype."""
    return aggregate_from_maps([token_maps(hw, token_indices, dtype) for hw in hw_toks])


def iterative_warp(images, att_maps, iterations, out_size, transform, exp_scale, exp_divisor, apply_inverse):
    """run's loop (:445-456) with save_warped_image (:142-172) per pass -> list over passes of lists of uint8 images."""
    from oracle import warp_oracle as O
    width, height = out_size
    step_scale = exp_scale / max(1, iterations)
    cur = [np.asarray(im) for im in images]
    passes = []
    for _ in range(iterations):
        nxt = []
        for im, a in zip(cur, att_maps):
            Hh, Ww = im.shape[:2]
            full = minmax_normalize(resize_cubic(a, Ww, Hh))
            nxt.append(warp_u8(O, im, full, width, height, transform, step_scale, exp_divisor, apply_inverse))
        passes.append(nxt)
        cur = nxt
    return passes


def maps_from_attention(att, new_width, new_height, transform, exp_scale, exp_divisor, apply_inverse):
    """The (tx, ty) of the ablation's warp_image_by_attention (:99-133).  It is new_method's grid construction (the
    oracle's maps_from_attention) except in the near-zero fallback (:119-123), where the ablation takes uniform profiles
    with their own totals (sx = w, sy = h) while new_method keeps mean(biased) * h * w clamped to EPSILON."""
    from oracle import warp_oracle as O
    if transform not in O.TRANSFORMS:
        transform = "identity"
    h, w = att.shape[:2]
    with np.errstate(all="ignore"):
        biased = O._transform(np.maximum(att.astype(F64), 0), transform, exp_scale, exp_divisor) + O.BASE_ATTENTION
        px, py = np.sum(biased, axis=0), np.sum(biased, axis=1)
        if apply_inverse:
            px = O._inverse(px - O.BASE_ATTENTION * h, transform, exp_scale, exp_divisor) + O.BASE_ATTENTION * h
            py = O._inverse(py - O.BASE_ATTENTION * w, transform, exp_scale, exp_divisor) + O.BASE_ATTENTION * w
    if not (np.sum(px) < O.EPSILON or np.sum(py) < O.EPSILON):
        return O.maps_from_attention(att, new_width, new_height, transform, exp_scale, exp_divisor, apply_inverse)
    return uniform_axis_map(w, new_width), uniform_axis_map(h, new_height)


def uniform_axis_map(n: int, n_out: int) -> np.ndarray:
    """The fallback's map of one axis: uniform profile, total n."""
    c = np.concatenate(([0], np.cumsum(np.ones(n, F64)) / float(n))) * n_out
    c[-1] = n_out
    return np.interp(np.arange(n_out), c, np.concatenate(([0], np.arange(n) + 1))).astype(F32)


def warp_u8(O, image, att, width, height, transform, exp_scale, exp_divisor, apply_inverse):
    """warp_image_by_attention (:93-140): the maps above, cv2.remap's uint8 arithmetic as the oracle restates it."""
    mx, my = maps_from_attention(att, width, height, transform, exp_scale, exp_divisor, apply_inverse)
    return O.remap_bilinear(image, mx, my, "cv2")
