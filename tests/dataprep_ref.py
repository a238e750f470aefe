"""numpy restatement of the arithmetic between "decoded sample" and "batch" of the MarginalNet trainer's data path
(MN/dataloader.py:123-137, 160-189, 204-273; MN/data.py:10-47).  Independent of the library and of oracle/: its own
triangle filter, Pillow's coefficient construction, the NEAREST index recurrence and the attention-value chain.

  bilinear_coeffs(n_in, n_out)     Pillow's precompute_coeffs + normalize_coeffs_8bpc with the filter 1 - |x|, support 1
  resize_bilinear_u8(img, H, W)    Image.resize((W, H), BILINEAR): horizontal pass first (vertical first for the very tall
                                   sources of vertical_first()), uint8 in between, a pass is skipped on an axis that
                                   keeps its size
  to_tensor_u8(img)                ToTensor: uint8 -> float32 -> / 255 (IEEE float32 division), channels first
  nearest_index(n_in, n_out)       Pillow's NEAREST resize (affine scale path): the accumulated double recurrence
  attention_values(arr, normalize) _load_attention_map_from_artifact's normalisation (float32)
  attention_u8(arr, normalize)     ... followed by (arr * 255).astype(uint8)
  prepare_images / prepare_attention_maps   the stacked batches
  transform_for_sample             MN/data.py:32-47
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _triangle(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def bilinear_coeffs(n_in: int, n_out: int):
    """-> (bounds int32 [n_out,2] = (first tap, count), kk int32 [n_out,ksize], ksize); identity table (ksize 1) when the
    axis keeps its size, as the library's helper reports a skipped pass."""
    if n_in == n_out:
        bounds = np.stack([np.arange(n_out), np.ones(n_out, dtype=np.int64)], axis=1).astype(np.int32)
        return bounds, np.full((n_out, 1), 1 << PRECISION_BITS, dtype=np.int32), 1
    scale = n_in / n_out
    fscale = max(scale, 1.0)
    support = 1.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fscale
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    kk = np.zeros((n_out, ksize), dtype=np.int32)
    for o in range(n_out):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = [_triangle((i + lo - center + 0.5) * ss) for i in range(hi - lo)]
        tot = 0.0
        for v in w:
            tot += v
        if tot != 0.0:
            w = [v / tot for v in w]
        for i, v in enumerate(w):
            kk[o, i] = int((-0.5 if v < 0 else 0.5) + v * (1 << PRECISION_BITS))      # C's (int) truncates towards zero
        bounds[o] = (lo, hi - lo)
    return bounds, kk, ksize


def _resample_last_axis(src: np.ndarray, n_out: int) -> np.ndarray:
    bounds, kk, _ = bilinear_coeffs(src.shape[-1], n_out)
    s = src.astype(np.int64)
    out = np.empty(src.shape[:-1] + (n_out,), dtype=np.uint8)
    for o in range(n_out):
        lo, cnt = int(bounds[o, 0]), int(bounds[o, 1])
        acc = (s[..., lo:lo + cnt] * kk[o, :cnt].astype(np.int64)).sum(axis=-1) + (1 << (PRECISION_BITS - 1))
        out[..., o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def vertical_first(h: int, w: int, out_h: int) -> bool:
    """PIL.Image.resize (Pillow 12) resizes a source more than 100 times as high as wide that it shrinks vertically in two
    calls, the vertical one first; every other source takes ImagingResample's own order, horizontal first."""
    return h > w * 100 and out_h < h


def resize_bilinear_u8(img: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """uint8 [H,W] or [H,W,C] -> [out_h,out_w(,C)] as ``Image.resize((out_w, out_h), BILINEAR)``."""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    x = a[:, :, None] if a.ndim == 2 else a
    horizontal = lambda v: v if v.shape[1] == out_w else np.moveaxis(_resample_last_axis(np.moveaxis(v, 1, -1), out_w), -1, 1)
    vertical = lambda v: v if v.shape[0] == out_h else np.moveaxis(_resample_last_axis(np.moveaxis(v, 0, -1), out_h), -1, 0)
    if vertical_first(x.shape[0], x.shape[1], out_h):
        x = horizontal(vertical(x))
    else:
        x = vertical(horizontal(x))
    x = np.ascontiguousarray(x)
    return x[:, :, 0] if a.ndim == 2 else x


def to_tensor_u8(img: np.ndarray) -> np.ndarray:
    """uint8 [H,W] / [H,W,C] -> float32 [C,H,W] = value / 255 in IEEE float32 (torchvision's ToTensor on the CPU)."""
    a = np.asarray(img)
    x = a[:, :, None] if a.ndim == 2 else a
    return (np.ascontiguousarray(x.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0)).astype(np.float32)


def nearest_index(n_in: int, n_out: int) -> np.ndarray:
    a = n_in / n_out
    xo = a * 0.5
    idx = np.empty(n_out, dtype=np.int32)
    for x in range(n_out):
        idx[x] = math.floor(xo)
        xo += a
    return idx


def resize_nearest(img: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    a = np.asarray(img)
    if a.shape[:2] == (out_h, out_w):
        return a.copy()
    return np.ascontiguousarray(a[nearest_index(a.shape[0], out_h)][:, nearest_index(a.shape[1], out_w)])


def attention_values(arr: np.ndarray, normalize: bool = True) -> np.ndarray:
    """MN/dataloader.py:178-189 on a 2-D float32 array; ``normalize=False`` skips the division (the overlay branch's
    values gray / 255 pass through the sanitise and the clip unchanged)."""
    arr = np.asarray(arr, dtype=np.float32)
    with np.errstate(all="ignore"):
        max_val = float(arr.max()) if arr.size else 0.0
        if normalize and max_val > 0:
            if max_val > 1.0:
                arr = arr / np.float32(max_val)
        arr = np.nan_to_num(arr, nan=0.0, posinf=0.0, neginf=0.0)
        arr = np.clip(arr, 0.0, 1.0)
    return arr.astype(np.float32)


def attention_u8(arr: np.ndarray, normalize: bool = True) -> np.ndarray:
    return (attention_values(arr, normalize) * np.float32(255)).astype(np.uint8)          # :230


def _size(image_size):
    if image_size is None:
        raise ValueError("image_size=None keeps native sizes: such samples cannot be stacked")
    return (int(image_size), int(image_size)) if isinstance(image_size, int) else (int(image_size[0]), int(image_size[1]))


def prepare_images(images, image_size=512) -> np.ndarray:
    sh, sw = _size(image_size)
    return np.stack([to_tensor_u8(resize_bilinear_u8(np.asarray(im), sh, sw)) for im in images])


def prepare_attention_maps(maps, image_size=512, normalize=True) -> np.ndarray:
    sh, sw = _size(image_size)
    return np.stack([to_tensor_u8(resize_nearest(attention_u8(m, normalize), sh, sw)) for m in maps])


def transform_for_sample(dataset_name, bucket, mapping) -> str:
    """The expected transform name, worked out case by case: no dataset name or a non-GQA one -> "iden"; a GQA sample ->
    the table's entry for the bucket's string, "sqrt" when the table has none (a missing bucket is looked up as None)."""
    is_gqa = dataset_name is not None and str(dataset_name).lower().find("gqa") >= 0
    if not is_gqa:
        return "iden"
    key = str(bucket) if bucket is not None else None
    listed = [v for k, v in mapping.items() if k == key]
    return listed[0] if listed else "sqrt"
