"""What tests/test_clip_ragged_gpu.py and tests/test_clip_ragged_cpu.py share: the reference of the ragged CLIP preprocess
(pipeline.ClipBatch, csrc/clip_ragged.hip) and its case lists.  The padded canvas is built by Pillow itself (Image.new +
paste), the resize, crop and normalisation come from tests/clip_ref.py (Pillow, numpy); nothing of the product is read."""
import functools

import numpy as np
from PIL import Image

import clip_ref as R

SIZE = 336


def background_of(mean):
    return tuple(int(m * 255) for m in mean)


def pad_canvas(img_u8, background):
    """LLaVA's expand2square with Pillow: uint8 [H,W,C] -> uint8 [n,n,C], n = max(H, W)."""
    img = np.asarray(img_u8)
    H, W, C = img.shape
    if H == W:
        return img
    n = max(H, W)
    if C == 1:
        pil, canvas = Image.fromarray(img[:, :, 0]), Image.new("L", (n, n), int(background[0]))
    else:
        pil, canvas = Image.fromarray(img), Image.new("RGB", (n, n), tuple(int(b) for b in background[:3]))
    canvas.paste(pil, ((n - W) // 2, 0) if H > W else (0, (n - H) // 2))
    out = np.asarray(canvas)
    return out[:, :, None] if C == 1 else out


def reference(img_u8, size=SIZE, pad_to_square=True, mean=R.OPENAI_CLIP_MEAN, std=R.OPENAI_CLIP_STD, background=None):
    """float32 [C,size,size]."""
    src = pad_canvas(img_u8, background_of(mean) if background is None else background) if pad_to_square else np.asarray(img_u8)
    return R.clip_preprocess(src, size, mean, std)


def image(H, W, name, seed=0, C=3, size=SIZE):
    return R.pattern(name, H, W, C, size, seed)


@functools.lru_cache(maxsize=None)
def cached_reference(H, W, name, seed=0, size=SIZE, pad_to_square=True):
    """The default-constant reference of image(H, W, name, seed): computed once per session, never written to."""
    out = reference(image(H, W, name, seed, size=size), size, pad_to_square)
    out.setflags(write=False)
    return out


def taps(n, size=SIZE):
    """Pillow's BICUBIC tap count n -> size; 1 for the identity tables of an axis that keeps its size."""
    return 1 if n == size else R.taps(n, size)


# (H, W, fused, window): what ClipBatch.plan must report for the image padded to a square and resized to 336
PAD_GEOMETRY = [(1, 1, 1, 8), (1, 40, 1, 8), (40, 1, 1, 8), (2, 3, 1, 8), (61, 48, 1, 8), (48, 61, 1, 8), (5, 8, 1, 8)]
IDENTITY = [(336, 336, 1, 8), (336, 200, 1, 8), (200, 336, 1, 8), (337, 300, 1, 8), (335, 336, 1, 8)]
WINDOW_EDGES = [(40, 504, 1, 8), (504, 40, 1, 8), (40, 505, 1, 16), (505, 40, 1, 16),          # 7 | 9 taps
                (40, 1176, 1, 16), (1176, 40, 1, 16), (40, 1177, 0, 0), (1177, 40, 0, 0)]       # 15 | 17 taps
WINDOW_EDGE_TAPS = [7, 7, 9, 9, 15, 15, 17, 17]
FAR = [(40, 2400, 0, 0)]                                                                       # 31 taps
DRIVERS = [(683, 1024, 1, 16), (1024, 683, 1, 16), (768, 1024, 1, 16)]
ALIGNMENT = [(37, 40, 1, 8), (37, 41, 1, 8), (37, 42, 1, 8), (37, 43, 1, 8)]                   # 3W mod 4 = 0, 3, 2, 1
ALL_PAD = PAD_GEOMETRY + IDENTITY + WINDOW_EDGES + FAR + DRIVERS + ALIGNMENT
