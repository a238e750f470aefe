"""A reference for pipeline.clip_preprocess that shares nothing with the product: Pillow itself resizes (one mode-"L" image
per channel, Image.BICUBIC), numpy crops, rescales and normalises.  No table of attwarp_amd._tables and no coefficient of
oracle.warp_oracle is read here, so an error those two share cannot hide.  tests/test_clip_ref_cpu.py ties this reference
to oracle.clip_preprocess (which the goldens tie to the HF processor) on every RGB case below.

Also here: the seeded input patterns of the sweep, route() -- the launcher's choice between the LDS-staged kernels
and the one-thread-per-output pair (both csrc/clip.hip) restated in Python, so that every case can assert that
it reaches the path it is named for -- and the case lists that tests/test_clip_sweep_gpu.py runs."""
import math
from collections import namedtuple

import numpy as np
from PIL import Image

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
# per-channel constants of the sweep: all different, one mean negative, one std above 1
SWEEP_MEAN = (0.4, -0.5, 0.6, 0.7)
SWEEP_STD = (0.2, 3.0, 0.25, 0.35)


# ---- geometry and reference ------------------------------------------------------------------------------------------------
def geometry(H, W, size):
    """(nh, nw, top, left): shorter edge to ``size``, long edge int(size * long / short), centre crop origin."""
    short, long_ = (H, W) if H <= W else (W, H)
    new_long = int(size * long_ / short)
    nh, nw = (size, new_long) if H <= W else (new_long, size)
    return nh, nw, (nh - size) // 2, (nw - size) // 2


def resize_crop_u8(img_u8, size):
    """uint8 [H,W,C] -> uint8 [size,size,C]: Pillow's BICUBIC resize of every channel on its own, then the centre crop."""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W, C = img.shape
    nh, nw, top, left = geometry(H, W, size)
    out = np.empty((size, size, C), dtype=np.uint8)
    for c in range(C):
        band = Image.fromarray(np.ascontiguousarray(img[:, :, c]))
        assert band.mode == "L"
        r = np.asarray(band.resize((nw, nh), Image.BICUBIC))
        assert r.shape == (nh, nw)
        out[:, :, c] = r[top:top + size, left:left + size]
    return out


def normalize(crop_u8, mean, std):
    """uint8 [size,size,C] -> float32 [C,size,size]: float32(float64(u8) * (1/255)), then (x - mean) / std in float32."""
    C = crop_u8.shape[2]
    x = (crop_u8.astype(np.float64) * (1 / 255)).astype(np.float32)
    m = np.array(mean[:C], dtype=np.float32)
    s = np.array(std[:C], dtype=np.float32)
    x = ((x - m).astype(np.float32) / s).astype(np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def clip_preprocess(img_u8, size, mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD):
    return normalize(resize_crop_u8(img_u8, size), mean, std)


# ---- the launcher's route ---------------------------------------------------------------------------------------------------
def taps(n_in, n_out):
    """Pillow's ksize for BICUBIC (support 2): 2 * ceil(2 * max(in / out, 1)) + 1."""
    return 2 * int(math.ceil(2.0 * max(n_in / n_out, 1.0))) + 1


Route = namedtuple("Route", "ksize_x ksize_y RB oc route nh nw top left")

NT, NQ, NS, LDS = 256, 2, 8, 48 * 1024


def kernels(W, C, size, ksize_x):
    """The launcher's choice for source rows of W pixels and tables of ksize_x columns: (name, RB, oc)."""
    wc, oc = W * C, size * C
    wcp, ocp = (wc + 3) & ~3, (oc + 3) & ~3
    RB = min(8, LDS // (wcp + ocp))
    lds_v = C * 256 * 4 + oc * 4
    generic = (C == 2 or RB < 1 or ksize_x > 16 or oc % 4 != 0 or oc > 4 * NT * NQ or oc > NT * NS or lds_v > LDS)
    return "generic" if generic else ("staged8" if ksize_x <= 8 else "staged16"), RB, oc


def route(H, W, C, size):
    """What attwarp_clip_preprocess_u8 does with a [B,H,W,C] batch (the tmp buffer 4-byte aligned, no variant forced).
    ksize_x / ksize_y are Pillow's tap counts; the tables reach the launcher padded to at least 8 columns.  RB: source
    rows per workgroup of the staged horizontal pass, from its LDS budget (0: a row does not fit)."""
    nh, nw, top, left = geometry(H, W, size)
    kx, ky = taps(W, nw), taps(H, nh)
    name, RB, oc = kernels(W, C, size, max(kx, 8))
    return Route(kx, ky, RB, oc, name, nh, nw, top, left)


# ---- tables that fill every coefficient register ------------------------------------------------------------------------------
def full_tables(n_in, n_out, ks, seed):
    """Hand-made 22-bit tables in Pillow's layout whose rows all have exactly ``ks`` non-zero taps (Pillow's own BICUBIC
    rows have an odd number, 15 at the most on the staged route: the 8th and the 16th register stay zero there).  Weights
    in [0.5, 1), every fourth one times -0.25, normalised to 2^22 like Pillow's; int32 (bounds [n_out,2], kk [n_out,ks])."""
    assert ks <= n_in
    rng = np.random.default_rng([seed, n_in, n_out, ks])
    w = rng.uniform(0.5, 1.0, (n_out, ks))
    w[:, 1::4] *= -0.25                                       # negative lobes: sum |w| <= 1.4 * sum w
    kk = np.rint(w / w.sum(axis=1, keepdims=True) * (1 << 22)).astype(np.int32)
    assert (kk != 0).all() and (kk < 0).any()
    assert (np.abs(kk.astype(np.int64)).sum(axis=1) * 255 + (1 << 21) < 2 ** 31).all()      # the int32 accumulator holds
    first = (np.arange(n_out) * (n_in - ks)) // max(n_out - 1, 1)
    bounds = np.stack([first, np.full(n_out, ks)], axis=1).astype(np.int32)
    return bounds, kk


def resample_u8(src, bounds, kk, lo, n):
    """Pillow's 8-bit pass along the LAST axis in int64 for the output positions lo .. lo + n - 1."""
    s = src.astype(np.int64)
    out = np.empty(src.shape[:-1] + (n,), dtype=np.uint8)
    for i in range(n):
        first, cnt = int(bounds[lo + i, 0]), int(bounds[lo + i, 1])
        acc = np.full(src.shape[:-1], 1 << 21, dtype=np.int64)
        for t in range(cnt):
            acc += s[..., first + t] * int(kk[lo + i, t])
        out[..., i] = np.clip(acc >> 22, 0, 255)
    return out


# ---- input patterns ---------------------------------------------------------------------------------------------------------
PATTERNS = ("noise", "extremes", "blocks", "ramp", "white", "black")


def block_side(H, W, size):
    """Side of the ``blocks`` squares: twice the reduction factor, so that an edge sits inside most windows of the filter
    and its negative lobes drive the accumulator below 0 and above 255."""
    return 2 * int(math.ceil(max(min(H, W) / size, 1.0)))


def pattern(name, H, W, C, size, seed=0):
    """One uint8 [H,W,C] image."""
    rng = np.random.default_rng([seed, H, W, C, PATTERNS.index(name)])
    if name == "noise":
        return rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if name == "extremes":
        return (rng.integers(0, 2, (H, W, C), dtype=np.uint8) * np.uint8(255)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "blocks":
        s = block_side(H, W, size)
        board = ((((xx // s) + (yy // s)) & 1) * 255).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(board[:, :, None], C, axis=2))
    if name == "ramp":
        return np.stack([((7 * xx + 13 * yy + 85 * c) & 255).astype(np.uint8) for c in range(C)], axis=2)
    if name == "white":
        return np.full((H, W, C), 255, dtype=np.uint8)
    if name == "black":
        return np.zeros((H, W, C), dtype=np.uint8)
    raise ValueError(name)


def batch(H, W, C, size, names, seed=0):
    """uint8 [len(names),H,W,C], image b drawn from pattern names[b] (seed + b: two noise images differ)."""
    return np.stack([pattern(n, H, W, C, size, seed + b) for b, n in enumerate(names)])


# ---- the sweep's cases: (H, W, C, size, route, RB) --------------------------------------------------------------------------
Case = namedtuple("Case", "H W C size route RB")

TAP_EDGES = [                                  # taps x / y
    Case(48, 48, 3, 32, "staged8", 8),         # 7 / 7: the last KS = 8 shape
    Case(49, 49, 3, 32, "staged16", 8),        # 9 / 9: the first KS = 16 shape
    Case(112, 112, 3, 32, "staged16", 8),      # 15 / 15: the last KS = 16 shape
    Case(113, 113, 3, 32, "generic", 8),       # 17 / 17: generic by tap count
    Case(113, 112, 3, 32, "staged16", 8),      # 15 / 17: staged, the vertical 8-row loop runs three rounds
    Case(112, 120, 3, 32, "generic", 8),       # 17 / 15: generic, crop left of 1
]
TAP_EDGE_KSIZES = [(7, 7), (9, 9), (15, 15), (17, 17), (15, 17), (17, 15)]

SMALL = [
    Case(20, 20, 3, 32, "staged8", 8),         # 5 taps padded to 8: the vertical ksize == 8 branch, rows clamped
    Case(32, 40, 3, 32, "staged8", 8),         # both axes keep their size (identity tables), crop left of 4
    Case(40, 32, 3, 32, "staged8", 8),         # the same, crop top of 4
    Case(1, 1, 3, 32, "staged8", 8),
    Case(1, 7, 3, 32, "staged8", 8),
    Case(7, 1, 3, 32, "staged8", 8),
    Case(2, 3, 3, 32, "staged8", 8),
]

CHANNELS = [
    Case(96, 90, 1, 32, "staged16", 8),        # 13 taps
    Case(97, 131, 4, 32, "staged16", 8),       # 15 taps, crop left of 5
    Case(50, 60, 2, 32, "generic", 8),         # C == 2 is always generic
]

WIDE = [
    Case(700, 690, 3, 680, "staged8", 8),      # ow > 384 (second xx pass), ow*C/4 > 256 (both NQ dwords)
    Case(600, 560, 3, 400, "staged8", 8),
    Case(600, 560, 4, 512, "staged8", 8),      # oc = 2048: exactly the limit
    Case(530, 520, 1, 512, "staged8", 8),      # two xx passes
    Case(700, 690, 3, 682, "generic", 8),      # oc % 4 != 0
    Case(700, 690, 3, 683, "generic", 8),      # oc > 2048
]

LDS_ROWS = [
    Case(64, 2100, 3, 32, "staged16", 7),
    Case(40, 16000, 3, 32, "staged8", 1),
    Case(40, 16352, 3, 32, "staged8", 1),      # wcp + ocp = 49152: the largest staged row
    Case(40, 16380, 3, 32, "generic", 0),      # a row no longer fits
    Case(13, 600, 3, 32, "staged8", 8),        # a second workgroup of 5 rows
]

ALIGNMENT = [
    Case(48, 48, 3, 32, "staged8", 8),         # rows of 144 bytes: dword staging unless the pointer is odd
    Case(33, 47, 3, 32, "staged8", 8),         # images of 4653 bytes: image 1 starts on an odd byte
]
PAD_TO_SQUARE = [(48, 61), (61, 48)]           # both become 61 x 61: 9 taps
PAD_ROUTE = "staged16"

ALL_CASES = TAP_EDGES + SMALL + CHANNELS + WIDE + LDS_ROWS + ALIGNMENT

# pattern sets: every case sees saturating edges, a channel-distinct ramp and noise; small cases also the flat ones
SET_A = ("blocks", "ramp", "noise")
SET_B = ("extremes", "white", "black")


def check_route(case):
    """The case reaches the path it is named for."""
    r = route(case.H, case.W, case.C, case.size)
    assert (r.route, r.RB) == (case.route, case.RB), (case, r)
    return r
