"""Inputs shared by the PNG encoder's tests (test_png_ref_cpu.py runs them through the restatement, test_png_gpu.py through
the kernels): small images at the sizes where the encoder changes path."""
from __future__ import annotations

import functools

import numpy as np

import png_ref as R

RUN_LENGTHS = [1, 2, 3, 4, 257, 258, 259, 260, 261, 262, 516, 517]
GEOMETRY_W, GEOMETRY_C = 85, 3                      # rows of 256 filtered bytes: 96 rows per segment
ROWS_PER_SEG = R.rows_per_segment(1 + GEOMETRY_W * GEOMETRY_C)


def _rng(seed):
    return np.random.default_rng(5200 + seed)


def photo(h, w, c, seed=0):
    """Smooth gradients with a little noise: compressible, every literal in use."""
    rng = _rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = [(96 + 80 * np.sin(xx / (7.0 + k)) * np.cos(yy / (11.0 + 2 * k)) + rng.normal(0, 2.0, (h, w))) for k in range(c)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def ramp(h, w, c):
    xx = np.arange(w)[None, :, None]
    yy = np.arange(h)[:, None, None]
    k = np.arange(c)[None, None, :]
    return ((3 + 2 * k) * xx + (k + 1) * yy + 40 * k).astype(np.uint8)


def checker(h, w, c):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((xx // 3 + yy // 2) & 1) * 200 + 20).astype(np.uint8)[:, :, None], c, 2)


def noise(h, w, c, seed=1):
    return _rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def runs_image():
    """One grey row under filter "none": runs of exactly RUN_LENGTHS equal bytes, neighbours different."""
    row = np.concatenate([np.full(n, 10 + k, np.uint8) for k, n in enumerate(RUN_LENGTHS)])
    return np.stack([row, row[::-1]])[:, :, None]


def fibonacci_image():
    """Grey, three rows, filter "none": no two equal neighbours, so every byte is a literal and the histogram is the
    Fibonacci numbers F1 .. F17 exactly -- end of block 1, the three filter-type bytes 3, and 15 pixel values with the
    other counts (4176 pixels) -- whose Huffman tree is 16 deep."""
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    counts = [c for c in fib[1:] if c != 3]          # F2 .. F17 without the 3
    n = sum(counts)
    vals = np.concatenate([np.full(c, 1 + k, np.uint8) for k, c in reversed(list(enumerate(counts)))])   # most frequent first
    arr = np.zeros(n, np.uint8)
    arr[0::2] = vals[:(n + 1) // 2]
    arr[1::2] = vals[(n + 1) // 2:]
    assert (arr[1:] != arr[:-1]).all()
    return arr.reshape(3, n // 3)[:, :, None]


def adaptive_image():
    """Rows that favour different filters: small noise (none), horizontal ramps (sub), repeated rows (up), a diagonal."""
    rng = _rng(7)
    w = 67
    a = rng.integers(0, 3, (6, w, 3), dtype=np.uint8)
    b = ramp(6, w, 3) * 0 + (np.arange(w)[None, :, None] * 5 + rng.integers(0, 255, (6, 1, 3))).astype(np.uint8)
    c = np.repeat(rng.integers(0, 256, (1, w, 3), dtype=np.uint8), 6, 0)
    yy, xx = np.mgrid[0:6, 0:w]
    d = np.repeat(((xx * 7 + yy * 9) & 255).astype(np.uint8)[:, :, None], 3, 2)
    return np.concatenate([a, b, c, d])


def ragged_batch():
    """40 images from 1 x 1 to 200 x 333, grey and RGB never mixed in a tensor but mixed in the batch."""
    rng = _rng(11)
    out = []
    for i in range(40):
        h = 1 + (199 * i * i) // (39 * 39)
        w = 1 + (332 * i * i) // (39 * 39)
        c = 1 if i % 5 == 4 else 3
        kind = i % 4
        im = photo(h, w, c, i) if kind == 0 else noise(h, w, c, i) if kind == 1 else ramp(h, w, c) if kind == 2 else \
            np.full((h, w, c), int(rng.integers(0, 256)), np.uint8)
        out.append(im)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, image [H,W,C], filter, order)]"""
    c = []
    c += [("1x1_grey", np.array([[[37]]], np.uint8), "sub", "rgb"), ("1x1_rgb", np.array([[[1, 2, 3]]], np.uint8), "sub", "rgb"),
          ("1xW", photo(1, 37, 3), "sub", "rgb"), ("Hx1", photo(41, 1, 3), "sub", "rgb"),
          ("Hx1_grey_paeth", photo(1500, 1, 1), "paeth", "rgb")]
    c += [(f"w{w}", photo(9, w, 3, w), "sub", "rgb") for w in (1, 2, 3, 5, 85, 86)]
    g = ROWS_PER_SEG
    c += [("one_segment", photo(g, GEOMETRY_W, GEOMETRY_C), "sub", "rgb"),
          ("segment_plus_row", photo(g + 1, GEOMETRY_W, GEOMETRY_C), "up", "rgb"),
          ("last_segment_one_row", photo(2 * g + 1, GEOMETRY_W, GEOMETRY_C), "paeth", "rgb"),
          ("max_row_bytes", photo(2, R.MAX_ROW_BYTES - 1, 1), "sub", "rgb")]
    c += [("runs", runs_image(), "none", "rgb"), ("all_zero", np.zeros((300, 300, 3), np.uint8), "sub", "rgb"),
          ("constant_sub", np.full((50, 61, 3), 77, np.uint8), "sub", "rgb"),
          # one literal + end of block means a run of at most 3 bytes, which the 153-byte block header always sends down
          # the stored fallback: this case exercises the two-symbol code lengths and the size decision, not the dynamic
          # emitter (all_zero and constant_sub emit dynamic blocks of two literals plus matches)
          ("single_symbol", np.zeros((1, 2, 1), np.uint8), "none", "rgb"),
          ("fibonacci", fibonacci_image(), "none", "rgb"),
          ("noise_stored", noise(97, 131, 3), "sub", "rgb")]
    for f in R.FILTERS:
        for ch in (3, 1):
            c += [(f"{f}_ramp_c{ch}", ramp(40, 67, ch), f, "rgb"), (f"{f}_checker_c{ch}", checker(40, 67, ch), f, "rgb"),
                  (f"{f}_noise_c{ch}", noise(40, 67, ch, 3), f, "rgb")]
    c += [("adaptive_rows", adaptive_image(), "adaptive", "rgb"), ("bgr", photo(23, 31, 3, 5), "paeth", "bgr")]
    return c


@functools.lru_cache(maxsize=None)
def _ref_cached(key):
    name, filt, order = key
    img = next(i for n, i, f, o in cases() if (n, f, o) == key)
    return R.encode(img, filt, order)


def reference(name, filt, order):
    """The restatement's file for a case, computed once per process."""
    return _ref_cached((name, filt, order))
