"""Plain numpy restatement of the panel kernel of attwarp_amd/csrc/panel.hip: the byte conversion with its
value policy, the heat row (per-image maximum, normalisation, torch's bilinear with align_corners=False) and
torchvision.utils.make_grid's geometry.  Every float32 operation is one numpy float32 operation: individually rounded, no
contraction.  Sources are numpy arrays [N,C,H,W] (float32 or uint8, C 3 or 1) or ``Heat(A)`` with A float32 [N,1,h,w]."""
import numpy as np

MAX_SRC = 8
MAX_HEAT = 4096
f32 = np.float32


class Heat:
    def __init__(self, A):
        self.A = np.asarray(A)


def to_byte(v, clamp=False):
    """float32 array -> uint8: (unsigned char)(v * 255.0f), truncated toward zero, where torch defines it (-1 < t < 256);
    t <= -1 -> 0, t >= 256 -> 255, NaN -> 0.  ``clamp``: v clamped to [0, 1] first (a NaN stays NaN and becomes 0)."""
    v = np.asarray(v, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        if clamp:
            v = np.minimum(np.maximum(v, f32(0)), f32(1))      # (np.maximum / np.minimum propagate NaN)
        t = v * f32(255.0)
        ok = (t > f32(-1.0)) & (t < f32(256.0))
        out = np.where(t >= f32(256.0), 255, 0).astype(np.uint8)
        out[ok] = np.trunc(t[ok]).astype(np.int32).astype(np.uint8)
    return out


def taps(n_in, n_out):
    """torch's area_pixel_compute_source_index (align_corners=False) for every output index -> (i0, i1, l0, l1)."""
    scale = f32(n_in) / f32(n_out)
    dst = np.arange(n_out, dtype=f32)
    src = np.maximum(scale * (dst + f32(0.5)) - f32(0.5), f32(0))
    assert src.dtype == f32
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(f32)
    l0 = f32(1) - l1
    return i0, i1, l0.astype(f32), l1.astype(f32)


def heat_values(A, H, W):
    """One map [h,w] float32 -> the float32 [H,W] values the heat row converts: A / (max(A) + 1e-6f) (a NaN anywhere makes
    the maximum NaN, as amax does), then the four-tap sum l0y * (l0x*a + l1x*b) + l1y * (l0x*c + l1x*d)."""
    A = np.asarray(A, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.max(A)                                        # np.max propagates NaN
        q = (A / (m + f32(1e-6))).astype(f32)
        y0, y1, ly0, ly1 = taps(A.shape[0], H)
        x0, x1, lx0, lx1 = taps(A.shape[1], W)
        top = lx0[None, :] * q[y0][:, x0] + lx1[None, :] * q[y0][:, x1]
        bot = lx0[None, :] * q[y1][:, x0] + lx1[None, :] * q[y1][:, x1]
        v = ly0[:, None] * top + ly1[:, None] * bot
    assert v.dtype == f32
    return v


def heat_bytes(A, H, W):
    return to_byte(heat_values(A, H, W))


def geometry(K, H, W, nrow, padding=2, right_margin=0):
    """make_grid's geometry (torchvision/utils.py) -> (xmaps, ymaps, padding used, Hg, Wg + right_margin).  A single image
    is returned as it is: no padding."""
    pad = 0 if K == 1 else padding
    xmaps = min(nrow, K)
    ymaps = -(-K // xmaps)
    return xmaps, ymaps, pad, ymaps * (H + pad) + pad, xmaps * (W + pad) + pad + right_margin


def place(cells, nrow, padding=2, pad_value=0, right_margin=0):
    """make_grid of uint8 cells [K,3,H,W] -> uint8 [3, Hg, Wg + right_margin]."""
    K, _, H, W = cells.shape
    xmaps, ymaps, pad, Hg, Wt = geometry(K, H, W, nrow, padding, right_margin)
    out = np.full((3, Hg, Wt), pad_value, dtype=np.uint8)
    for k in range(K):
        y, x = (k // xmaps) * (H + pad) + pad, (k % xmaps) * (W + pad) + pad
        out[:, y:y + H, x:x + W] = cells[k]
    return out


def row_cells(row, n, H, W, clamp=False):
    """The first n images of one source as uint8 [n,3,H,W]."""
    if isinstance(row, Heat):
        A = row.A
        assert A.dtype == f32 and A.ndim == 4 and A.shape[1] == 1 and A.shape[0] >= n and A.shape[2] * A.shape[3] <= MAX_HEAT
        b = np.stack([heat_bytes(A[i, 0], H, W) for i in range(n)])[:, None]
    else:
        row = np.asarray(row)
        assert row.ndim == 4 and row.shape[0] >= n and row.shape[1] in (1, 3) and row.shape[2:] == (H, W)
        b = row[:n] if row.dtype == np.uint8 else to_byte(row[:n], clamp)
    return np.broadcast_to(b, (n, 3, H, W))


def make_grid_u8(rows, n, H, W, nrow=None, padding=2, pad_value=0, layout="hwc", clamp=False, right_margin=0):
    assert 1 <= len(rows) <= MAX_SRC and n >= 1
    clamps = [clamp] * len(rows) if isinstance(clamp, bool) else list(clamp)
    cells = np.concatenate([row_cells(r, n, H, W, c) for r, c in zip(rows, clamps)])
    chw = place(cells, n if nrow is None else nrow, padding, pad_value, right_margin)
    return chw if layout == "chw" else np.ascontiguousarray(chw.transpose(1, 2, 0))
