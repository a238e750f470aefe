"""Inputs of tests/test_axis_limits_gpu.py: the per-axis and profile kernels at the sizes their launchers document as limits
(16384 elements per axis, 8192 for the fused kernels, a low-resolution side of 64, a grid side of 64 or 26, 65535 images per
launch).  Every case is a thin array -- a limit on one axis, a handful of elements on the other -- built from a fixed
seed, with the property its name claims; tests/test_axis_limits_cpu.py checks those properties without a GPU."""
import functools

import numpy as np

from oracle import warp_oracle as O

F32 = np.float32

MAX_L = 16384            # attwarp_{cdf_from_density, make_strictly_increasing, axis_map_from_cdf, safe_softmax}, profiles
FUSED_MAX_L = 8192       # attwarp_axis_maps_from_pdf, attwarp_axis_maps_from_steps, attwarp_attn_reduce_and_maps
MAX_LO = 64              # low-resolution PDF length / grid side of the fused kernels
MAX_B = 65535            # images per launch (grid.y / grid.x)
AM_MAX_G = 26            # attn_reduce_and_maps: g*g a multiple of 4 and <= 768

# 64 KiB of dynamic LDS is passed at 8192 doubles, at 16369 floats behind the 64-byte reduction scratch, and at 16384 floats
AXIS_LENGTHS = (8191, 8192, 8193, 16368, 16369, 16383, 16384)
RESAMPLE_NL = ((24, 16384), (16384, 24), (8192, 8192), (8192, 8193), (16384, 16384), (1, 16384), (16384, 1))
MAP_N_OUT = (1, 500, 16384)
ATT_HW = ((3, 16384), (16384, 8), (5, 16383), (16381, 5), (4, 8200), (6, 12296), (16384, 4))
ATT_OUT_WH = ((500, 400), (16384, 3))          # (new_width, new_height)
POOL_W = (16384, 16383)


def _frozen(a: np.ndarray) -> np.ndarray:
    a.flags.writeable = False
    return a


# ---- numpy's pairwise summation plan, restated (attwarp_amd/csrc/profiles_blocks.hpp: pw_build) -----------------------------
def pairwise_plan(n: int):
    """(leaves, depth): the (offset, length) leaves of np.sum over n contiguous elements -- n <= 128 is a leaf, otherwise
    n2 = n/2 - (n/2) % 8 and the two halves recurse -- and the deepest stack of the postfix program that adds them."""
    leaves, prog = [], []

    def rec(off, m):
        if m <= 128:
            leaves.append((off, m))
            prog.append(0)
        else:
            m2 = m // 2
            m2 -= m2 % 8
            rec(off, m2)
            rec(off + m2, m - m2)
            prog.append(1)

    rec(0, int(n))
    sp = depth = 0
    for p in prog:
        sp += 1 if p == 0 else -1
        depth = max(depth, sp)
    return leaves, depth


# ---- part 1: unfused per-axis kernels ------------------------------------------------------------------------------
DENSITY_ROWS = ("random", "sequential", "spike", "zero")


@functools.lru_cache(maxsize=None)
def densities(L: int) -> np.ndarray:
    """[4, L] float32, rows as DENSITY_ROWS: random values in [0.25, 1) (every normalised value far above 2^-28: the
    parallel scan), every third value 1e-13 (the sequential scan), one spike plus a denormal, all zero."""
    rng = np.random.default_rng(71000 + L)
    p = (0.25 + 0.75 * rng.random((4, L))).astype(F32)
    p[1, ::3] = 1e-13
    p[2] = 0
    p[2, L // 2] = 1.0
    p[2, min(5, L - 1)] = 3e-39
    p[3] = 0
    return _frozen(p)


def takes_sequential_scan(p_row: np.ndarray) -> bool:
    """The kernel's rule on the oracle's normalised density: a parallel scan is bit-equal to the sequential cumsum only if
    every non-zero value is >= 2^-28 (all partial sums exact in double); otherwise one lane scans."""
    p = np.asarray(p_row, F32)
    p = np.nan_to_num(np.where(np.isnan(p), F32(0), np.maximum(p, F32(0))), nan=0.0, posinf=0.0, neginf=0.0).astype(F32)
    denom = np.maximum(F32(p.astype(np.float64).sum()), F32(1e-6))
    q = (p / denom).astype(F32)
    return bool(((q != 0) & (q < F32(2.0 ** -28))).any() or not q.astype(np.float64).sum() < 2.0)


CDF_ROWS = ("monotone", "flat", "nonfinite", "decreasing")


@functools.lru_cache(maxsize=None)
def cdfs(N: int) -> np.ndarray:
    """[4, N] float32 'CDFs', rows as CDF_ROWS: a proper CDF, a constant one (every repaired step is the eps / N floor),
    the proper one with NaN / +inf / -inf planted, a decreasing ramp."""
    rng = np.random.default_rng(72000 + N)
    F = np.empty((4, N), F32)
    F[0] = O.cdf_from_density((0.05 + rng.random((1, N))).astype(F32))[0]
    F[1] = 0.5
    F[2] = F[0]
    F[2, N // 7] = np.nan
    F[2, N // 3] = np.inf
    F[2, (2 * N) // 3] = -np.inf
    F[3] = np.linspace(1.0, 0.0, N, dtype=np.float64).astype(F32)
    return _frozen(F)


MAP_ROWS = ("ties", "strict")


@functools.lru_cache(maxsize=None)
def map_cdfs(L: int):
    """(F_ties, F_strict), each [2, L] float32: CDFs of densities with runs of zeros (equal neighbouring knots: the
    tie-break ramp is taken) and of densities in [0.5, 1.5) (every knot above the one before it)."""
    rng = np.random.default_rng(73000 + L)
    p = (0.5 + rng.random((2, L))).astype(F32)
    pt = p.copy()
    pt[0, L // 4: L // 2] = 0
    pt[1, ::2] = 0
    return _frozen(O.cdf_from_density(pt)), _frozen(O.cdf_from_density(p))


SOFTMAX_ROWS = ("pm80", "nonfinite", "constant", "random")


@functools.lru_cache(maxsize=None)
def logits(N: int) -> np.ndarray:
    """[4, N] float32, rows as SOFTMAX_ROWS: +-80 (exp(-160) underflows float32), normal values with NaN / +inf / -inf
    planted (each counts as 0), one constant, normal values."""
    rng = np.random.default_rng(74000 + N)
    x = rng.standard_normal((4, N)).astype(F32)
    x[0] = np.where(rng.random(N) < 0.5, F32(80), F32(-80))
    x[0, N - 1] = 80
    x[1, N // 5] = np.nan
    x[1, N // 2] = np.inf
    x[1, N - 1] = -np.inf
    x[2] = 3.25
    return _frozen(x)


# ---- part 2: profile kernels ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attention(h: int, w: int, dtype: str) -> np.ndarray:
    """[2, h, w] attention maps: uint8 bytes, float32 in [-0.5, 2.5) (negatives are clamped), float64 in [0, 1)."""
    rng = np.random.default_rng(75000 + 3 * h + w)
    if dtype == "uint8":
        a = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    elif dtype == "float32":
        a = (rng.random((2, h, w), dtype=F32) * F32(3.0) - F32(0.5)).astype(F32)
    else:
        a = rng.random((2, h, w))
    return _frozen(a)


@functools.lru_cache(maxsize=None)
def marginal_maps(h: int, w: int) -> np.ndarray:
    """[3, 1, h, w] float32 for gt_marginals: the float32 attention plus one image with a NaN and one with +inf."""
    a = attention(h, w, "float32")
    A = np.stack([a[0], a[1], a[0]])[:, None].copy()
    A[1, 0, h // 3, w // 5] = np.nan
    A[2, 0, h // 2, w // 2] = np.inf
    return _frozen(A)


@functools.lru_cache(maxsize=None)
def pool_maps(W: int) -> np.ndarray:
    """[2, 1, 5, W] float32 for adaptive_avg_pool."""
    rng = np.random.default_rng(76000 + W)
    return _frozen((rng.random((2, 1, 5, W), dtype=F32) * F32(4.0) - F32(1.0)).astype(F32))


# ---- part 3: fused kernels ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def low_res_pdfs(Lo: int):
    """(px, py), each [2, Lo] float32 rows that sum to 1."""
    rng = np.random.default_rng(77000 + Lo)
    px = rng.random((2, Lo), dtype=F32) ** 2 + F32(1e-3)
    py = rng.random((2, Lo), dtype=F32) ** 2 + F32(1e-3)
    return _frozen((px / px.sum(1, keepdims=True)).astype(F32)), _frozen((py / py.sum(1, keepdims=True)).astype(F32))


def pdf_chain(px: np.ndarray, py: np.ndarray, H: int, W: int, out_size=None):
    """The oracle chain axis_maps_from_pdf fuses: right-inverse up-sample, clamp, CDF, inverse maps."""
    Fx = O.cdf_from_density(np.maximum(O.upsample_pdf_right_inverse(px, W), 0))
    Fy = O.cdf_from_density(np.maximum(O.upsample_pdf_right_inverse(py, H), 0))
    return O.maps_from_cdf(Fx, Fy, out_size)


@functools.lru_cache(maxsize=None)
def step_maps(g: int) -> np.ndarray:
    """[3, 2, g*g] float32 per-step attention maps (rows sum to 1)."""
    rng = np.random.default_rng(78000 + g)
    s = rng.random((3, 2, g * g), dtype=F32) ** 3 + F32(1e-4)
    return _frozen((s / s.sum(-1, keepdims=True)).astype(F32))


def steps_chain(steps: np.ndarray, g: int, H: int, W: int, out_size=None):
    """The oracle chain axis_maps_from_attention_steps fuses, from float32 or float16 step maps."""
    B = steps.shape[1]
    att = O.attn_finalize([s for s in steps]).astype(F32).reshape(B, 1, g, g)
    qx, qy = O.gt_marginals(att)
    return pdf_chain(qx, qy, H, W, out_size)


# ---- part 4: the batch edge -----------------------------------------------------------------------------------------
def batch_sources(B: int = MAX_B) -> np.ndarray:
    """Image b of a batch of B is distinct image src[b] of six: five tiled over the batch, the sixth in the last place."""
    src = (np.arange(B) % 5).astype(np.int64)
    src[-1] = 5
    return src


@functools.lru_cache(maxsize=None)
def six_maps() -> np.ndarray:
    """[6, 8, 8] float32, six distinct images."""
    rng = np.random.default_rng(79000)
    return _frozen((rng.random((6, 8, 8), dtype=F32) ** 2).astype(F32))


@functools.lru_cache(maxsize=None)
def six_step_maps() -> np.ndarray:
    """[2, 6, 4] float32 step maps of a 2 x 2 grid for six distinct images."""
    rng = np.random.default_rng(79001)
    s = rng.random((2, 6, 4), dtype=F32) + F32(0.05)
    return _frozen((s / s.sum(-1, keepdims=True)).astype(F32))
