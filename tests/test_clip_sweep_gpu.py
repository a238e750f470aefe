"""GPU sweep of pipeline.clip_preprocess against Pillow itself (tests/clip_ref.py) on every route its launcher takes: the
LDS-staged kernels of csrc/clip.hip with 8 and with 16 coefficient registers, and the one-thread-per-output pair of
the same file.  tests/test_gpu_parity.py pins the operating point (500 x 500 -> 336, RGB, noise) to the HF processor; here
are the tap counts where the variant changes, up-scaling and one-pixel sources, C = 1, 2, 4, outputs wider than one pass of
either staged kernel, every rows-per-workgroup class of the LDS budget, and source pointers off a 4-byte boundary.

Every case asserts, through clip_ref.route, that it reaches the path it is named for, then runs a batch whose images come
from different patterns (checkerboards that drive both passes past both clamps -- tests/test_clip_ref_cpu.py counts them --
a ramp that differs per channel, noise; for the small shapes also random 0 / 255 bytes, white and black) with per-channel
mean / std that are all different, and for RGB also with the OpenAI constants.  Bit for bit:
  (a) float32 on the route the launcher chooses == clip_ref,
  (b) float32 with the generic kernels forced (clip_variant=1) == clip_ref,
  (c) float16 on both == clip_ref(...).astype(float16)."""
import contextlib

import numpy as np
import pytest
import torch

import clip_ref as R
from attwarp_amd import _lib
from oracle import warp_oracle as O
from test_gpu_parity import N, T, dev  # noqa: F401  (dev is the module's GPU fixture)

pytestmark = pytest.mark.gpu

DEFAULTS = (R.OPENAI_CLIP_MEAN, R.OPENAI_CLIP_STD)


def _ids(c):
    return "%dx%dx%d-%d" % (c.H, c.W, c.C, c.size)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype)
    bits = np.uint32 if want.dtype == np.float32 else np.uint16
    bad = np.argwhere(got.view(bits) != want.view(bits))
    if len(bad):
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} elements differ from Pillow, first at (b, c, y, x) = {i}: "
                             f"{float(got[i])!r} != {float(want[i])!r}")


def _check(x, crops, size, consts, what, **kw):
    """(a), (b), (c) for the device batch ``x`` whose Pillow-resized, cropped uint8 images are ``crops``."""
    from attwarp_amd import pipeline
    C = crops[0].shape[2]
    for mean, std in consts:
        want = np.stack([R.normalize(c, mean, std) for c in crops])
        want16 = want.astype(np.float16)
        for forced in (False, True):
            with (_lib.debug_override(clip_variant=1) if forced else contextlib.nullcontext()):
                g32 = pipeline.clip_preprocess(x, size, torch.float32, mean, std, **kw)
                g16 = pipeline.clip_preprocess(x, size, torch.float16, mean, std, **kw)
            tag = f"{what} mean={mean[:C]} {'generic forced' if forced else 'default route'}"
            _same(N(g32), want, tag + " float32")
            _same(N(g16), want16, tag + " float16")


def _run_case(dev, case, sets, seed):
    R.check_route(case)
    consts = [(R.SWEEP_MEAN[:case.C], R.SWEEP_STD[:case.C])] + ([DEFAULTS] if case.C == 3 else [])
    for names in sets:
        imgs = R.batch(case.H, case.W, case.C, case.size, names, seed)
        crops = [R.resize_crop_u8(im, case.size) for im in imgs]
        _check(T(imgs, dev), crops, case.size, consts, f"{_ids(case)} {names}")


@pytest.mark.parametrize("case", R.TAP_EDGES, ids=_ids)
def test_tap_edges(dev, case):
    """7 | 9 taps (8 to 16 coefficient registers) and 15 | 17 (staged to generic), and the two shapes whose axes fall on
    different sides of 16 | 17: the staged route takes any vertical tap count."""
    _run_case(dev, case, (R.SET_A, R.SET_B), 11)


@pytest.mark.parametrize("case", R.SMALL, ids=_ids)
def test_upscaling_identity_tiny(dev, case):
    """Fewer than 8 taps (tables padded to 8: the vertical kernel's ksize == 8 branch, tap rows clamped to the image),
    axes that keep their size, sources of one to three pixels."""
    _run_case(dev, case, (R.SET_A, R.SET_B), 12)


@pytest.mark.parametrize("case", R.CHANNELS, ids=_ids)
def test_channels(dev, case):
    """One and four channels on the 16-register variant, two channels (always generic), each with its own mean / std."""
    _run_case(dev, case, (R.SET_A, R.SET_B), 13)


@pytest.mark.parametrize("case", R.WIDE, ids=_ids)
def test_wide_outputs(dev, case):
    """Outputs wider than 384 pixels (the horizontal kernel's second pixel per thread) and than 1024 bytes (the vertical
    kernel's second dword per thread), ow * C at 2048 exactly, and just past the two limits that send a shape to the
    generic kernels (ow * C % 4 != 0, ow * C > 2048)."""
    _run_case(dev, case, (R.SET_A,), 14)


@pytest.mark.parametrize("case", R.LDS_ROWS, ids=_ids)
def test_lds_rows(dev, case):
    """Rows per workgroup of the staged horizontal pass as its LDS budget sets them: 7, 1, 1 with the largest row that
    fits (49152 + 128 bytes of dynamic LDS), 0 (generic), and 8 with a last workgroup of 5 rows."""
    _run_case(dev, case, (R.SET_A,), 15)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_source_off_dword_boundary(dev, off):
    """Rows of 144 bytes, a whole number of dwords, behind a pointer that is not: the byte-staging branch by address."""
    case = R.ALIGNMENT[0]
    R.check_route(case)
    assert case.W * case.C % 4 == 0
    imgs = R.batch(case.H, case.W, case.C, case.size, R.SET_A, 16)
    buf = torch.zeros(imgs.size + 8, dtype=torch.uint8, device=dev)
    x = buf[off:off + imgs.size].view(imgs.shape)
    x.copy_(T(imgs, dev))
    assert x.is_contiguous() and x.data_ptr() % 4 == off
    crops = [R.resize_crop_u8(im, case.size) for im in imgs]
    _check(x, crops, case.size, [(R.SWEEP_MEAN[:3], R.SWEEP_STD[:3]), DEFAULTS], f"{_ids(case)} offset {off}")


def test_source_images_of_odd_size(dev):
    """Images of 33 * 47 * 3 = 4653 bytes: image 1 of the batch starts on an odd byte, rows are no whole dwords."""
    case = R.ALIGNMENT[1]
    assert case.H * case.W * case.C % 2 == 1
    _run_case(dev, case, (R.SET_A, R.SET_B), 17)


@pytest.mark.parametrize("hw", R.PAD_TO_SQUARE, ids=lambda hw: "%dx%d" % hw)
def test_pad_to_square(dev, hw):
    """pad_to_square=True on a wide and a tall image (odd margin): clip_ref on the oracle's expand2square."""
    H, W = hw
    n = max(H, W)
    assert R.route(n, n, 3, 32).route == R.PAD_ROUTE
    imgs = R.batch(H, W, 3, 32, R.SET_A, 18)
    crops = [R.resize_crop_u8(O.expand2square(im), 32) for im in imgs]
    _check(T(imgs, dev), crops, 32, [DEFAULTS], f"pad {H}x{W}", pad_to_square=True)


@pytest.mark.parametrize("ks", [8, 16])
def test_every_coefficient_register(dev, ks):
    """attwarp_clip_preprocess_u8 with tables whose rows all hold ks non-zero taps.  Pillow's BICUBIC rows have an odd
    count, so through pipeline.clip_preprocess the last register of either staged variant only ever holds zero; the entry
    point takes any table of up to 16 columns on the staged route.  Reference: the same integer arithmetic in int64
    (clip_ref.resample_u8), then clip_ref.normalize; random 0 / 255 bytes and a checkerboard, weights with negative
    lobes (the clamps belong to the Pillow cases above).  A crop origin of (3, 4); bit for bit on both routes, both types,
    the horizontal pass's uint8 rows included."""
    import ctypes
    from attwarp_amd._lib import call, ptr, stream_ptr
    B, H, W, C, size, top, left = 2, 41, 64, 3, 32, 3, 4
    assert R.kernels(W, C, size, ks)[0] == ("staged8" if ks == 8 else "staged16")
    imgs = R.batch(H, W, C, size, ("extremes", "blocks"), 19)
    bx, kx = R.full_tables(W, size + 2 * left, ks, 1)
    by, ky = R.full_tables(H, size + 2 * top, ks, 2)
    tmp_ref = R.resample_u8(imgs.transpose(0, 1, 3, 2), bx, kx, left, size)                  # [B,H,C,W] -> [B,H,C,size]
    crops = R.resample_u8(tmp_ref.transpose(0, 2, 3, 1), by, ky, top, size).transpose(0, 3, 2, 1)       # [B,size,size,C]
    mean, std = R.SWEEP_MEAN[:C], R.SWEEP_STD[:C]
    want = np.stack([R.normalize(c, mean, std) for c in crops])
    x, dbx, dkx, dby, dky = (T(a, dev) for a in (imgs, bx, kx, by, ky))
    m, s = (ctypes.c_float * C)(*mean), (ctypes.c_float * C)(*std)
    for forced in (False, True):
        for dt, ident, w in ((torch.float32, _lib.F32, want), (torch.float16, _lib.F16, want.astype(np.float16))):
            tmp = torch.empty(B, H, size, C, device=dev, dtype=torch.uint8)
            out = torch.empty(B, C, size, size, device=dev, dtype=dt)
            with (_lib.debug_override(clip_variant=1) if forced else contextlib.nullcontext()):
                call("attwarp_clip_preprocess_u8", ptr(x), B, H, W, C, top, left, size, ptr(dbx), ptr(dkx), ks, ptr(dby),
                     ptr(dky), ks, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), ptr(tmp), ptr(out),
                     ident, stream_ptr(dev))
            _same(N(out), w, f"{ks} full taps {'generic forced' if forced else 'default route'} {dt}")
            assert np.array_equal(N(tmp), tmp_ref.transpose(0, 1, 3, 2)), "horizontal pass"
