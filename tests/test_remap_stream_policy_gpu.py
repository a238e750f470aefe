"""The cache policy of the 1024 x 3 float32 resample (remap_rows_kernel.hpp, STREAM) changes no bit.

The streaming variant stores its output rows nontemporal; the launcher picks it only for launches larger than the
Infinity Cache.  Here the tuning flavour forces each policy (test hook ``remap_stream``: 0 cached, 1 streaming) on small
inputs of the one class that has the variant, and every result must equal the C oracle bit for bit.  Heights follow the shipped rows per block R: R + 1, 2R + 1 (a one-row last block) and R - 1."""
import os

import numpy as np
import pytest
import torch

from attwarp_amd import _lib

pytestmark = pytest.mark.gpu

B, W, C, HS = 3, 1024, 3, 24          # images per launch, row width (the only class with the variant), source height
POLICIES = (0, 1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert os.path.exists(_lib.LIB_PATH), "HIP library missing -- the product has no fallback"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle():
    from oracle import c_oracle
    c_oracle.load()
    return c_oracle


@pytest.fixture(scope="module")
def shipped():
    """the plan of the headline launch: rows per block of the class under test"""
    plan = _lib.remap_plan(256, C, 1024, W, 1024, W, "cv2")
    assert plan is not None and plan["stream"] != 0
    return plan


@pytest.fixture(scope="module")
def pixels():
    rng = np.random.default_rng(77)
    img = rng.random((B, HS, W, C), dtype=np.float32)
    mx = np.stack([np.clip(np.arange(W) + 0.37 * np.sin(np.arange(W) / (40.0 + 7 * b)) + 0.21 * b, 0, W - 1) for b in range(B)])
    return img, mx.astype(np.float32)


def row_maps(kind, Ho):
    """[B, Ho] row maps into HS source rows; image b is shifted by a fraction so the three images differ"""
    y = np.arange(Ho, dtype=np.float64)
    sh = np.array([0.0, 0.11, 0.46])[:, None]
    if kind == "near_identity":
        m = y[None] + 0.3 + sh
    elif kind == "peaked":                 # steps of two or more source rows: both rows of every output row are new
        m = 2.5 * y[None] + 0.25 + sh
    elif kind == "flat":                   # the same two source rows twice
        m = np.floor(y / 2)[None] + 0.5 + 0.25 * sh
    elif kind == "decreasing":             # up two rows, then back down one row at a time and one step of three
        up = np.array([5.4, 7.4, 6.4, 5.4, 4.4, 1.4, 0.4, 2.4, 3.4])
        m = np.resize(up, Ho)[None] + sh
    elif kind == "clamped":                # both ends outside the image: i1 == i0 at the top and at the bottom
        m = np.linspace(-2.5, HS + 1.5, Ho)[None] + sh if Ho > 1 else np.array([[-2.5]]) + sh
    else:
        raise AssertionError(kind)
    return np.ascontiguousarray(np.broadcast_to(m, (B, Ho)), dtype=np.float32)


KINDS = ("near_identity", "peaked", "flat", "decreasing", "clamped")


def run(dev, img, mx, my, mode, stream):
    from attwarp_amd import checkpoint_utils as cu
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with _lib.debug_override(remap_variant=3, remap_stream=stream):
        plan = _lib.remap_plan(img.shape[0], C, img.shape[1], W, my.shape[1], W, mode)
        assert plan is not None and plan["stream"] == stream, plan           # the forced policy is the one that runs
        out = cu.remap_separable(t(img), t(mx), t(my), mode=mode, channels_last=True)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("mode", ["exact", "cv2"])
@pytest.mark.parametrize("height", ["R+1", "2R+1", "R-1"])
def test_every_policy_equals_the_oracle(dev, oracle, shipped, pixels, mode, height):
    R = shipped["rows"]
    Ho = {"R+1": R + 1, "2R+1": 2 * R + 1, "R-1": R - 1}[height]
    assert Ho >= 1
    img, mx = pixels
    for kind in KINDS:
        my = row_maps(kind, Ho)
        ref = np.stack([oracle.remap_bilinear(img[b], mx[b], my[b], "hwc", mode) for b in range(B)])
        for stream in POLICIES:
            got = run(dev, img, mx, my, mode, stream)
            assert same_bits(got, ref), (kind, Ho, mode, stream)


@pytest.mark.parametrize("mode", ["exact", "cv2"])
def test_inf_and_nan_pixels(dev, oracle, shipped, pixels, mode):
    """+-inf and NaN pixels travel through every policy alike.  Against the oracle: the same bits wherever the oracle's value
    is a number or an infinity, and a NaN exactly where the oracle has one (the payload of a NaN that arithmetic produces is
    the processor's, not the oracle's: the CPU's default NaN carries the sign bit, the GPU's does not)."""
    img, mx = pixels
    img = img.copy()
    img[0, 3, 100:140, 0] = np.inf
    img[1, 4, 500:520, 1] = -np.inf
    img[2, 2, 1000:1024, 2] = np.nan
    img[0, 5, 0:8, :] = np.nan
    img[1, 5, 300:310, 2] = np.inf
    img[1, 6, 300:310, 2] = -np.inf            # inf - inf between two source rows
    Ho = 2 * shipped["rows"] + 1
    my = row_maps("near_identity", Ho)
    ref = np.stack([oracle.remap_bilinear(img[b], mx[b], my[b], "hwc", mode) for b in range(B)])
    assert np.isnan(ref).any() and np.isinf(ref).any()
    cached = run(dev, img, mx, my, mode, 0)
    num = ~np.isnan(ref)
    assert np.array_equal(np.isnan(cached), ~num)
    assert np.array_equal(cached.view(np.uint32)[num], ref.view(np.uint32)[num])
    for stream in POLICIES[1:]:
        assert same_bits(run(dev, img, mx, my, mode, stream), cached), (mode, stream)


def test_two_row_blocks_per_workgroup(dev, oracle, shipped):
    """The launcher itself chooses two row blocks per workgroup (one row list: the jump to the second block is a step of the row loop) once the launch has 4096 workgroups: images of height 4R, every image against the oracle.
    The launch exceeds the Infinity Cache, so the gate picks the streaming variant by itself; the cached form is forced."""
    from attwarp_amd import checkpoint_utils as cu
    R = shipped["rows"]
    if shipped["cpw"] < 2:
        pytest.fail("the shipped shape has one row block per workgroup: this case needs a new home")
    H = 4 * R
    nb = 4096 // ((4 + shipped["cpw"] - 1) // shipped["cpw"]) + 2
    plan = _lib.remap_plan(nb, C, H, W, H, W, "cv2")
    assert plan["cpw"] == 2 and plan["rows"] == R and plan["stream"] == shipped["stream"], plan
    gen = torch.Generator(device=dev).manual_seed(5)
    img = torch.rand((nb, H, W, C), device=dev, generator=gen)
    y = torch.arange(H, device=dev, dtype=torch.float32)
    x = torch.arange(W, device=dev, dtype=torch.float32)
    jit = torch.rand((nb, 1), device=dev, generator=gen)
    my = (y[None] * (0.8 + 0.4 * jit) + jit).clamp(0, H - 1).contiguous()
    mx = (x[None] * (0.9 + 0.2 * jit) + 3 * jit).clamp(0, W - 1).contiguous()
    out = cu.remap_separable(img, mx, my, mode="cv2", channels_last=True)
    with _lib.debug_override(remap_stream=0):
        assert _lib.remap_plan(nb, C, H, W, H, W, "cv2") == dict(plan, stream=0)
        cached = cu.remap_separable(img, mx, my, mode="cv2", channels_last=True)
    assert torch.equal(out.view(torch.int32), cached.view(torch.int32))
    img_h, mx_h, my_h, out_h = img.cpu().numpy(), mx.cpu().numpy(), my.cpu().numpy(), out.cpu().numpy()
    from concurrent.futures import ThreadPoolExecutor
    def check(b):
        return same_bits(out_h[b], oracle.remap_bilinear(img_h[b], mx_h[b], my_h[b], "hwc", "cv2"))
    with ThreadPoolExecutor(max_workers=8) as ex:
        ok = list(ex.map(check, range(nb)))
    assert all(ok), [b for b, v in enumerate(ok) if not v][:10]
