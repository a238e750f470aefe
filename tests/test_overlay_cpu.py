"""CPU checks of the Jet heat-map overlay (attwarp_heatmap_overlay): the committed COLORMAP_JET table against an independent
recomputation of OpenCV's steps, the index tables of degenerate maps, blend_mask's alpha selection, and the C ABI's
argument validation (no GPU here: every call must fail in validation, before anything is enqueued)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import overlay_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from attwarp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_committed_jet_table_equals_the_restatement():
    t = R.committed_jet_table()
    assert np.array_equal(t, R.jet_table())
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_jet_table
    finally:
        sys.path.pop(0)
    assert np.array_equal(t, gen_jet_table.jet_table())          # the generator of the committed header
    # anchors (B, G, R)
    assert tuple(t[0]) == (128, 0, 0) and tuple(t[127]) == (130, 255, 126)
    assert tuple(t[128]) == (126, 255, 130) and tuple(t[255]) == (0, 0, 128)


def test_jet_table_depends_on_the_float32_steps():
    """320 of the 768 products are .5 ties in real arithmetic: rounding the exact Octave values instead of the float32
    steps gives another table, and so does skipping interp1 (one entry)."""
    x = np.arange(256) / 255.0
    t = R.jet_table().astype(np.int64)
    r = np.select([(x >= 3 / 8) & (x < 5 / 8), (x >= 5 / 8) & (x < 7 / 8), x >= 7 / 8], [4 * x - 1.5, 1.0, -4 * x + 4.5], 0.0)
    g = np.select([(x >= 1 / 8) & (x < 3 / 8), (x >= 3 / 8) & (x < 5 / 8), (x >= 5 / 8) & (x < 7 / 8)], [4 * x - 0.5, 1.0, -4 * x + 3.5], 0.0)
    b = np.select([x < 1 / 8, (x >= 1 / 8) & (x < 3 / 8), (x >= 3 / 8) & (x < 5 / 8)], [4 * x + 0.5, 1.0, -4 * x + 2.5], 0.0)
    exact = np.stack([b, g, r], axis=1) * 255
    frac = exact - np.floor(exact)
    assert int(np.isclose(frac, 0.5, atol=1e-9).sum()) == 320
    no_interp = np.clip(np.rint(np.stack([b, g, r], 1).astype(np.float32) * np.float32(255)), 0, 255)
    assert int((no_interp != t).any(axis=1).sum()) == 1
    assert np.abs(t - exact).max() <= 0.5 + 1e-6


def test_normalize_tables_of_degenerate_masks():
    # max == min (the constant 1/576 attention map of the drivers' OOM fallback): scale 0 -> every index 0
    for v in (0, 7, 255):
        assert not R.normalize_table(v, v)[v]
        m = np.full((5, 7), v, np.uint8)
        assert not R.blend_mask_indices(m).any()
    # one bright pixel on a dark mask
    m = np.zeros((9, 11), np.uint8); m[4, 5] = 200
    idx = R.blend_mask_indices(m)
    assert idx[4, 5] == 255 and (np.delete(idx.ravel(), 4 * 11 + 5) == 0).all()
    # the minimum always lands on 0; the maximum lands on 254 or 255 depending on (min, max): the float32 fma can fall
    # just below 255
    top = {}
    for lo in range(256):
        for hi in range(lo + 1, 256):
            t = R.normalize_table(lo, hi)
            assert t[lo] == 0 and t[hi] in (254, 255)
            assert (np.diff(t[lo:hi + 1].astype(int)) >= 0).all()
            top[(lo, hi)] = int(t[hi])
    assert 254 in top.values() and 255 in top.values()


def test_save_warped_indices_of_degenerate_maps():
    # uint8: equal values -> zeros; the range divided in float64
    assert not R.save_warped_indices(np.full((4, 4), 9, np.uint8)).any()
    m = np.array([[3, 4], [5, 10]], np.uint8)
    assert np.array_equal(R.save_warped_indices(m), np.array([[0, 36], [72, 255]], np.uint8))
    # float maps: a NaN anywhere fails `max > min + EPSILON` -> zeros; an infinite range -> 0 / NaN products -> zeros
    f = np.linspace(0, 1, 20, dtype=np.float32).reshape(4, 5)
    for bad in (np.nan, np.inf, -np.inf):
        g = f.copy(); g[1, 2] = bad
        assert not R.save_warped_indices(g).any(), bad
        assert not R.save_warped_indices(g.astype(np.float64)).any(), bad
    # a float32 range below EPSILON (the test runs in float32 under NEP 50) -> zeros; float64 the same
    assert not R.save_warped_indices(np.array([[0.5, 0.5 + 2 ** -24]], np.float32) * np.float32(1e-3)).any()
    assert not R.save_warped_indices(np.array([[1.0, 1.0 + 5e-10]])).any()
    assert R.save_warped_indices(f)[-1, -1] == 255 and R.save_warped_indices(f)[0, 0] == 0


def test_add_weighted_restatement_at_half_is_order_free():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, 4096, dtype=np.uint8); b = rng.integers(0, 256, 4096, dtype=np.uint8)
    want = np.clip(np.rint(a.astype(np.float64) * 0.5 + b.astype(np.float64) * 0.5), 0, 255)
    assert np.array_equal(R.add_weighted_u8(a, 0.5, b, 0.5), want)
    assert np.array_equal(R.add_weighted_u8(b, 0.5, a, 0.5), want)
    # other weights: within 1 of the real-number result
    y = R.add_weighted_u8(a, 0.7, b, 0.3).astype(np.float64)
    assert np.abs(y - (a * 0.7 + b * 0.3)).max() <= 0.5 + 1e-6


def test_blend_mask_alpha_selection():
    from attwarp_amd import attention_extraction as ae
    cases = [0, 0.0, -1, 0.3, 1, 1.0, 1.5, None, "0.3", True, False, np.float64(0.3), np.float32(0.3), np.int64(1)]
    for g in cases:
        assert ae.blend_alpha(g) == R.blend_alpha(g), g
    assert ae.blend_alpha(0) == 0.5 and ae.blend_alpha(0.3) == 0.3 and ae.blend_alpha(1) == 1
    assert ae.blend_alpha(np.float32(0.3)) == 0.5            # not a Python float: the reference falls back to 0.5


def _records(n, H=40, W=683, base=0x200000):
    recs = (ctypes.c_uint8 * (32 * n))()
    arr = np.frombuffer(recs, dtype=np.dtype([("image", "<u8"), ("map", "<u8"), ("out", "<u8"), ("H", "<i4"), ("W", "<i4")]))
    for i in range(n):
        arr[i] = (base + 0x100000 * i + 1, base + 0x100000 * i + 0x80000, base + 0x100000 * i + 0xC0001, H, W)
    return recs, arr


def test_overlay_abi_validation_without_gpu(lib):
    from attwarp_amd import _lib
    assert ctypes.sizeof(ctypes.c_void_p) == 8
    assert lib.attwarp_overlay_workspace_bytes(1) == 256 * 16 and lib.attwarp_overlay_workspace_bytes(32) == 32 * 256 * 16
    assert lib.attwarp_overlay_workspace_bytes(0) == 0 and lib.attwarp_overlay_workspace_bytes(-3) == 0
    recs, arr = _records(3)
    P = ctypes.c_void_p
    ok = dict(images=ctypes.addressof(recs), images_dev=P(0x900000), B=3, map_dtype=_lib.U8, style=_lib.OVERLAY_BLEND_MASK,
              alpha=0.5, in_order=_lib.RGB, out_order=_lib.RGB, ws=P(0xA00000), stream=None)
    names = list(ok)
    def call(**kw):
        a = dict(ok, **kw)
        return lib.attwarp_heatmap_overlay(*[a[k] for k in names])
    def err():
        return lib.attwarp_last_error()
    assert call(images=None) == -1 and b"null pointer" in err()
    assert call(images_dev=None) == -1 and call(ws=None) == -1
    assert call(B=0) == -1 and b"batch size" in err()
    assert call(B=70000) == -2
    assert call(map_dtype=_lib.F16) == -1 and b"map_dtype" in err()
    assert call(style=2) == -1 and b"style" in err()
    assert call(style=_lib.OVERLAY_BLEND_MASK, map_dtype=_lib.F32) == -1 and b"uint8" in err()
    assert call(in_order=2) == -1 and call(out_order=-1) == -1 and b"channel orders" in err()
    assert call(alpha=float("nan")) == -1 and call(alpha=float("inf")) == -1 and b"alpha" in err()
    assert call(ws=P(0xA00008)) == -1 and call(images_dev=P(0x900004)) == -1 and b"aligned" in err()
    # per-image records
    for field, val, msg in (("image", 0, b"image 1: null"), ("map", 0, b"image 1: null"), ("out", 0, b"image 1: null"),
                            ("H", 0, b"image 1: non-positive"), ("W", -5, b"image 1: non-positive")):
        saved = arr[1][field]
        arr[1][field] = val
        assert call() == -1 and msg in err(), field
        arr[1][field] = saved
    # float maps must be element aligned (uint8 maps, images and outputs may sit at any byte address)
    arr[2]["map"] += 2
    assert call(map_dtype=_lib.F32, style=_lib.OVERLAY_SAVE_WARPED) == -1 and b"image 2: map not 4-byte aligned" in err()
    arr[2]["map"] += 4
    assert call(map_dtype=_lib.F64, style=_lib.OVERLAY_SAVE_WARPED) == -1 and b"image 2: map not 8-byte aligned" in err()
    arr[2]["map"] -= 6
    arr[0]["H"], arr[0]["W"] = 40000, 40000
    assert call() == -2 and b"image 0" in err()


def test_overlay_has_no_cpu_fallback():
    import torch
    from attwarp_amd import pipeline
    img = torch.zeros(2, 8, 9, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pipeline.heatmap_overlay(img, torch.zeros(2, 8, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="style"):
        pipeline.heatmap_overlay(img, torch.zeros(2, 8, 9, dtype=torch.uint8), style="other")
