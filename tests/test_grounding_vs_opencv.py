"""Pin-on-arrival of the layer sweep's resize against OpenCV itself: cv2.resize(float32 grid, (W, H), INTER_LANCZOS4), the
call of uncertainty_attn_maps_llava.py:63-64.  OpenCV is not installed where this project is built, so tests/grounding_ref.py
restates resizeGeneric_ (the kernels are bit-exact against it).  This file skips without ``cv2``; with it, it reports the
largest difference in float32 ulp and asserts <= 4 ulp of each map's largest magnitude (OpenCV's vectorised vertical pass
sums the taps in another order, with FMA where the build has it), and equal top1 except at near ties.  CPU only."""
import numpy as np
import pytest

import grounding_ref as R

cv2 = pytest.importorskip("cv2", reason="OpenCV is not installed: the resize stays pinned to the published algorithm only")

SIZES = [(1024, 768), (683, 1024), (1024, 1024), (500, 375), (333, 500), (640, 427), (18, 27), (24, 24), (7, 333), (25, 23)]


def _grids(n, seed=3):
    rng = np.random.default_rng(seed)
    a = rng.random((n, 24, 24), dtype=np.float32) ** 4
    return (a / a.sum(axis=(1, 2), keepdims=True)).astype(np.float32)


def test_lanczos4_resize_within_a_few_ulp_of_opencv():
    worst = 0.0
    for i, (W, H) in enumerate(SIZES):
        g = _grids(len(SIZES))[i]
        got = cv2.resize(g, (W, H), interpolation=cv2.INTER_LANCZOS4)
        want = R.resize_lanczos4(g, W, H)
        ulp = np.spacing(np.float32(np.abs(want).max()))
        d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / ulp)
        worst = max(worst, d)
        assert d <= 4, (W, H, d)
    print(f"\n[test_grounding_vs_opencv] OpenCV {cv2.__version__}: largest difference {worst:.2f} ulp of the map's maximum")


def test_top1_equal_except_near_ties():
    rng = np.random.default_rng(8)
    g = _grids(40, seed=9)
    flips = 0
    for i in range(40):
        W, H = SIZES[i % 6]
        box = (int(rng.integers(0, W // 2)), int(rng.integers(0, H // 2)), int(rng.integers(1, W // 2)), int(rng.integers(1, H // 2)))
        got = cv2.resize(g[i], (W, H), interpolation=cv2.INTER_LANCZOS4)
        want = R.resize_lanczos4(g[i], W, H)
        a, b = R.box_metrics(got, box), R.box_metrics(want, box)
        if a[1] != b[1]:
            # a flip is only allowed when the two maxima are within a few ulp of each other in both maps
            ulp = np.spacing(np.float32(np.abs(want).max()))
            assert abs(float(want.flat[a[0]]) - float(want.flat[b[0]])) <= 8 * ulp
            flips += 1
    assert flips <= 2
