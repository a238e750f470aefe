"""Pin-on-arrival of the Stable-Diffusion warp ablation's map arithmetic against OpenCV itself: cv2.resize(float32 map, (W, H),
INTER_CUBIC) and cv2.GaussianBlur(map, (5, 5), sigmaX=1.0), the calls of Stable_diffusion_based_warp.py:159, 396, 409-410.
OpenCV is not installed where this project is built, so tests/sdwarp_ref.py restates its published algorithms (the kernels
are bit-exact against that).  This file skips without ``cv2``; with it, it reports the largest difference in float32 ulp of
each map's largest magnitude and asserts <= 4 ulp (OpenCV's vectorised passes may sum the taps in another order, with FMA
where the build has it), and the exact tables.  CPU only."""
import numpy as np
import pytest

import sdwarp_ref as R

cv2 = pytest.importorskip("cv2", reason="OpenCV is not installed: cubic resize and blur stay pinned to the published algorithm only")

CASES = [((12, 12), (500, 375)), ((24, 24), (1024, 768)), ((96, 96), (683, 1024)), ((200, 300), (64, 48)),
         ((375, 500), (500, 500)), ((3, 5), (257, 2)), ((1, 1), (7, 9)), ((768, 1024), (500, 500))]


def _ulps(got, want):
    ulp = np.spacing(np.float32(max(np.abs(want).max(), np.finfo(np.float32).tiny)))
    return float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / ulp)


def test_cubic_resize_within_a_few_ulp_of_opencv():
    rng = np.random.default_rng(3)
    worst = 0.0
    for (h, w), (W, H) in CASES:
        a = rng.random((h, w), dtype=np.float32)
        d = _ulps(cv2.resize(a, (W, H), interpolation=cv2.INTER_CUBIC), R.resize_cubic(a, W, H))
        worst = max(worst, d)
        assert d <= 4, ((h, w), (W, H), d)
    print(f"\n[test_sdwarp_vs_opencv] OpenCV {cv2.__version__}: INTER_CUBIC largest difference {worst:.2f} ulp of the map's maximum")


def test_gaussian_kernel_and_blur_within_a_few_ulp_of_opencv():
    k = cv2.getGaussianKernel(5, 1.0, cv2.CV_32F).ravel()
    assert k.tobytes() == R.gaussian5_taps(1.0).tobytes()
    rng = np.random.default_rng(4)
    worst = 0.0
    for (H, W) in [(1, 1), (1, 7), (2, 2), (3, 5), (375, 500), (257, 513)]:
        a = rng.random((H, W), dtype=np.float32)
        d = _ulps(cv2.GaussianBlur(a, ksize=(5, 5), sigmaX=1.0), R.blur5(a))
        worst = max(worst, d)
        assert d <= 4, ((H, W), d)
    print(f"\n[test_sdwarp_vs_opencv] OpenCV {cv2.__version__}: GaussianBlur largest difference {worst:.2f} ulp of the map's maximum")
