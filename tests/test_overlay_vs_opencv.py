"""Pin-on-arrival of the heat-map overlay's OpenCV steps (cv2.normalize NORM_MINMAX, cv2.applyColorMap COLORMAP_JET,
cv2.addWeighted), the same scheme as test_oracle_vs_opencv.py: OpenCV is not installed where this project is built, so
tests/overlay_ref.py restates OpenCV's published algorithms and the HIP kernels are bit-exact against that restatement.
This file skips without ``cv2``; with it, it compares the restatement with the real functions -- the Jet table and the
index tables of every (min, max) pair exactly, random overlays exactly at alpha = 0.5 and within 1 elsewhere (OpenCV's
scalar tail and other builds may evaluate addWeighted in another order).  CPU only."""
import numpy as np
import pytest

import overlay_ref as R

cv2 = pytest.importorskip("cv2", reason="OpenCV is not installed: the overlay stays pinned to the published algorithm only")


@pytest.fixture(scope="module", autouse=True)
def announce():
    print("\n[test_overlay_vs_opencv] comparing the restatement against OpenCV", cv2.__version__)


def test_jet_table_equals_opencv():
    got = cv2.applyColorMap(np.arange(256, dtype=np.uint8).reshape(16, 16), cv2.COLORMAP_JET).reshape(256, 3)
    assert np.array_equal(got, R.jet_table())
    assert np.array_equal(got, R.committed_jet_table())


def test_normalize_tables_equal_opencv_for_every_min_max_pair():
    v = np.arange(256, dtype=np.float32)
    for lo in range(256):
        for hi in range(lo, 256):
            m = np.clip(v, lo, hi).reshape(16, 16)              # a mask holding exactly the values lo .. hi
            got = cv2.normalize(m, None, 0, 255, cv2.NORM_MINMAX).astype(np.uint8).ravel()
            assert np.array_equal(got[lo:hi + 1], R.normalize_table(lo, hi)[lo:hi + 1]), (lo, hi)


@pytest.mark.parametrize("alpha", [0.5, 0.3, 1.0, 0.77])
def test_random_overlays_against_opencv(alpha):
    rng = np.random.default_rng(int(alpha * 100))
    for h, w in [(37, 53), (64, 683), (200, 301)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        m = rng.integers(0, 256, (h, w), dtype=np.uint8)
        m = np.clip(m, *sorted(rng.integers(0, 256, 2))).astype(np.uint8)
        # blend_mask (llava.py:254-269)
        norm = cv2.normalize(m.astype(np.float32), None, 0, 255, cv2.NORM_MINMAX).astype(np.uint8)
        heat = cv2.applyColorMap(norm, cv2.COLORMAP_JET)
        want = cv2.cvtColor(cv2.addWeighted(cv2.cvtColor(img, cv2.COLOR_RGB2BGR), 1 - alpha, heat, alpha, 0), cv2.COLOR_BGR2RGB)
        got = R.blend_mask_overlay(img, m, alpha)
        # save_warped_image (new_method.py:455-475)
        f = (rng.random((h, w)) ** 2).astype(np.float32)
        heat2 = cv2.applyColorMap(R.save_warped_indices(f), cv2.COLORMAP_JET)
        want2 = cv2.addWeighted(heat2, alpha, img, 1 - alpha, 0)
        got2 = R.save_warped_overlay(img, f, alpha)
        for g, w_ in ((got, want), (got2, want2)):
            d = np.abs(g.astype(int) - w_.astype(int))
            assert d.max() <= (0 if alpha == 0.5 else 1), (alpha, h, w, int(d.max()))
