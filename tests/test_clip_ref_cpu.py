"""What tests/test_clip_sweep_gpu.py stands on, checked without a GPU: the Pillow-built reference (clip_ref) equals the numpy
restatement oracle.clip_preprocess bit for bit on every RGB case of the sweep, the ``blocks`` pattern really drives both
passes of the tap-edge cases out of [0, 255] (a condition on the inputs, not a measurement of the kernels), and the case
list reaches every path of the launcher it claims to, according to clip_ref.route."""
import numpy as np
import pytest

import clip_ref as R
from oracle import warp_oracle as O

RGB_CASES = sorted({(c.H, c.W, c.size) for c in R.ALL_CASES if c.C == 3})


def test_reference_constants_are_the_oracles():
    assert R.OPENAI_CLIP_MEAN == O.OPENAI_CLIP_MEAN and R.OPENAI_CLIP_STD == O.OPENAI_CLIP_STD


@pytest.mark.parametrize("hws", RGB_CASES, ids=lambda c: "%dx%d-%d" % c)
def test_reference_equals_oracle(hws):
    """Pillow itself against the numpy restatement of Pillow, every pattern, default mean / std."""
    H, W, size = hws
    for name in R.PATTERNS:
        img = R.pattern(name, H, W, 3, size, seed=5)
        assert np.array_equal(R.clip_preprocess(img, size), O.clip_preprocess(img, size)), (hws, name)


@pytest.mark.parametrize("hw", R.PAD_TO_SQUARE)
def test_reference_equals_oracle_padded(hw):
    H, W = hw
    for name in ("blocks", "noise"):
        sq = O.expand2square(R.pattern(name, H, W, 3, 32, seed=6))
        assert sq.shape == (61, 61, 3)
        assert np.array_equal(R.clip_preprocess(sq, 32), O.clip_preprocess(sq, 32))


def test_reference_channels_are_independent():
    """oracle.clip_preprocess is RGB only: for four channels every plane of the reference equals the oracle's mode-"L"
    resize of that channel, cropped, with that channel's constants."""
    H, W, size = 97, 131, 32
    img = R.pattern("noise", H, W, 4, size, seed=7)
    full = R.clip_preprocess(img, size, R.SWEEP_MEAN, R.SWEEP_STD)
    assert full.shape == (4, size, size) and full.dtype == np.float32
    nh, nw, top, left = R.geometry(H, W, size)
    for c in range(4):
        want = O.pil_resize_u8(img[:, :, c], nw, nh, "bicubic")                  # the oracle's mode-"L" resize
        crop = want[top:top + size, left:left + size, None]
        assert np.array_equal(full[c], R.normalize(crop, R.SWEEP_MEAN[c:c + 1], R.SWEEP_STD[c:c + 1])[0])


def _unclamped_pass(src, bounds, kk, cols):
    """Pillow's 8-bit pass along the last axis for the output positions ``cols``, WITHOUT the clamp: acc >> 22."""
    s = src.astype(np.int64)
    out = np.empty(src.shape[:-1] + (len(cols),), dtype=np.int64)
    for i, xx in enumerate(cols):
        xmin, cnt = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(src.shape[:-1], 1 << 21, dtype=np.int64)
        for x in range(cnt):
            acc += s[..., xmin + x] * int(kk[xx, x])
        out[..., i] = acc >> 22
    return out


@pytest.mark.parametrize("case", R.TAP_EDGES, ids=lambda c: "%dx%d" % (c.H, c.W))
def test_blocks_saturate_both_passes(case):
    """The clamps of clip8 are exercised only if accumulators leave [0, 255]: with the oracle's tables and no clamp, each
    pass of every tap-edge case has at least 100 accumulators below 0 and at least 100 above 255 (counted over what the
    kernels compute: all source rows x the cropped columns, then the cropped square; all channels)."""
    H, W, C, size = case.H, case.W, case.C, case.size
    img = R.pattern("blocks", H, W, C, size)
    nh, nw, top, left = R.geometry(H, W, size)
    bx, kx, _ = O.pil_resample_coeffs(W, nw, "bicubic")
    by, ky, _ = O.pil_resample_coeffs(H, nh, "bicubic")
    hacc = _unclamped_pass(img.transpose(0, 2, 1), bx, kx, range(left, left + size))         # [H, C, size]
    tmp = np.clip(hacc, 0, 255).astype(np.uint8)
    vacc = _unclamped_pass(tmp.transpose(1, 2, 0), by, ky, range(top, top + size))           # [C, size, size]
    for what, acc in (("horizontal", hacc), ("vertical", vacc)):
        lo, hi = int((acc < 0).sum()), int((acc > 255).sum())
        print(f"{case.H}x{case.W} {what}: {lo} below 0 (min {acc.min()}), {hi} above 255 (max {acc.max()})")
        assert lo >= 100 and hi >= 100, (case, what, lo, hi)


def test_tap_count_table():
    assert [R.taps(n, 32) for n in (48, 49, 112, 113)] == [7, 9, 15, 17]
    assert R.taps(20, 32) == 5 and R.taps(32, 32) == 5
    for case, (kx, ky) in zip(R.TAP_EDGES, R.TAP_EDGE_KSIZES):
        r = R.route(case.H, case.W, case.C, case.size)
        assert (r.ksize_x, r.ksize_y) == (kx, ky), (case, r)
        _, _, ox = O.pil_resample_coeffs(case.W, r.nw, "bicubic")
        _, _, oy = O.pil_resample_coeffs(case.H, r.nh, "bicubic")
        assert (ox, oy) == (kx, ky)


def test_route_coverage():
    """Every class of the launcher's conditions and of the staged kernels' fixed loops has a case."""
    rs = [(c, R.check_route(c)) for c in R.ALL_CASES]
    staged = [(c, r) for c, r in rs if r.route != "generic"]
    generic = [(c, r) for c, r in rs if r.route == "generic"]

    def some(pairs, pred):
        return any(pred(c, r) for c, r in pairs)

    assert {r.route for _, r in rs} == {"staged8", "staged16", "generic"}
    assert {c.C for c, _ in staged} == {1, 3, 4} and {c.C for c, _ in rs} == {1, 2, 3, 4}
    for C in (1, 3, 4):                                   # both horizontal variants for every channel count that has them
        assert some(staged, lambda c, r: c.C == C and r.route == "staged16"), C
    # the horizontal kernel's xx += NTH second pass, the vertical kernel's second dword, with C = 3 among them
    assert some(staged, lambda c, r: c.size > 384)
    assert some(staged, lambda c, r: c.C == 3 and r.oc // 4 > R.NT)
    assert some(staged, lambda c, r: c.C == 1 and c.size > 384)
    # the limits of oc from both sides
    assert some(staged, lambda c, r: r.oc == 4 * R.NT * R.NQ)
    assert some(staged, lambda c, r: r.oc == 4 * R.NT * R.NQ - 8)
    assert some(generic, lambda c, r: r.oc == 4 * R.NT * R.NQ + 1)
    assert some(generic, lambda c, r: r.oc % 4 != 0 and r.oc < 4 * R.NT * R.NQ and r.ksize_x <= 16 and r.RB >= 1)
    # rows per workgroup: 8, 7, 1, the largest row that fits, none; a last workgroup and a last staging round of < 8 rows
    assert {r.RB for _, r in staged} >= {1, 7, 8} and some(generic, lambda c, r: r.RB == 0 and r.ksize_x <= 16)
    assert some(staged, lambda c, r: r.RB == 1 and ((c.W * c.C + 3) & ~3) + ((r.oc + 3) & ~3) == R.LDS)
    assert some(staged, lambda c, r: c.H > r.RB and c.H % r.RB != 0 and c.W * c.C % 4 == 0)
    assert some(staged, lambda c, r: r.RB == 7 and c.W * c.C % 4 == 0)
    # tap counts: both sides of 8 | 9 and of 16 | 17, mixed counts on both routes, fewer than 8 (padded), identity axes
    assert {r.ksize_x for _, r in staged} >= {5, 7, 9, 13, 15} and {r.ksize_x for _, r in generic} >= {17}
    assert some(staged, lambda c, r: r.ksize_y > 16) and some(generic, lambda c, r: r.ksize_y <= 16 and r.ksize_x > 16)
    assert some(staged, lambda c, r: c.H == r.nh and r.left > 0) and some(staged, lambda c, r: c.W == r.nw and r.top > 0)
    assert some(staged, lambda c, r: c.H < c.size and c.W < c.size)
    # crops on both axes and routes; source rows that are and are not whole dwords
    assert some(staged, lambda c, r: r.left > 0) and some(staged, lambda c, r: r.top > 0)
    assert some(generic, lambda c, r: r.left > 0)
    assert some(staged, lambda c, r: c.W * c.C % 4 != 0) and some(staged, lambda c, r: c.W * c.C % 4 == 0)
    # out of scope (Pillow reorders its passes): much higher than wide AND shrinking vertically
    assert not any(c.H > 100 * c.W and r.nh < c.H for c, r in rs)
    for H, W in R.PAD_TO_SQUARE:
        assert R.route(max(H, W), max(H, W), 3, 32).route == R.PAD_ROUTE


def test_patterns():
    for name in R.PATTERNS:
        a, b = R.pattern(name, 9, 11, 3, 4, seed=1), R.pattern(name, 9, 11, 3, 4, seed=1)
        assert a.dtype == np.uint8 and a.shape == (9, 11, 3) and np.array_equal(a, b)
    assert set(np.unique(R.pattern("extremes", 40, 40, 3, 32))) == {0, 255}
    ramp = R.pattern("ramp", 8, 8, 4, 8)
    assert ramp[2, 3, 1] == (7 * 3 + 13 * 2 + 85) & 255 and len({ramp[0, 0, c] for c in range(4)}) == 4
    blocks = R.pattern("blocks", 112, 112, 3, 32)
    assert R.block_side(112, 112, 32) == 8 and blocks[0, 0, 0] == 0 and blocks[0, 8, 2] == 255 and blocks[8, 8, 1] == 0
    bt = R.batch(9, 11, 3, 4, ("noise", "noise"))
    assert not np.array_equal(bt[0], bt[1])
