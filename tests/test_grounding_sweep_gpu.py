"""Size-limit sweep of the layer-selection kernels (csrc/grounding.hip: resize_kernel, metrics_kernel<fused / dense>,
metrics_final_kernel; attn_probe_kernel + head_mean_kernel of csrc/probe.hip) against tests/grounding_ref.py, the numpy
restatement.  The expected values are computed at run time from the float32 inputs copied back from the device.

What is compared, and how:
* resize: every output bit (NaN positions where the grid holds non-finite values, the bits everywhere else);
* box metrics, every map of every case, dense and fused: ``argmax`` and ``top1`` exactly against ``R.box_metrics`` of the
  reference map; ``fused`` and ``dense`` bit for bit in all three outputs; ``am`` within the bound below;
* head-mean probe: every output bit in float32, float16 and bfloat16.

The ``am`` bound is derived, not tuned.  The test's reference sums are ``math.fsum`` over the float64 reference map
(exact, so the reference adds no error).  The kernel adds n float64 terms in a fixed order, so each of its two sums is off
by at most n * 2^-53 * sum(|v|); the largest map here has n = 32768 x 257 = 8.42 M pixels and n * 2^-53 = 9.4e-10 < 1e-9.
For am = box / (total + 1e-12) that gives |am - ref| <= (|d box| + |ref| |d total|) / |total + 1e-12|
<= 2e-9 * max(1, |ref|) * sum(|v|) / |sum(v) + 1e-12|, which is what is asserted.  So that this stays a bound of 4e-9
relative and not a licence, every finite case first asserts sum(|v|) <= 2 |sum(v)| on its reference map (LANCZOS4 has
negative lobes; the grids_of recipe gives 1.05 - 1.28).  Non-finite totals: both sides NaN, or equal.

The cases are the structural edges of the kernels: grids of 1, 2, 63 and 64 rows or columns (64 x 256 floats is the whole
default LDS grant of a launch, plus 80 bytes of static LDS in the metrics kernel), output sides of 1, 2 and one less than,
equal to and one more than a 256-column tile and a 256-row band, down-sampling (the vertical window reloads every row),
128 x 2 and 2 x 128 partials per map, 65535 maps per call (256 blocks of the combining kernel), a ragged call whose grid.x
is empty for most maps, boxes by numpy's slice rules, and every (lanes per row, chunks per lane) instantiation of the probe
at kv up to 15872 and ntok up to 1024.  Refusals are host-side only.
"""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import grounding_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
BIG = (1 << 40) - 1

# ---- the cases (plain data and CPU-only builders: importable without a GPU) --------------------------------------------
GRIDS = [(1, 1), (1, 64), (64, 1), (2, 2), (7, 8), (23, 24), (63, 64), (64, 63), (64, 64)]          # (h, w)
SIDES = (1, 2, 255, 256, 257, 513)
GIANTS = [(32768, 3), (3, 32768), (32768, 257), (257, 32768)]                                      # (W, H) at 64 x 64
HOSTILE_SIZES = [(257, 513), (2, 255), (513, 1), (256, 256), (5, 3)]
# nc = 16-byte chunks of a key row = head_dim / (16 / esize) -> (lanes per row, chunks per lane) of launch_t; then
# heads / kv_heads, kv_heads, ntok, kv.  head_dim = 4 nc in float32 (4 ... 256), 8 nc in float16 / bfloat16 (8 ... 512).
PROBE_CASES = [
    (16, 4, 1, 576, 15872),     # (16, 1)  the study's shape at MAX_KV
    (32, 1, 2, 576, 577),       # (16, 2)
    (48, 8, 1, 1024, 1024),     # (16, 3)  kv == ntok
    (64, 4, 2, 1024, 1025),     # (16, 4)
    (8, 8, 1, 1024, 15872),     # (8, 1)   start + ntok == kv at both limits
    (24, 1, 3, 576, 576),       # (8, 3)
    (4, 4, 2, 1, 2),            # (4, 1)
    (12, 8, 1, 1, 1),           # (4, 3)   one key
    (2, 1, 4, 576, 15872),      # (2, 1)
    (6, 4, 1, 1024, 1025),      # (2, 3)
    (1, 8, 1, 1, 15872),        # (1, 1)
    (3, 1, 2, 576, 577),        # (1, 3)
]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def grids_of(rng, M, h, w):
    a = rng.random((M, h, w), dtype=F32) ** 4
    return (a / a.sum(axis=(1, 2), keepdims=True)).astype(F32)


def case_grids(rng, sizes, h, w):
    """One grid per (W, H).  Up-sampled maps take the peaked grids_of recipe.  A down-sampled axis keeps 8 of its taps and
    skips the rest, so on a peaked grid the negative lobes can cancel most of a map's total (sum|v| / |sum v| reached 6.5 at
    1 x 64 -> 2 x 1) and ``am`` would be ill-conditioned; those sizes take grids with a floor, (1 + rand) normalised, which
    keep the map positive."""
    g = grids_of(rng, len(sizes), h, w)
    flat = 1 + rng.random((len(sizes), h, w), dtype=F32)
    flat = (flat / flat.sum(axis=(1, 2), keepdims=True)).astype(F32)
    down = np.array([W < w or H < h for (W, H) in sizes])
    g[down] = flat[down]
    return g


def sizes_of(h, w):
    """(W, H) of one grid shape: every pair of SIDES (up- and down-sampling in one and both axes), dsize == ssize, and
    one axis kept."""
    s = [(W, H) for W in SIDES for H in SIDES] + [(w, h), (w, 257), (255, h)]
    return list(dict.fromkeys(s))


def box_family(W, H):
    """(x, y, w, h) boxes as interpret_bbox gives them, for a [H,W] map."""
    b = [(W // 4, H // 4, max(1, W // 2), max(1, H // 2)),                  # interior
         (0, 0, W, H),                                                      # the whole map
         (W // 3, H // 3, 0, 0), (0, 0, 0, H), (0, 0, W, 0),                # empty
         (W // 2, H // 2, -3, 4), (W // 2, H // 2, 4, -3), (W, H, -W, -H),  # negative w / h
         (-3, -2, 2, 1), (-3, -2, 3, 2), (-3, -2, W + 5, H + 5), (-W, -H, W, H), (-W - 1, -H - 1, W, H),   # negative start
         (W, H, 3, 3), (W + 5, 0, 3, H), (0, H + 5, W, 3),                  # start past the end
         (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1),                           # corner pixels
         (0, 0, BIG, BIG), (-BIG, -BIG, BIG, BIG), (BIG, BIG, BIG, BIG), (-BIG, 0, BIG, -BIG)]             # +-(2^40 - 1)
    for e in (255, 256, 257):                                               # ending / starting at a tile and band edge
        b += [(0, 0, e, e), (e, e, W, H), (e - 1, e - 1, 2, 2)]
    return b


@functools.lru_cache(maxsize=None)
def ref_tables(n_in, n_out):
    return R.lanczos4_coeffs(n_in, n_out)


def ref_resize(g, W, H):
    h, w = g.shape[-2:]
    return R.resize_lanczos4(g, W, H, (ref_tables(w, W), ref_tables(h, H)))


def fsum(a):
    """math.fsum of an array, a chunk at a time (exact: one fsum over all elements)."""
    flat = np.ascontiguousarray(a, dtype=F64).ravel()
    return math.fsum(itertools.chain.from_iterable(flat[i:i + (1 << 20)].tolist() for i in range(0, flat.size, 1 << 20)))


class RefMap:
    """A reference map [H,W] float32 with its exact sums."""

    def __init__(self, att, what):
        self.att, self.what = np.ascontiguousarray(att, dtype=F32), what
        self.a64 = self.att.astype(F64)
        self.finite = bool(np.isfinite(self.att).all())
        if self.finite:
            self.tot, self.sabs = fsum(self.a64), fsum(np.abs(self.a64))
            assert self.sabs <= 2 * abs(self.tot), (what, "a badly chosen input: sum|v| / |sum v| > 2", self.sabs, self.tot)

    def metrics(self, box):
        """(argmax, top1, am reference, am bound or None)"""
        arg, top1, am_np = R.box_metrics(self.att, box)
        if not self.finite:
            return arg, top1, am_np, None
        x0, y0, w, h = box
        ref = fsum(self.a64[y0:y0 + h, x0:x0 + w]) / (self.tot + 1e-12)
        return arg, top1, ref, 2e-9 * max(1.0, abs(ref)) * self.sabs / abs(self.tot + 1e-12)


def check_metrics(refs, boxes, dense, fused, what):
    """refs[i]: the RefMap of map i.  dense / fused: BoxMetrics (either may be None)."""
    worst = 0.0
    res = [r for r in (dense, fused) if r is not None]
    got = [(r.argmax.cpu().numpy(), r.top1.cpu().numpy(), r.am.cpu().numpy()) for r in res]
    if len(got) == 2:
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), what
        assert np.array_equal(got[0][2].view(np.uint64), got[1][2].view(np.uint64)), what
    arg, top1, am = got[0]
    for i, (ref, box) in enumerate(zip(refs, boxes)):
        a, t, want, bound = ref.metrics(box)
        assert int(arg[i]) == a and int(top1[i]) == t, (what, ref.what, box, int(arg[i]), a, int(top1[i]), t)
        g = float(am[i])
        if bound is None:                                        # non-finite totals: NaN on both sides, or equal
            assert (np.isnan(g) and np.isnan(want)) or g == want, (what, ref.what, box, g, want)
        else:
            assert abs(g - want) <= bound, (what, ref.what, box, g, want, bound)
            worst = max(worst, abs(g - want) / bound if bound else 0.0)
    print(f"{what}: {len(boxes)} maps, worst am error {worst:.2e} of its bound")


def hostile_grids(h, w):
    """Grids with NaN, +-inf, -0.0 and denormals; the last two are finite (signed zeros and denormals only)."""
    rng = np.random.default_rng(70_000 + 64 * h + w)
    g = case_grids(rng, [(1, 1)] * 6, max(h, 2), w)[:, :h]       # the floored recipe: a down-sampled map may miss the planted pixel
    g[0, h // 2, w // 3] = np.nan
    g[1, 0, 0], g[1, h - 1, w - 1] = np.inf, -np.inf
    g[2, h // 3, w // 2], g[2, h - 1, 0], g[2, 0, w - 1] = np.inf, np.nan, F32(-0.0)
    g[3] = -g[3]
    g[3, 1 % h, 1 % w] = -np.inf
    g[4] = ((1 + rng.random((h, w), dtype=F32)) * F32(0.5e-38)).astype(F32)   # denormals and the smallest normals
    g[4, 0, 0] = g[4, h - 1, w // 2] = F32(-0.0)
    g[5] = np.where(rng.random((h, w)) < 0.5, F32(1e-45), F32(-0.0)).astype(F32)
    g[5, 0, 0] = F32(1e-45)
    return g


def planted_maps():
    """name -> dense [H,W] map with a planted extremum (3 x 3 blocks of 513 x 513; 3 x 2 of 600 wide, 257 high)."""
    rng = np.random.default_rng(80_000)
    out = {}

    def base(H=513, W=513):
        return grids_of(rng, 1, H, W)[0]

    for name, (r, c) in (("first pixel", (0, 0)), ("last pixel", (512, 512)), ("255,255", (255, 255)), ("255,256", (255, 256)),
                         ("256,255", (256, 255))):
        m = base()
        m[r, c] = 0.5
        out[name] = m
    m = base()
    m[300, 10] = m[10, 300] = m[10, 301] = m[256, 0] = m[255, 512] = 0.25     # ties: (10, 300) is the first in row-major order
    out["equal maxima in different tiles and bands"] = m
    m = base(257, 600)
    m[256, 0] = m[255, 599] = m[255, 256] = 0.25
    out["equal maxima across the band edge, 600 wide"] = m
    m = base()
    m[0, 0], m[400, 400] = 3.0e38, np.nan
    out["a NaN in a later block, a larger finite value earlier"] = m
    m = base()
    m[300, 300] = m[10, 500] = np.nan
    out["two NaNs in different blocks"] = m
    m = base(257, 600)
    m[256, 599] = m[256, 598] = np.nan
    out["two NaNs in the last block"] = m
    out["all -inf"] = np.full((513, 513), -np.inf, F32)
    out["all zero"] = np.zeros((513, 513), F32)
    m = np.full((257, 600), F32(-0.0))
    m[200, 300] = F32(0.0)                                       # -0.0 == 0.0: the first pixel stays the argmax
    out["signed zeros"] = m
    return out


def probe_case(nc, group, hkv, ntok, kv, esize):
    """float32 (q [B,H,D], k [B,Hkv,kv,D], starts, kv_begin): three samples -- no padding and the span at 0; padding that
    ends inside the span, the span at kv - ntok; one attended key (kv_begin = kv - 1), the span at kv - ntok."""
    D = nc * (16 // esize)
    rng = np.random.default_rng(90_000 + 131 * nc + 7 * ntok + kv + esize)
    B, H = 3, group * hkv
    q = rng.standard_normal((B, H, D)).astype(F32)
    k = rng.standard_normal((B, hkv, kv, D)).astype(F32)
    k[0, :, kv // 3:kv // 3 + 40] *= 3                          # a peaked region
    last = kv - ntok
    starts = [0, last, last]
    kv_begin = [0, min(last + ntok // 2, kv - 1), kv - 1]
    return q, k, starts, kv_begin, D


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import os
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from attwarp_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "HIP library missing -- the product has no fallback"
    _lib.load()
    return torch.device("cuda:0")


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def assert_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).sum()))


def assert_bits_or_nan(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions", int((gn != wn).sum()))
    assert np.array_equal(bits(got)[~wn], bits(want)[~wn]), (what, int((bits(got)[~wn] != bits(want)[~wn]).sum()))


def sweep(dev, grids, sizes, boxes_of, what, exact=assert_bits):
    """grids [n,h,w] float32 and one (W, H) per grid: the resize against the restatement, then every box of boxes_of(W, H)
    on every map through the dense kernel (on the resized maps) and the fused one (from the grids)."""
    from attwarp_amd import grounding as G
    tg = T(grids, dev)
    g = N(tg)                                                    # both sides see the float32 values the device holds
    views = G.resize_lanczos4(tg, sizes)
    refs, idx, boxes = [], [], []
    for i, (W, H) in enumerate(sizes):
        want = ref_resize(g[i], W, H)
        exact(N(views[i]), want, f"{what} -> W{W} H{H}")
        if (H, W) == g[i].shape:
            assert_bits_or_nan(N(views[i]), g[i], f"{what} copy")
        ref = RefMap(want, f"{what} -> W{W} H{H}")
        for box in boxes_of(W, H):
            refs.append(ref), idx.append(i), boxes.append(box)
    msizes = [sizes[i] for i in idx]
    fused = G.grid_box_metrics(tg[torch.tensor(idx, device=dev)], msizes, boxes)
    dense = G.box_metrics([views[i] for i in idx], boxes)
    check_metrics(refs, boxes, dense, fused, what)


# ---- resize and metrics over the grid and output shapes -------------------------------------------------------------------
@pytest.mark.parametrize("h,w", GRIDS)
def test_resize_and_metrics(dev, h, w):
    sizes = sizes_of(h, w)
    grids = case_grids(np.random.default_rng(1000 * h + w), sizes, h, w)
    sweep(dev, grids, sizes, box_family, f"grid {h}x{w}")


def test_giants_in_one_ragged_call(dev):
    """The largest maps next to the smallest in one call: grid.x is the 256 blocks of 32768 x 257, and the 1 x 1 maps use one."""
    sizes = [(1, 1), GIANTS[0], (2, 2), GIANTS[1], (1, 1), GIANTS[2], (64, 64), GIANTS[3]]
    grids = case_grids(np.random.default_rng(2), sizes, 64, 64)

    def boxes_of(W, H):
        return [(W // 4, H // 4, W // 2 + 1, H // 2 + 1), (0, 0, W, H), (-3, -2, 2, 1), (W - 1, H - 1, 1, 1), (255, 0, 2, H),
                (0, 255, W, 2), (-BIG, -BIG, BIG, BIG), (256, 256, BIG, BIG)]
    sweep(dev, grids, sizes, boxes_of, "ragged giants 64x64")


def test_largest_batch(dev):
    """65535 maps in a call: grid.y at its limit, 256 blocks of the combining kernel; 2 x 2 grids to 1 x 1 and 3 x 2."""
    from attwarp_amd import grounding as G
    M = 65535
    sizes = [(1, 1) if i % 2 == 0 else (3, 2) for i in range(M)]
    grids = case_grids(np.random.default_rng(3), [(1, 1)] * M, 2, 2)
    tg = T(grids, dev)
    g = N(tg)
    views = G.resize_lanczos4(tg, sizes)
    want = {(1, 1): ref_resize(g[0::2], 1, 1), (3, 2): ref_resize(g[1::2], 3, 2)}
    ref_maps = [want[sizes[i]][i // 2] for i in range(M)]
    assert [tuple(v.shape) for v in views[:2]] == [(1, 1), (2, 3)]
    whole = torch.cat([v.reshape(-1) for v in views]).cpu().numpy()          # every map, in order
    assert_bits(whole, np.concatenate([m.ravel() for m in ref_maps]), "largest batch, every map")
    family = [(0, 0, 1, 1), (0, 0, 3, 2), (1, 0, 2, 2), (-1, -1, 1, 1), (0, 0, 0, 0), (2, 1, 5, 5), (-BIG, 0, BIG, 1), (0, 0, BIG, BIG)]
    boxes = [family[i % len(family)] for i in range(M)]
    fused = G.grid_box_metrics(tg, sizes, boxes)
    dense = G.box_metrics(list(views), boxes)
    refs = [RefMap(m, f"largest batch map {i}") for i, m in enumerate(ref_maps)]
    check_metrics(refs, boxes, dense, fused, "largest batch")
    # 65535 one-pixel maps, dense from one tensor and fused from the 2 x 2 grids
    ones = G.resize_lanczos4(tg, (1, 1))
    ref1 = ref_resize(g, 1, 1)
    assert_bits(N(ones), ref1, "65535 one-pixel maps")
    refs = [RefMap(m, f"one-pixel map {i}") for i, m in enumerate(ref1)]
    check_metrics(refs, boxes, G.box_metrics(ones, boxes), G.grid_box_metrics(tg, (1, 1), boxes), "65535 one-pixel maps")


@pytest.mark.parametrize("h,w", [(24, 24), (64, 64), (1, 64), (5, 1)])
def test_hostile_grids(dev, h, w):
    grids = hostile_grids(h, w)
    sizes = HOSTILE_SIZES + [(w, h)]
    n = len(grids)
    sweep(dev, np.concatenate([grids] * len(sizes)), [s for s in sizes for _ in range(n)],
          lambda W, H: box_family(W, H)[:8] + [(0, 0, 1, 1), (W - 1, H - 1, 1, 1)], f"hostile grids {h}x{w}", assert_bits_or_nan)


def test_planted_extrema(dev):
    from attwarp_amd import grounding as G
    maps = planted_maps()
    names = list(maps)
    dmaps = {k: T(v, dev) for k, v in maps.items()}
    refs, tensors, boxes = [], [], []
    for name in names:
        m = N(dmaps[name])
        H, W = m.shape
        ref = RefMap(m, name)
        for box in box_family(W, H):
            refs.append(ref), tensors.append(dmaps[name]), boxes.append(box)
    dense = G.box_metrics(tensors, boxes)
    check_metrics(refs, boxes, dense, None, "planted extrema")
    arg = dict(zip([r.what for r in refs], N(dense.argmax).tolist()))
    assert arg["equal maxima in different tiles and bands"] == 10 * 513 + 300
    assert arg["a NaN in a later block, a larger finite value earlier"] == 400 * 513 + 400
    assert arg["two NaNs in different blocks"] == 10 * 513 + 500
    assert arg["all -inf"] == 0 and arg["all zero"] == 0 and arg["signed zeros"] == 0
    am = dict(zip([(r.what, b) for r, b in zip(refs, boxes)], N(dense.am).tolist()))
    assert am[("all zero", (0, 0, 513, 513))] == 0.0


# ---- limits: host-side refusals only --------------------------------------------------------------------------------------
def test_sizes_past_the_limits_raise_and_the_stream_stays_good(dev):
    from attwarp_amd import _lib, grounding as G
    refused = (ValueError, _lib.AttWarpError)
    ok = torch.zeros(2, 4, 4, device=dev)
    one = torch.zeros(1, 1, device=dev)

    def valid():                                                  # a full-size call on the same stream, bit for bit
        sizes = [(257, 256), (1, 513)]
        grids = case_grids(np.random.default_rng(4), sizes, 64, 64)
        sweep(dev, grids, sizes, lambda W, H: box_family(W, H)[:4], "after a refused call")

    for call in (lambda: G.resize_lanczos4(torch.zeros(2, 65, 4, device=dev), (10, 10)),
                 lambda: G.resize_lanczos4(torch.zeros(2, 4, 65, device=dev), (10, 10)),
                 lambda: G.grid_box_metrics(torch.zeros(2, 65, 4, device=dev), (10, 10), [(0, 0, 1, 1)] * 2),
                 lambda: G.grid_box_metrics(torch.zeros(2, 4, 65, device=dev), (10, 10), [(0, 0, 1, 1)] * 2),
                 lambda: G.resize_lanczos4(ok, (32769, 1)),
                 lambda: G.resize_lanczos4(ok, [(4, 4), (1, 32769)]),
                 lambda: G.grid_box_metrics(ok, (32769, 1), [(0, 0, 1, 1)] * 2),
                 lambda: G.box_metrics([torch.zeros(1, 32769, device=dev)], [(0, 0, 1, 1)]),
                 lambda: G.resize_lanczos4(torch.zeros(65536, 2, 2, device=dev), (1, 1)),
                 lambda: G.grid_box_metrics(torch.zeros(65536, 2, 2, device=dev), (1, 1), [(0, 0, 1, 1)] * 65536),
                 lambda: G.box_metrics([one] * 65536, [(0, 0, 1, 1)] * 65536),
                 lambda: G.box_metrics([one], [(1 << 40, 0, 1, 1)]),
                 lambda: G.box_metrics([one], [(0, 0, 1, -(1 << 40))]),
                 lambda: G.grid_box_metrics(ok, (5, 5), [(0, 0, 1, 1), (0, 1 << 40, 1, 1)])):
        with pytest.raises(refused):
            call()
        valid()
    # the ABI itself, past the Python checks: records of a valid call with one field past its limit
    rec = np.zeros(2, dtype=G._GRID_MAP_DTYPE)
    buf = torch.zeros(4096, device=dev)
    rec["src"] = rec["out"] = rec["ofs_x"] = rec["coef_x"] = rec["ofs_y"] = rec["coef_y"] = buf.data_ptr()
    rec["H"] = rec["W"] = 8
    rec_dev = torch.zeros(rec.nbytes, device=dev, dtype=torch.uint8)
    outs = [torch.zeros(2, device=dev, dtype=torch.int64), torch.zeros(2, device=dev, dtype=torch.int32),
            torch.zeros(2, device=dev, dtype=torch.float64)]
    ws = torch.zeros(4096, device=dev, dtype=torch.uint8)

    def abi(fused, h, w, M=2, **kw):
        r = rec.copy()
        for k_, v in kw.items():
            r[k_] = v
        return lambda: _lib.call("attwarp_box_metrics", r.ctypes.data, _lib.ptr(rec_dev), M, fused, h, w, *[_lib.ptr(o) for o in outs],
                                 _lib.ptr(ws), _lib.stream_ptr(dev))
    for call in (abi(1, 65, 4), abi(1, 4, 65), abi(1, 4, 4, W=32769), abi(0, 0, 0, H=32769), abi(1, 4, 4, M=65536),
                 abi(0, 0, 0, box_x=1 << 40), abi(1, 4, 4, box_h=-(1 << 40)),
                 lambda: _lib.call("attwarp_resize_lanczos4", rec.ctypes.data, _lib.ptr(rec_dev), 2, 65, 4, _lib.stream_ptr(dev)),
                 lambda: _lib.call("attwarp_resize_lanczos4", rec.ctypes.data, _lib.ptr(rec_dev), 65536, 4, 4, _lib.stream_ptr(dev))):
        with pytest.raises(_lib.AttWarpError):
            call()
    valid()


# ---- the head-mean probe ------------------------------------------------------------------------------------------------
def run_probe(dev, dt, q32, k32, starts, kv_begin, ntok, what):
    from attwarp_amd import attention_extraction as ae
    bf = dt == torch.bfloat16
    q, k = T(q32, dev).to(dt), T(k32, dev).to(dt)
    qn, kn = N(q.float() if bf else q), N(k.float() if bf else k)
    B, D = q32.shape[0], q32.shape[2]
    sc = D ** -0.5
    got = ae.probe_head_mean(q, k, torch.tensor(starts, dtype=torch.int32, device=dev), ntok,
                             None if kv_begin is None else torch.tensor(kv_begin, dtype=torch.int32, device=dev), sc)
    assert got.dtype == dt and tuple(got.shape) == (B, ntok), what
    g = N(got.float())
    for b in range(B):                                           # sample by sample: the restatement holds K in float64
        want = R.head_mean_rows(qn[b:b + 1], kn[b:b + 1], starts[b:b + 1], ntok, sc,
                                None if kv_begin is None else kv_begin[b:b + 1], bf16=bf)
        assert np.array_equal(g[b], want[0].astype(F32)), (what, b, int((g[b] != want[0]).sum()))
    return g


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("nc,group,hkv,ntok,kv", PROBE_CASES)
def test_head_mean_probe(dev, dt, nc, group, hkv, ntok, kv):
    esize = 4 if dt == torch.float32 else 2
    q, k, starts, kv_begin, D = probe_case(nc, group, hkv, ntok, kv, esize)
    what = f"head_mean {dt} D{D} heads{group * hkv}/{hkv} ntok{ntok} kv{kv}"
    g = run_probe(dev, dt, q, k, starts, kv_begin, ntok, what)
    assert g[2, -1] == 1.0 and not g[2, :-1].any(), what          # one attended key: the last of the span
    run_probe(dev, dt, q, k, starts, None, ntok, what + " unpadded")


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_head_mean_probe_refusals(dev, dt):
    from attwarp_amd import _lib, attention_extraction as ae
    esize = 4 if dt == torch.float32 else 2
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    D5 = 5 * (16 // esize)                                        # nc = 5: one lane of five chunks, more than launch_t has
    with pytest.raises(_lib.AttWarpError):
        ae.probe_head_mean(torch.zeros(1, 2, D5, device=dev, dtype=dt), torch.zeros(1, 2, 64, D5, device=dev, dtype=dt), st, 8)
    D = 16 // esize
    with pytest.raises(_lib.AttWarpError):                        # kv = MAX_KV + 1
        ae.probe_head_mean(torch.zeros(1, 1, D, device=dev, dtype=dt), torch.zeros(1, 1, 15873, D, device=dev, dtype=dt), st, 8)
    with pytest.raises(_lib.AttWarpError):                        # ntok = 1025
        ae.probe_head_mean(torch.zeros(1, 1, D, device=dev, dtype=dt), torch.zeros(1, 1, 2048, D, device=dev, dtype=dt), st, 1025)
    q, k, starts, kv_begin, _ = probe_case(1, 8, 1, 1, 15872, esize)
    run_probe(dev, dt, q, k, starts, kv_begin, 1, f"head_mean {dt} after a refused call")
