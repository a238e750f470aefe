"""The Stable-Diffusion warp ablation on the GPU: csrc/sdwarp.hip and attwarp_amd.sd_warp against the numpy restatement
(tests/sdwarp_ref.py), bit for bit, and against the fixture recorded from the reference (tests/golden/sd_warp.npz)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import sdwarp_ref as R  # noqa: E402
import test_sdwarp_cpu as C  # noqa: E402  (the fixture, its inputs and the bounds derived there)

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
TOKENS = (1, 7, 64, 77, 256)
BH = ((1, 1), (2, 5), (2, 20))


@pytest.fixture(scope="module")
def sd():
    from attwarp_amd import sd_warp
    return sd_warp


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def hw_sizes(tokens):
    c = R.xattn_chunk(tokens)
    return (1, 9, 144, c - 1, c, c + 1, 2 * c + 3) if c > 1 else (1, 9, 144, c, c + 1, 2 * c + 3)


def make_tensor(rng, shape, dtype, offset=0):
    """A random tensor of positive values in the dtype (optionally a view at an element offset into its buffer) and the
    numpy array the restatement reads (bf16: float32 holding the bf16 values)."""
    n = int(np.prod(shape))
    buf = torch.from_numpy(rng.random(n + offset).astype(F32)).to(dev()).to(TORCH_DT[dtype])
    t = buf[offset:].view(*shape)
    host = t.float().cpu().numpy() if dtype == "bf16" else t.cpu().numpy()
    return t, host


def as_np(t, dtype):
    return t.float().cpu().numpy() if dtype == "bf16" else t.cpu().numpy()


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    assert np.array_equal(got.view(u)[~nan], want.view(u)[~nan])


def check_reduce(sd, tensors, hosts, want_hw, dtype):
    sums, hw = sd.xattn_reduce(tensors, want_hw)
    sums = as_np(sums, dtype)
    for m, (a, w) in enumerate(zip(hosts, want_hw)):
        ts, ht = R.xattn_reduce(a, dtype)
        same_bits(sums[m], ts)
        if w:
            same_bits(as_np(hw[m], dtype), ht)
        else:
            assert hw[m] is None


# ---- the reduce ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("tokens", TOKENS)
def test_reduce_every_shape(sd, tokens, dtype):
    """Every HW x (B, heads) of one tokens / dtype in ONE call (records of all sizes side by side)."""
    rng = np.random.default_rng(tokens * 7 + len(dtype))
    tensors, hosts = [], []
    for HW in hw_sizes(tokens):
        for (B, heads) in BH:
            t, a = make_tensor(rng, (B, heads, HW, tokens), dtype)
            tensors.append(t)
            hosts.append(a)
    check_reduce(sd, tensors, hosts, [True] * len(tensors), dtype)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_reduce_odd_element_offset(sd, dtype):
    rng = np.random.default_rng(3)
    c = R.xattn_chunk(77)
    t, a = make_tensor(rng, (2, 5, c + 1, 77), dtype, offset=1)           # slices at changing 16-byte phases
    assert t.data_ptr() % 4 == 2
    check_reduce(sd, [t], [a], [True], dtype)
    for off in (1, 3, 7):                                                   # one phase for all slices (144 * 77 = 8 * 1386),
        t, a = make_tensor(rng, (2, 5, 144, 77), dtype, offset=off)         # groups cut at the head and tail of every chunk
        assert t.data_ptr() % 16 == 2 * off
        check_reduce(sd, [t], [a], [True], dtype)


def test_reduce_mixed_call(sd):
    rng = np.random.default_rng(40)
    sizes = hw_sizes(7)
    tensors, hosts, want = [], [], []
    for i in range(40):
        B, heads = BH[i % 3]
        t, a = make_tensor(rng, (B, heads, sizes[i % len(sizes)], 7), "f16", offset=i % 2)
        tensors.append(t)
        hosts.append(a)
        want.append(i % 3 != 1)
    check_reduce(sd, tensors, hosts, want, "f16")


def test_reduce_65535_records(sd):
    rng = np.random.default_rng(5)
    M = 65535
    big = torch.from_numpy(rng.random((M, 2, 3, 1, 7)).astype(F32)).to(dev())
    sums, hw = sd.xattn_reduce(list(big.view(M, 2, 3, 1, 7)), [i % 2 == 0 for i in range(M)])
    a = big.cpu().numpy().astype(F64)                       # [M,B,heads,1,tokens]: the documented order, vectorised over M
    tot = np.zeros((M, 7))
    acc_h = np.zeros((M, 7))
    for h in range(3):
        acc_b = np.zeros((M, 7))
        for b in range(2):
            acc_b = acc_b + a[:, b, h, 0]
        tot = tot + acc_b
        acc_h = acc_h + acc_b.astype(F32).astype(F64)
    same_bits(sums.cpu().numpy(), tot.astype(F32))
    for m in (0, 2, 65534):
        same_bits(hw[m].cpu().numpy(), acc_h[m].astype(F32)[None])
    assert hw[1] is None


def test_reduce_float16_overflow_stores_inf(sd):
    t = torch.full((2, 5, 144, 7), 0.5, dtype=torch.float16, device=dev())
    t[..., 0] = 60.0                                        # 2 * 5 * 144 * 60 = 86400 > 65504
    sums, hw = sd.xattn_reduce([t], [True])
    got = sums.cpu().numpy()[0]
    assert np.isposinf(got[0]) and got[1] == np.float16(720.0)
    check_reduce(sd, [t], [t.cpu().numpy()], [True], "f16")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_reduce_against_fsum(sd, dtype):
    """Independent of the restatement: the exact sum (math.fsum) rounded once, at most 1 ulp of the dtype away."""
    rng = np.random.default_rng(11)
    t, a = make_tensor(rng, (2, 5, 144, 7), dtype)
    got = sd.xattn_reduce([t], [False])[0].cpu().numpy()[0]
    for k in range(7):
        exact = math.fsum(a[..., k].astype(F64).ravel().tolist())
        want = np.array(exact).astype(a.dtype)
        assert abs(float(got[k]) - float(want)) <= float(np.spacing(want)), (k, got[k], want)


def test_reduce_refusals(sd):
    from attwarp_amd import _lib
    t = torch.ones(1, 2, 3, 4, device=dev())

    def valid():
        s, _ = sd.xattn_reduce([t], [False])
        assert np.array_equal(s.cpu().numpy(), np.full((1, 4), 6.0, F32))

    rec = np.zeros(65536, dtype=sd._XATTN_DTYPE)
    out = torch.empty(4, device=dev())
    ws = torch.empty(1 << 16, device=dev(), dtype=torch.uint8)
    rec["attn"], rec["token_sums"], rec["B"], rec["heads"], rec["HW"] = t.data_ptr(), out.data_ptr(), 1, 2, 3
    rec_dev = torch.from_numpy(rec.view(np.uint8)).to(dev())
    for M, tokens in ((1, 0), (1, 257), (65536, 4)):
        with pytest.raises(_lib.AttWarpError):
            _lib.call("attwarp_xattn_reduce", rec.ctypes.data, rec_dev.data_ptr(), M, _lib.F32, tokens, ws.data_ptr(),
                      _lib.stream_ptr(dev()))
        valid()
    with pytest.raises(RuntimeError):
        sd.xattn_reduce([t.cpu()], [False])
    valid()
    with pytest.raises(ValueError):
        sd.xattn_reduce([t, t], [False])
    valid()
    with pytest.raises(ValueError):
        sd.xattn_reduce([torch.ones(1, 1, 1, 257, device=dev())], [False])
    valid()


# ---- the fixture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_drop_in_names_against_the_reference(sd, dtype):
    x, shapes = C.inputs(dtype)
    cap = {s: {k: torch.from_numpy(x[(s, k)]).to(dev()).view(x[(s, k)].shape[0], x[(s, k)].shape[1], *shapes[(s, k)], -1)
               for k in C.LAYERS} for s in C.STEPS}
    red = sd.reduce_captured_maps(cap, keep_hw_tok=1)
    for mode, kw in (("all", {}), ("sel", dict(inference_step_selection=[801, 621], num_layers=2)),
                     ("last", dict(last_timestep=True))):
        want = C.GOLD[f"imp_{mode}_{dtype}"]
        _, bound = C.restated_importance(dtype, mode)
        for source in (cap, red):
            got = sd.compute_token_importance(source, **kw)
            assert got.dtype == want.dtype
            err = np.abs(got.astype(F64) - want.astype(F64))
            print(f"importance {mode} {dtype}: max err {err.max():.3e}, smallest bound {bound.min():.3e}")
            assert np.all(err <= bound)
    top = list(np.argsort(sd.compute_token_importance(red))[-C.TOP_K:][::-1])
    assert top == list(C.GOLD[f"top_{dtype}"])
    _, bound = C.aggregated(dtype)
    want = C.GOLD[f"agg_{dtype}"]
    for source in (cap, red):
        got = sd.aggregate_attention_map_for_tokens(source, top, inference_step_selection=None, num_last_layers=1)
        assert got.dtype == np.float32 and got.shape == want.shape
        err = np.abs(got.astype(F64) - want.astype(F64)).max()
        print(f"aggregate {dtype}: max err {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    with pytest.raises(ValueError):
        sd.compute_token_importance(red, inference_step_selection=[])
    with pytest.raises(ValueError):
        sd.aggregate_attention_map_for_tokens(red, top, inference_step_selection=[])


def test_aggregate_resizes_smaller_maps(sd):
    """Layers of different sizes: token_maps (torch's own sum(-1) in the dtype, as in the reference) within the float32
    summation bound k * 2^-24 * sum|v| of the restatement; from those maps on -- cubic resize of the smaller maps to the
    largest (:394-397), np.mean's order, min-max -- every bit."""
    rng = np.random.default_rng(9)
    idx = [3, 1, 4]
    cap, hws = {}, []
    for s, (H, W) in ((5, (4, 6)), (9, (8, 8)), (7, (8, 8))):
        t, a = make_tensor(rng, (2, 3, H, W, 11), "f32")
        cap[s] = {0: t}
        hws.append(R.xattn_reduce(a.reshape(2, 3, H * W, 11), "f32")[1].reshape(H, W, 11))
    red = sd.reduce_captured_maps(cap, keep_hw_tok=1)
    maps = []
    for s, hw in zip((5, 7, 9), (hws[0], hws[2], hws[1])):          # sorted steps
        same_bits(red.hw_tok[(s, 0)].cpu().numpy(), hw)
        m = sd.token_maps(red.hw_tok[(s, 0)], idx).cpu().numpy()
        bound = len(idx) * 2.0 ** -24 * np.abs(hw[..., idx].astype(F64)).sum(axis=-1)
        assert np.all(np.abs(m.astype(F64) - R.token_maps(hw, idx, "f32").astype(F64)) <= bound)
        maps.append(m)
    same_bits(sd.aggregate_attention_map_for_tokens(red, idx), R.aggregate_from_maps(maps))
    same_bits(sd.aggregate_attention_map_for_tokens(cap, idx), R.aggregate_from_maps(maps))


# ---- INTER_CUBIC -----------------------------------------------------------------------------------------------------------
def run_cubic(sd, srcs, sizes):
    outs = sd.resize_cubic([torch.from_numpy(np.ascontiguousarray(s)).to(dev()) for s in srcs], sizes)
    return [o.cpu().numpy() for o in outs]


def test_cubic_every_size_in_one_call(sd):
    rng = np.random.default_rng(1)
    sides = (1, 2, 255, 256, 257, 513)
    srcs, sizes = [], []
    for (h, w) in ((1, 1), (2, 2), (3, 5), (12, 12), (96, 96)):
        s = rng.standard_normal((h, w)).astype(F32)
        for W in sides:
            for H in sides:
                srcs.append(s)
                sizes.append((W, H))
    for s, (W, H), got in zip(srcs, sizes, run_cubic(sd, srcs, sizes)):
        same_bits(got, R.resize_cubic(s, W, H))


def test_cubic_large_sources_and_copies(sd):
    rng = np.random.default_rng(2)
    a = rng.standard_normal((200, 300)).astype(F32)
    b = rng.standard_normal((5, 4)).astype(F32)
    srcs = [a, a, a, b, b]
    sizes = [(64, 48), (500, 500), (300, 200), (32768, 3), (3, 32768)]
    for s, (W, H), got in zip(srcs, sizes, run_cubic(sd, srcs, sizes)):
        same_bits(got, R.resize_cubic(s, W, H))


def test_cubic_special_values(sd):
    a = np.arange(30, dtype=F32).reshape(5, 6) - 7
    a[1, 2], a[3, 4], a[0, 0], a[4, 5], a[2, 2] = np.nan, np.inf, -np.inf, -0.0, 0.0
    z = np.full((3, 3), -0.0, F32)
    srcs, sizes = [a, a, z, z], [(17, 11), (3, 2), (7, 5), (3, 3)]
    for s, (W, H), got in zip(srcs, sizes, run_cubic(sd, srcs, sizes)):
        same_bits(got, R.resize_cubic(s, W, H))


def test_cubic_65535_maps(sd):
    rng = np.random.default_rng(4)
    M = 65535
    src = rng.standard_normal((M, 2, 3)).astype(F32)
    t = torch.from_numpy(src).to(dev())
    outs = sd.resize_cubic(list(t), [(4, 3)] * M)
    want = R.resize_cubic(src, 4, 3)
    got = outs[0].new_empty(0)
    got = torch.stack(outs).cpu().numpy()
    same_bits(got, want)


def test_cubic_refusals(sd):
    m = torch.ones(2, 2, device=dev())
    with pytest.raises(ValueError):
        sd.resize_cubic([m], [(0, 3)])
    with pytest.raises(ValueError):
        sd.resize_cubic([m], [(3, 32769)])
    with pytest.raises(ValueError):
        sd.resize_cubic([m.double()], [(3, 3)])
    same_bits(sd.resize_cubic([m], [(3, 3)])[0].cpu().numpy(), R.resize_cubic(np.ones((2, 2), F32), 3, 3))


# ---- blur and min-max ----------------------------------------------------------------------------------------------------------
SIDES = (1, 2, 3, 5, 255, 256, 257, 513)


def test_blur_and_normalise_every_size(sd):
    rng = np.random.default_rng(6)
    maps = [rng.standard_normal((H, W)).astype(F32) for H in SIDES for W in SIDES]
    t = [torch.from_numpy(m).to(dev()) for m in maps]
    blurred = sd.blur5(t)
    both = sd.blur5_normalize(t)
    plain = sd.minmax_normalize(t)
    for m, tb, bn, pn, src in zip(maps, blurred, both, plain, t):
        b = R.blur5(m)
        same_bits(tb.cpu().numpy(), b)
        same_bits(bn.cpu().numpy(), R.minmax_normalize(b))
        same_bits(pn.cpu().numpy(), R.minmax_normalize(m))
        same_bits(src.cpu().numpy(), m)                              # inputs untouched


def test_normalise_constant_nan_inf_and_in_place(sd):
    c = np.full((5, 300), 2.5, F32)
    n = np.arange(600, dtype=F32).reshape(3, 200)
    n[1, 150] = np.nan
    i1 = np.arange(12, dtype=F32).reshape(3, 4)
    i1[0, 0] = -np.inf
    i2 = i1.copy()
    i2[0, 0] = np.inf
    r = np.random.default_rng(8).standard_normal((70, 130)).astype(F32)
    maps = [c, n, i1, i2, r, np.zeros((1, 1), F32)]
    t = [torch.from_numpy(m.copy()).to(dev()) for m in maps]
    for m, bn in zip(maps, sd.blur5_normalize(t)):
        same_bits(bn.cpu().numpy(), R.minmax_normalize(R.blur5(m)))
    outs = sd.minmax_normalize(t, in_place=True)
    for m, o, src in zip(maps, outs, t):
        assert o is src
        same_bits(src.cpu().numpy(), R.minmax_normalize(m))
    assert np.array_equal(t[0].cpu().numpy(), np.zeros((5, 300), F32))
    assert np.isnan(t[1].cpu().numpy()).all()


def test_upsample_attention_map(sd):
    a = np.random.default_rng(10).random((12, 12)).astype(F32)
    got = sd.upsample_attention_map(a, (70, 61))
    same_bits(got, R.upsample_attention_map(a, (70, 61)))


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _images(rng):
    shapes = ((40, 61), (57, 33), (64, 80))
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in shapes]
    maps = [rng.random(s).astype(F32) for s in ((12, 12), (7, 9), (80, 100))]
    return images, maps


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("transform,inverse", [("identity", False), ("exp", True), ("log", False)])
def test_iterative_warp(sd, iterations, transform, inverse):
    rng = np.random.default_rng(12)
    images, maps = _images(rng)
    got = sd.iterative_warp([torch.from_numpy(i).to(dev()) for i in images], [torch.from_numpy(m).to(dev()) for m in maps],
                            iterations, (50, 44), transform, 1.5, 2.0, inverse)
    want = R.iterative_warp(images, maps, iterations, (50, 44), transform, 1.5, 2.0, inverse)
    assert len(got) == iterations
    for g, w in zip(got, want):
        g = g.cpu().numpy()
        assert g.shape == (3, 44, 50, 3) and g.dtype == np.uint8
        for b in range(3):
            assert np.array_equal(g[b], w[b])


def test_save_warped_image_round_trip(sd, tmp_path):
    from PIL import Image
    from attwarp_amd import new_method
    rng = np.random.default_rng(13)
    images, maps = _images(rng)
    bgr, att = images[0], maps[0]
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "out.png")
    new_method._imwrite(src, bgr)
    assert sd.save_warped_image(src, att, dst, width=50, height=44, transform="sqrt", exp_scale=1.0, exp_divisor=1.0) is True
    got = np.array(Image.open(dst).convert("RGB"))[:, :, ::-1]
    want = sd.iterative_warp([torch.from_numpy(bgr).to(dev())], [torch.from_numpy(att).to(dev())], 1, (50, 44), "sqrt")[0][0]
    assert np.array_equal(got, want.cpu().numpy())
    assert sd.ATTENTION_TRANSFORM == "sqrt"
    same = rng.random(bgr.shape[:2]).astype(F32)
    sd.set_transform_function("identity")
    w2 = sd.warp_image_by_attention(bgr, same, 50, 44)
    assert np.array_equal(w2, R.warp_u8(__import__("oracle.warp_oracle", fromlist=["x"]), bgr, same, 50, 44, "identity", 1.0, 1.0, False))
    assert sd.save_warped_image_original(src, maps[1], dst, width=50, height=44) is True
    assert np.array(Image.open(dst)).shape == (44, 50, 3)
    with pytest.raises(FileNotFoundError):
        sd.save_warped_image(str(tmp_path / "missing.png"), att, dst)
