"""GPU tests of the trainer's data preparation (attwarp_amd.dataloader -> csrc/dataprep.hip) against the numpy restatement
tests/dataprep_ref.py (which test_dataprep_cpu.py ties to Pillow and to the reference's own dataloader): the ragged image
batch on the one-launch kernel and on the two-launch route, the attention maps, the composed batch against
tests/golden/dataprep.npz, and the refusals.  Every comparison is bit for bit."""
import os

import numpy as np
import pytest
import torch

import dataprep_ref as R

pytestmark = pytest.mark.gpu

# (H, W) pairs.  As width x height these are 1x1, 2x3, 7x5, 37x91, 64x48, 375x500, 683x1024 (W = 683: rows of 2049 bytes),
# 512x512 (both passes skipped at 512), 512x300 and 300x512 (one pass skipped)
RAGGED_HW = [(1, 1), (3, 2), (5, 7), (91, 37), (48, 64), (500, 375), (1024, 683), (512, 512), (300, 512), (512, 300)]
TARGETS = [512, (24, 40), 1]


@pytest.fixture(scope="module")
def dev():
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
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def images_of(sizes, seed, C=3):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        a = rng.integers(0, 256, (h, w, C), dtype=np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        a[..., 0] = (127 + 120 * np.sin(xx / 3.0) * np.cos(yy / 5.0)).astype(np.uint8)      # structure next to the noise
        out.append(a)
    return out


@pytest.fixture(scope="module")
def ragged():
    """The ragged batch and its reference per target, computed once."""
    imgs = images_of(RAGGED_HW, 7)
    return imgs, {str(t): R.prepare_images(imgs, t) for t in TARGETS}


def assert_equal(got, want, what=""):
    got = N(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), [int(b) for b in np.unique(np.nonzero(bad)[0])][:8])


@pytest.mark.parametrize("target", TARGETS, ids=str)
def test_ragged_images(dev, ragged, target):
    from attwarp_amd import dataloader as D
    imgs, want = ragged
    P = D.PreparedImages([T(a, dev) for a in imgs], target)
    if target == 512:               # every image on the one-launch kernel; the small targets shrink the wide images by more
        assert P.header.n_fused_images == len(imgs) and P.header.n_split_images == 0 and P.tmp is None      # than its 16 taps hold
    assert P.header.n_fused_images + P.header.n_split_images == len(imgs) and P.header.n_fused_images >= 3
    assert_equal(P.run(), want[str(target)], target)


def test_host_images_go_through_one_upload(dev, ragged):
    from PIL import Image
    from attwarp_amd import dataloader as D
    imgs, want = ragged
    assert_equal(D.prepare_images(imgs, (24, 40)), want[str((24, 40))], "numpy")
    assert_equal(D.prepare_images([Image.fromarray(a) for a in imgs], (24, 40)), want[str((24, 40))], "PIL")


def test_forced_two_launch_route_equals_the_fused_one(dev, ragged):
    from attwarp_amd import _lib, dataloader as D
    imgs, want = ragged
    dimgs = [T(a, dev) for a in imgs]
    for target in TARGETS:
        with _lib.debug_override(prep_variant=1):
            P = D.PreparedImages(dimgs, target)
            assert P.header.n_fused_images == 0 and P.header.n_split_images == len(imgs) and P.header.tmp_bytes > 0
            split = P.run()
        F = D.PreparedImages(dimgs, target)
        assert F.header.n_fused_images >= 3
        fused = F.run()
        assert torch.equal(split, fused), target
        assert_equal(split, want[str(target)], target)


def test_downscale_past_the_register_window(dev):
    """16x down-scales need 35 horizontal taps (130 -> 8): the two-launch route; a source 2000 high and 8 wide is one of those
    Image.resize runs vertical pass first."""
    from attwarp_amd import dataloader as D
    imgs = images_of([(130, 130), (2000, 8)], 11)
    for target in (8, (8, 9)):
        P = D.PreparedImages([T(a, dev) for a in imgs], target)
        assert P.header.n_fused_images == 0 and list(P.plan["vertical_first"]) == [0, 1]
        assert_equal(P.run(), R.prepare_images(imgs, target), target)
    mixed = images_of([(130, 130), (64, 48), (2000, 8), (7, 5)], 12)                       # both routes in one call
    P = D.PreparedImages([T(a, dev) for a in mixed], (8, 9))
    assert (P.header.n_fused_images, P.header.n_split_images) == (2, 2)
    assert_equal(P.run(), R.prepare_images(mixed, (8, 9)), "mixed")


def test_every_band_size_the_launcher_picks(dev):
    """Band heights 64 / 32 / 16 follow the vertical scale, 8 and 4 staged rows follow the LDS; band counts that do not
    divide the target; the 16-tap register window; a plan above half a CU's LDS."""
    from attwarp_amd import dataloader as D
    seen = set()
    cases = [((72, 40), [(100, 50), (72, 33), (71, 30), (32, 30), (31, 30), (5, 7)], 8),
             ((72, 40), [(100, 50), (60, 200), (31, 30)], 16),                                # 200 -> 40: 11 taps
             ((48, 768), [(96, 768), (48, 300), (96, 1200)], 8),
             ((24, 2048), [(20, 2048), (10, 2048), (7, 5)], 8)]
    for k, (target, sizes, ks) in enumerate(cases):
        imgs = images_of(sizes, 20 + k)
        P = D.PreparedImages([T(a, dev) for a in imgs], target)
        assert P.header.n_split_images == 0 and P.header.ks == ks, (target, P.header.ks)
        seen |= {(int(p["ny"]), int(p["rb"])) for p in P.plan}
        assert_equal(P.run(), R.prepare_images(imgs, target), (target, sizes))
        if k == 1:                      # the 11-tap image alone takes the 16-tap window, in a launch of its own
            wide = -(-72 // int(P.plan["ny"][1]))
            assert 0 < P.header.n_wide_items == wide < P.header.n_fused_items
        else:
            assert P.header.n_wide_items == 0
        if k == 3:
            assert P.header.lds_bytes > 80 * 1024
    assert {ny for ny, _ in seen} == {8, 16, 32, 64} and {rb for _, rb in seen} == {4, 8}, seen


def test_band_past_the_reserved_lds_rows_is_nan_not_wrong_pixels(dev):
    """The host bounds a band's source rows from H, S_h and ksize_y; a table whose record reserves fewer LDS rows than the
    band's taps span must not be computed from clamped taps: that band's output is NaN, the other bands are untouched."""
    from attwarp_amd import dataloader as D
    imgs = images_of([(100, 50), (64, 48)], 41)
    P = D.PreparedImages([T(a, dev) for a in imgs], (72, 40))
    want = R.prepare_images(imgs, (72, 40))
    assert_equal(P.run(), want, "untouched plan")
    ny, cap = int(P.plan["ny"][0]), int(P.plan["nr_cap"][0])
    P.plan["nr_cap"][0] = 3                                       # fewer rows than any band of 16 needs at scale 100 / 72
    assert cap > 3 and P.header.n_fused_images == 2
    P.table_dev.copy_(torch.from_numpy(P.table_host))
    got = N(P.run())
    assert np.isnan(got[0]).all()
    assert_equal(got[1:], want[1:], "the other image")
    P.plan["nr_cap"][0] = cap


def test_run_on_another_stream_than_the_planning_one(dev, ragged):
    from attwarp_amd import dataloader as D
    imgs, want = ragged
    dimgs = [T(a, dev) for a in imgs]
    rng = np.random.default_rng(9)
    maps = [rng.random((24, 24), dtype=np.float32) * 3, rng.random((16, 32), dtype=np.float32)]
    dmaps = [T(m, dev) for m in maps]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    P = D.PreparedImages(dimgs, (24, 40))
    A = D.PreparedAttention(dmaps, (24, 40))
    with torch.cuda.stream(side):                                  # no wait_stream: run() orders itself behind the uploads
        out, att = P.run(), A.run()
    side.synchronize()
    assert_equal(out, want[str((24, 40))], "side stream")
    assert_equal(att, R.prepare_attention_maps(maps, (24, 40)), "side stream, attention")


def test_300_small_images_in_one_call(dev):
    from attwarp_amd import dataloader as D
    imgs = images_of([(7, 5)] * 300, 31)
    P = D.PreparedImages(D.pipeline.upload_images(imgs), 24)
    assert P.header.n_fused_items == 300
    assert_equal(P.run(), R.prepare_images(imgs, 24), "300 x (7, 5)")


def test_images_at_odd_byte_offsets_and_single_channel(dev, ragged):
    from attwarp_amd import dataloader as D
    imgs, want = ragged
    sizes = [a.size for a in imgs]
    flat = torch.zeros(sum(sizes) + 2 * len(imgs) + 1, device=dev, dtype=torch.uint8)
    views, off = [], 1
    for a, n in zip(imgs, sizes):
        flat[off:off + n] = T(a, dev).reshape(-1)
        views.append(flat[off:off + n].view(*a.shape))
        off += n + (2 if (off + n) % 2 else 1)                                             # keep every start odd
    assert all(v.data_ptr() % 2 == 1 for v in views)
    assert_equal(D.prepare_images(views, (24, 40)), want[str((24, 40))], "odd offsets")
    assert_equal(D.prepare_images(views, 512), want["512"], "odd offsets, one launch")
    gray = images_of([(91, 37), (48, 64), (1024, 683), (5, 7)], 33, C=1)
    out = D.prepare_images([T(a, dev) for a in gray], (40, 24))
    assert tuple(out.shape) == (4, 1, 40, 24)
    assert_equal(out, R.prepare_images(gray, (40, 24)), "C = 1")
    assert_equal(D.prepare_images([T(a, dev) for a in gray[2:]], 512), R.prepare_images(gray[2:], 512), "C = 1, one launch")


def test_captured_graph_equals_the_eager_call(dev, ragged):
    from attwarp_amd import dataloader as D, pipeline
    imgs, want = ragged
    P = D.PreparedImages([T(a, dev) for a in imgs], (24, 40))
    eager = P.run().clone()
    rng = np.random.default_rng(5)
    maps = [T(rng.random((24, 24), dtype=np.float32) * 3, dev), T(rng.random((16, 32), dtype=np.float32), dev)]
    A = D.PreparedAttention(maps, (24, 40))
    eager_a = A.run().clone()
    graph, _ = pipeline.capture_step(lambda: (P.run(), A.run()))
    P.out.zero_(); A.out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(P.out, eager) and torch.equal(A.out, eager_a)
    assert_equal(P.out, want[str((24, 40))], "graph")


def attention_cases():
    rng = np.random.default_rng(61)
    le1 = rng.random((24, 24), dtype=np.float32)                                   # max <= 1: taken as it is
    gt1 = rng.random((700, 1000), dtype=np.float32) * np.float32(9.25)             # max > 1: divided
    zero_neg = -rng.random((16, 32), dtype=np.float32)
    zero_neg[::2] = 0
    nan = rng.random((16, 32), dtype=np.float32) * np.float32(4)                   # NaN: must not divide
    nan[3, 4] = np.nan
    inf = rng.random((24, 24), dtype=np.float32) * np.float32(2)
    inf[1, 1], inf[2, 2] = np.inf, -np.inf
    one = np.array([[2.5]], dtype=np.float32)
    allzero = np.zeros((1, 1), dtype=np.float32)
    return [le1, gt1, zero_neg, nan, inf, one, allzero]


@pytest.mark.parametrize("target", [512, (24, 100), 1], ids=str)
def test_attention_maps(dev, target):
    from attwarp_amd import dataloader as D
    maps = attention_cases()
    want = R.prepare_attention_maps(maps, target)
    assert_equal(D.prepare_attention_maps([T(m, dev) for m in maps], target), want, target)
    if target == (24, 100):
        assert_equal(D.prepare_attention_maps(maps, target), want, "numpy maps")
        w3 = want[3, 0]                                             # the NaN map was not divided: values above 1 clip to 1
        assert (w3 == 1.0).sum() > 100 and (R.prepare_attention_maps([np.nan_to_num(maps[3])], target)[0, 0] != w3).any()


def test_attention_without_normalisation_every_gray(dev):
    """The overlay branch: gray / 255 for every gray 0 .. 255 through x255 + truncation, and values that are not grays."""
    from attwarp_amd import dataloader as D
    gray = (np.arange(256, dtype=np.float32).reshape(16, 16) / 255.0).astype(np.float32)
    big = (np.arange(256, dtype=np.float32).reshape(16, 16) / np.float32(100.0)).astype(np.float32)      # max > 1, not divided
    for target in (16, (24, 100)):
        want = R.prepare_attention_maps([gray, big], target, normalize=False)
        assert_equal(D.prepare_attention_maps([T(gray, dev), T(big, dev)], target, normalize=False), want, target)
    # float32(g / 255) * 255 lands on or just above g for every gray, so the truncation gives g back: the loader's round trip
    assert np.array_equal(R.attention_u8(gray, normalize=False).reshape(-1), np.arange(256))


def test_collate_on_the_reference_fixture(dev, golden):
    from attwarp_amd import dataloader as D, pipeline
    fx = golden("dataprep")
    S, n = int(fx["S"]), int(fx["n"])
    mapping = dict(zip([str(s) for s in fx["category_names"]], [str(s) for s in fx["category_transforms"]]))
    kinds = [str(fx[f"kind_{i}"]) for i in range(n)]
    images = [fx[f"image_in_{i}"] for i in range(n)]
    datasets = [str(fx[f"dataset_{i}"]) for i in range(n)]
    buckets = [str(fx[f"bucket_{i}"]) or None for i in range(n)]
    questions, answers = [f"question {i}?" for i in range(n)], [f"answer {i}" for i in range(n)]
    for normalize in (True, False):
        idx = [i for i in range(n) if (kinds[i] == "npy") == normalize]
        maps = [fx[f"attention_in_{i}"] if normalize else fx[f"attention_loaded_{i}"] for i in idx]
        pick = lambda col: [col[i] for i in idx]
        batch = D.collate(pick(images), maps, pick(questions), pick(answers), pick(datasets), pick(buckets), S, normalize)
        assert set(batch) == {"image", "attention_map", "q_str", "answer", "dataset", "bucket"}
        assert batch["image"].is_cuda and batch["attention_map"].is_cuda
        assert_equal(batch["image"], np.stack([fx[f"image_{i}"] for i in idx]), "image")
        assert_equal(batch["attention_map"], np.stack([fx[f"attention_map_{i}"] for i in idx]), "attention_map")
        assert (batch["q_str"], batch["answer"], batch["dataset"], batch["bucket"]) == \
            (pick(questions), pick(answers), pick(datasets), pick(buckets))
        full = D.prepare_trainer_batch(pick(images), maps, pick(questions), pick(answers), pick(datasets), pick(buckets),
                                       mapping, S, grid=(8, 8), normalize=normalize)
        assert full["transforms"] == [R.transform_for_sample(d, b, mapping) for d, b in zip(pick(datasets), pick(buckets))]
        A, px, py = pipeline.trainer_attention_targets(batch["attention_map"], full["transforms"], (8, 8))
        assert torch.equal(full["attention_map"], batch["attention_map"]) and torch.equal(full["image"], batch["image"])
        assert torch.equal(full["A"], A) and torch.equal(full["px_gt"], px) and torch.equal(full["py_gt"], py)


def test_refusals(dev):
    from attwarp_amd import dataloader as D
    img = torch.zeros(8, 8, 3, device=dev, dtype=torch.uint8)
    att = torch.zeros(8, 8, device=dev, dtype=torch.float32)
    with pytest.raises(TypeError):
        D.prepare_images([img.float()], 8)                                     # wrong dtype
    with pytest.raises(TypeError):
        D.prepare_images([np.zeros((8, 8, 3), np.float32)], 8)
    with pytest.raises(ValueError):
        D.prepare_images([img[0]], 8)                                          # rank
    with pytest.raises(ValueError):
        D.prepare_images([img[:, :, :2]], 8)                                   # C = 2
    with pytest.raises(ValueError):
        D.prepare_images([img, img[:, :, :1]], 8)                              # mixed channel counts
    with pytest.raises(ValueError):
        D.prepare_images([img], None)                                          # native sizes cannot be stacked
    with pytest.raises(ValueError):
        D.prepare_images([], 8)
    with pytest.raises(RuntimeError):
        D.prepare_images([img.cpu(), img], 8)                                  # no CPU path
    with pytest.raises(TypeError):
        D.prepare_attention_maps([att.double()], 8)
    with pytest.raises(ValueError):
        D.prepare_attention_maps([att[None]], 8)                               # 3-D arrays are the caller's
    with pytest.raises(ValueError):
        D.prepare_attention_maps([att], None)
    with pytest.raises(ValueError):
        D.collate([img, img], [att], ["q", "q"], ["a", "a"], ["gqa", "gqa"], [None, None], 8)      # mismatched lengths
    with pytest.raises(ValueError):
        D.prepare_trainer_batch([img], [att], ["q"], ["a"], ["gqa"], [None, None], {}, 8)
    with pytest.raises(ValueError):
        D.PreparedImages([img], 8, out=torch.empty(1, 3, 8, 9, device=dev))
