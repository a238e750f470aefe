"""The ragged CLIP preprocess (pipeline.ClipBatch / clip_preprocess_ragged / process_images, csrc/clip_ragged.hip) on the GPU
against Pillow: every comparison is bit for bit.  The reference (tests/clip_ragged_ref.py) pads with Pillow's own
Image.new + paste and resizes every channel with Image.resize; the product never builds the padded canvas.  Every case
asserts the route and register window the plan reports before it compares, so a change of geometry cannot move a case to
another path unnoticed."""
import types

import numpy as np
import pytest
import torch

import clip_ref as R
import clip_ragged_ref as G

pytestmark = pytest.mark.gpu
SIZE = G.SIZE
PATTERNS3 = ("blocks", "ramp", "noise")


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("the ragged CLIP preprocess needs a GPU (there is no CPU fallback)")
    from attwarp_amd import pipeline
    return pipeline


def N(t):
    return t.detach().cpu().numpy()


def plan_of(cb):
    return [(int(p["fused"]), int(p["window"])) for p in cb.plan]


def check_cases(P, cases, patterns=PATTERNS3, **kw):
    """One batch: every case under every pattern; the plan first, then every image against the cached reference."""
    specs = [(H, W, name, 11 + i) for i, (H, W, _, _) in enumerate(cases) for name in patterns]
    views = P.upload_images([G.image(*s) for s in specs])
    cb = P.ClipBatch(views, SIZE, torch.float32, **kw)
    assert plan_of(cb) == [(f, w) for (_, _, f, w) in cases for _ in patterns]
    got = N(cb.run())
    for i, s in enumerate(specs):
        assert np.array_equal(got[i], G.cached_reference(*s)), s
    return cb


@pytest.mark.parametrize("case", G.PAD_GEOMETRY, ids=lambda c: "%dx%d" % c[:2])
def test_padding_geometry(P, case):
    cb = check_cases(P, [case], R.PATTERNS)
    H, W = case[:2]
    n = max(H, W)
    p = cb.plan[0]
    assert (int(p["canvas_w"]), int(p["canvas_h"]), int(p["pad_x"]), int(p["pad_y"])) == (n, n, (n - W) // 2, (n - H) // 2)


@pytest.mark.parametrize("case", G.IDENTITY, ids=lambda c: "%dx%d" % c[:2])
def test_identity_edges(P, case):
    cb = check_cases(P, [case])
    H, W = case[:2]
    assert int(cb.plan[0]["ksize_x"]) == int(cb.plan[0]["ksize_y"]) == G.taps(max(H, W)) == {336: 1, 337: 7}[max(H, W)]


@pytest.mark.parametrize("i", range(len(G.WINDOW_EDGES)), ids=lambda i: "%dx%d" % G.WINDOW_EDGES[i][:2])
def test_register_window_edges(P, i):
    case, ntaps = G.WINDOW_EDGES[i], G.WINDOW_EDGE_TAPS[i]
    cb = check_cases(P, [case])
    assert int(cb.plan[0]["ksize_x"]) == int(cb.plan[0]["ksize_y"]) == ntaps == G.taps(max(case[:2]))
    assert (int(cb.header.n_fused_images), int(cb.header.n_split_images)) == ((3, 0) if case[2] else (0, 3))
    assert (cb.tmp is None) == bool(case[2])


def test_far_beyond_the_window(P):
    cb = check_cases(P, G.FAR, ("blocks", "noise"))
    assert int(cb.plan[0]["ksize_x"]) == 31 and int(cb.header.n_h_items) > 0 and int(cb.header.n_v_items) > 0


@pytest.mark.parametrize("case", G.DRIVERS, ids=lambda c: "%dx%d" % c[:2])
def test_driver_sizes(P, case):
    check_cases(P, [case], ("blocks", "noise"))


def test_alignment_of_packed_views(P):
    """Widths 40 .. 43 give every residue of 3W mod 4; behind a 1 x 1 image the packed views of upload_images start at
    odd byte addresses."""
    specs = [(1, 1, "noise", 3)] + [(H, W, "noise", 20 + W) for (H, W, _, _) in G.ALIGNMENT] + \
            [(H, W, "ramp", 30 + W) for (H, W, _, _) in G.ALIGNMENT]
    views = P.upload_images([G.image(*s) for s in specs])
    assert {v.data_ptr() % 4 for v in views[1:]} == {0, 1, 2, 3} and {3 * s[1] % 4 for s in specs[1:]} == {0, 1, 2, 3}
    cb = P.ClipBatch(views, SIZE, torch.float32)
    assert set(plan_of(cb)) == {(1, 8)}
    got = N(cb.run())
    for i, s in enumerate(specs):
        assert np.array_equal(got[i], G.cached_reference(*s)), s


def mixed_specs():
    """About 40 images drawn from every case list, a different pattern per image."""
    specs = [(H, W, R.PATTERNS[i % len(R.PATTERNS)], 40 + i) for i, (H, W, _, _) in enumerate(G.ALL_PAD)]
    specs += [(H, W, R.PATTERNS[(i + 3) % len(R.PATTERNS)], 90 + i) for i, (H, W, _, _) in enumerate(G.PAD_GEOMETRY + G.IDENTITY)]
    return specs


def test_mixed_batch(P):
    specs = mixed_specs()
    assert 38 <= len(specs) <= 44
    views = P.upload_images([G.image(*s) for s in specs])
    cb = P.ClipBatch(views, SIZE, torch.float32)
    assert plan_of(cb) == [(f, w) for (_, _, f, w) in G.ALL_PAD + G.PAD_GEOMETRY + G.IDENTITY]
    h = cb.header
    assert int(h.n_fused_images) + int(h.n_split_images) == len(specs) and int(h.n_split_images) == 3 and int(h.ks) == 16
    assert 0 < int(h.n_wide_items) < int(h.n_fused_items)
    got = cb.run().clone()
    for i, s in enumerate(specs):
        assert np.array_equal(N(got[i]), G.cached_reference(*s)), s
    for i, v in enumerate(views):                                   # every image alone
        assert torch.equal(P.ClipBatch([v], SIZE, torch.float32).run()[0], got[i]), specs[i]
    perm = np.random.default_rng(7).permutation(len(specs))
    assert torch.equal(P.ClipBatch([views[j] for j in perm], SIZE, torch.float32).run(), got[torch.as_tensor(perm, device=got.device)])


def test_three_hundred_tiny_images(P):
    sizes = [(1, 1), (2, 3), (5, 8), (3, 2), (7, 7), (8, 5)]
    specs = [sizes[b % len(sizes)] + ("noise", 1000 + b) for b in range(300)]
    views = P.upload_images([G.image(*s) for s in specs])
    cb = P.ClipBatch(views, SIZE, torch.float32)
    assert int(cb.header.n_fused_images) == 300 and cb.plan.shape == (300,)
    got = N(cb.run())
    for b, spec in enumerate(specs):
        assert np.array_equal(got[b], G.reference(G.image(*spec))), (b, spec)


CONSTANT_CASES = [(48, 61, 1, 8), (5, 8, 1, 8), (40, 505, 1, 16), (40, 1177, 0, 0)]


def test_output_dtypes_and_constants(P):
    imgs = [G.image(H, W, "blocks" if i % 2 else "noise", 60 + i) for i, (H, W, _, _) in enumerate(CONSTANT_CASES)]
    views = P.upload_images(imgs)
    want32 = np.stack([G.reference(im) for im in imgs])
    got32 = P.ClipBatch(views, SIZE, torch.float32).run()
    got16 = P.ClipBatch(views, SIZE, torch.float16).run()
    assert got32.dtype == torch.float32 and got16.dtype == torch.float16 and got16.shape == (len(imgs), 3, SIZE, SIZE)
    assert np.array_equal(N(got32), want32)
    assert torch.equal(got16.cpu(), torch.from_numpy(want32).to(torch.float16))
    assert torch.equal(P.clip_preprocess_ragged(views), got16)      # the one-shot form: float16, padded, by default
    # per-channel constants that all differ, one mean negative, one std above 1
    got = P.ClipBatch(views, SIZE, torch.float32, R.SWEEP_MEAN[:3], R.SWEEP_STD[:3], background=G.background_of(R.OPENAI_CLIP_MEAN)).run()
    want = np.stack([G.reference(im, mean=R.SWEEP_MEAN, std=R.SWEEP_STD, background=G.background_of(R.OPENAI_CLIP_MEAN)) for im in imgs])
    assert np.array_equal(N(got), want)
    # a background that is neither the default nor equal across channels
    bg = (0, 255, 7)
    cb = P.ClipBatch(views, SIZE, torch.float32, background=bg)
    assert plan_of(cb) == [(f, w) for (_, _, f, w) in CONSTANT_CASES]
    assert np.array_equal(N(cb.run()), np.stack([G.reference(im, background=bg) for im in imgs]))
    assert not np.array_equal(N(cb.run()), want32)


def test_one_channel_images(P):
    imgs = [G.image(H, W, "noise", 70 + i, C=1) for i, (H, W) in enumerate([(48, 61), (61, 48), (40, 505), (5, 8)])]
    got = P.ClipBatch(P.upload_images(imgs), SIZE, torch.float32).run()
    assert got.shape == (4, 1, SIZE, SIZE)
    assert np.array_equal(N(got), np.stack([G.reference(im) for im in imgs]))


def test_both_routes_give_the_same_bytes(P):
    """The one-launch kernel against the two-launch route forced through the tuning library, on one batch that holds both
    register windows, padding on either axis, identity tables and the drivers' sizes."""
    from attwarp_amd import _lib
    cases = G.PAD_GEOMETRY + G.IDENTITY[:3] + G.WINDOW_EDGES[:6] + G.DRIVERS[:2]
    specs = [(H, W, PATTERNS3[i % 3], 80 + i) for i, (H, W, _, _) in enumerate(cases)]
    views = P.upload_images([G.image(*s) for s in specs])
    for dtype in (torch.float32, torch.float16):
        a = P.ClipBatch(views, SIZE, dtype)
        assert int(a.header.n_split_images) == 0 and a.tmp is None
        fused = a.run()
        with _lib.debug_override(clip_ragged_variant=1):
            b = P.ClipBatch(views, SIZE, dtype)
            assert int(b.header.n_fused_images) == 0 and int(b.header.tmp_bytes) > 0 and set(plan_of(b)) == {(0, 0)}
            split = b.run()
        assert torch.equal(fused, split)
    # and without the hook, through the window-edge pair: 1176 (last fused) and 1177 (first two-launch) against Pillow
    check_cases(P, [G.WINDOW_EDGES[4], G.WINDOW_EDGES[6]], ("blocks",))


NO_PAD = [(500, 375), (48, 61), (375, 500)]


def test_resize_and_crop_without_padding(P):
    imgs = [G.image(H, W, PATTERNS3[i], 100 + i) for i, (H, W) in enumerate(NO_PAD)]
    views = P.upload_images(imgs)
    cb = P.ClipBatch(views, SIZE, torch.float32, pad_to_square=False)
    assert set(plan_of(cb)) == {(1, 8)}
    for p, (H, W) in zip(cb.plan, NO_PAD):
        nh, nw, top, left = R.geometry(H, W, SIZE)
        assert (int(p["canvas_h"]), int(p["canvas_w"]), int(p["nh"]), int(p["nw"]), int(p["top"]), int(p["left"])) == (H, W, nh, nw, top, left)
        assert int(p["pad_x"]) == int(p["pad_y"]) == int(p["vertical_first"]) == 0
    got = cb.run()
    for i, im in enumerate(imgs):
        assert np.array_equal(N(got[i]), R.clip_preprocess(im, SIZE)), NO_PAD[i]
        assert torch.equal(got[i], P.clip_preprocess(views[i][None], SIZE, torch.float32)[0]), NO_PAD[i]


def test_vertical_first_image(P):
    """More than 100 times as high as wide and shrinking vertically: Pillow runs the vertical pass first; a tall image that
    does not shrink keeps the usual order.  Both in one batch with a plain image, size 32."""
    shapes = [(4100, 40), (48, 61), (300, 2)]
    imgs = [G.image(H, W, "blocks" if i == 0 else "noise", 110 + i, size=32) for i, (H, W) in enumerate(shapes)]
    cb = P.ClipBatch(P.upload_images(imgs), 32, torch.float32, pad_to_square=False)
    assert [int(v) for v in cb.plan["vertical_first"]] == [1, 0, 0]          # 300 x 2 grows to 4800 x 32: horizontal first
    assert plan_of(cb)[0] == (0, 0) and plan_of(cb)[1] == (1, 16)
    got = N(cb.run())
    for i, im in enumerate(imgs):
        assert np.array_equal(got[i], R.clip_preprocess(im, 32)), shapes[i]


def test_streams_and_graphs(P):
    cases = [G.PAD_GEOMETRY[4], G.WINDOW_EDGES[2], G.WINDOW_EDGES[6], G.DRIVERS[0]]
    views = P.upload_images([G.image(H, W, "noise", 120 + i) for i, (H, W, _, _) in enumerate(cases)])
    cb = P.ClipBatch(views, SIZE, torch.float16)
    eager = cb.run().clone()
    assert int(cb.header.n_fused_images) == 3 and int(cb.header.n_split_images) == 1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    cb.out.zero_()
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(side):
        cb.run()
    side.synchronize()
    assert torch.equal(cb.out, eager)
    graph, out = P.capture_step(cb.run)
    assert out is cb.out
    for _ in range(2):
        cb.out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cb.out, eager)


def test_pad_route_equals_the_dense_entry_point(P):
    for i, (H, W) in enumerate([(61, 48), (375, 500), (683, 1024)]):
        v = P.upload_images([G.image(H, W, "noise", 130 + i)])[0]
        want = P.clip_preprocess(P.expand2square(v[None]), SIZE, torch.float32)
        assert torch.equal(P.ClipBatch([v], SIZE, torch.float32).run(), want), (H, W)
        assert torch.equal(want, P.clip_preprocess(v[None], SIZE, torch.float32, pad_to_square=True))


def test_process_images_equals_the_hf_processor(P):
    pytest.importorskip("transformers")
    from PIL import Image
    from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil
    proc = CLIPImageProcessorPil(size={"shortest_edge": SIZE}, crop_size={"height": SIZE, "width": SIZE})
    shapes = [(375, 500), (500, 333), (61, 48), (336, 336), (427, 640)]
    pil = [Image.fromarray(G.image(H, W, PATTERNS3[i % 3], 140 + i)) for i, (H, W) in enumerate(shapes)]
    bg = tuple(int(x * 255) for x in proc.image_mean)
    padded = [Image.fromarray(G.pad_canvas(np.asarray(im), bg)) for im in pil]
    want = proc.preprocess(padded, return_tensors="np")["pixel_values"]
    got = P.process_images(pil, proc, types.SimpleNamespace(image_aspect_ratio="pad"))
    assert got.dtype == torch.float32 and got.is_cuda and np.array_equal(N(got), want)
    half = P.process_images(pil, proc, types.SimpleNamespace(image_aspect_ratio="pad"), dtype=torch.float16)
    assert torch.equal(half, got.to(torch.float16))
    # no aspect mode: the processor alone (resize + centre crop)
    plain = P.process_images(pil, proc, types.SimpleNamespace())
    assert np.array_equal(N(plain), proc.preprocess(pil, return_tensors="np")["pixel_values"])
    with pytest.raises(NotImplementedError):
        P.process_images(pil, proc, types.SimpleNamespace(image_aspect_ratio="anyres"))


def test_argument_checks(P):
    from attwarp_amd import _lib
    dev = torch.device("cuda")
    ok = torch.zeros(4, 5, 3, device=dev, dtype=torch.uint8)
    with pytest.raises(TypeError):
        P.ClipBatch([ok.float()])
    with pytest.raises(TypeError):
        P.ClipBatch([np.zeros((4, 5, 3), np.uint8)])
    with pytest.raises(TypeError):
        P.ClipBatch([ok], dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        P.ClipBatch([ok, torch.zeros(4, 5, 1, device=dev, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        P.ClipBatch([])
    with pytest.raises(ValueError):
        P.clip_preprocess_ragged([])
    with pytest.raises(ValueError):
        P.ClipBatch([torch.zeros(0, 5, 3, device=dev, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        P.ClipBatch([ok], out=torch.empty(1, 3, SIZE, SIZE, device=dev, dtype=torch.float32))      # float16 was asked for
    with pytest.raises(_lib.AttWarpError, match="canvas 8193 x 8193 exceeds 8192"):
        P.ClipBatch([torch.zeros(8193, 1, 3, device=dev, dtype=torch.uint8)])
    assert P.ClipBatch([torch.zeros(8192, 1, 3, device=dev, dtype=torch.uint8)]).header.n_split_images == 1
