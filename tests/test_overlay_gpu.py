"""GPU tests of the Jet heat-map overlays (attwarp_heatmap_overlay) against the numpy restatement of tests/overlay_ref.py,
bit for bit: blend_mask's merged image, save_warped_image's overlay file, the dense / list / ragged batch forms, and the
overlay of batches that come out of the ragged chain streams."""
import os

import numpy as np
import pytest
import torch

import overlay_ref as R
from oracle import warp_oracle as O
from conftest import main_batched_loop_inputs

pytestmark = pytest.mark.gpu


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


def smooth_mask(rng, h, w):
    """An up-sampled-mask-like uint8 map: smooth, with a sub-range of values."""
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.sin(xx / (3.0 + w / 9)) * np.cos(yy / (5.0 + h / 7)) + rng.random((h, w)) * 0.05
    lo, hi = sorted(rng.integers(0, 256, 2))
    hi = max(hi, lo + 1)
    return (lo + (f - f.min()) / (np.ptp(f) + 1e-12) * (hi - lo)).astype(np.uint8)


@pytest.mark.parametrize("grayscale", [0, 0.3, 1.0])
def test_blend_mask_merged_image_main_batched_loop(dev, grayscale):
    """blend_mask on the five driver images (683 x 1024 among them) and their masks, the last one the constant 1/576 map
    (revise_mask -> all-zero mask, min == max): the merged image equals the restatement and is not the input image."""
    from PIL import Image
    from attwarp_amd import attention_extraction as ae
    imgs, atts = main_batched_loop_inputs()
    alpha = R.blend_alpha(grayscale)
    for img, att in zip(imgs, atts):
        pil = Image.fromarray(img)
        merged, mask = ae.blend_mask(pil, torch.from_numpy(att).to(dev), 10, 3, Image.LANCZOS, grayscale)
        assert merged.mode == "RGB" and merged.size == pil.size
        got = np.asarray(merged)
        want = R.blend_mask_overlay(img, np.asarray(mask), alpha)
        assert np.array_equal(got, want)
        assert not np.array_equal(got, img)
    # the mask of the constant map is constant: every pixel takes Jet index 0
    m = np.asarray(mask)
    assert m.min() == m.max()


def test_blend_mask_random_images_and_masks(dev):
    from PIL import Image
    from attwarp_amd import attention_extraction as ae
    rng = np.random.default_rng(41)
    for (h, w) in [(333, 500), (61, 683), (40, 41), (97, 1021)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        att = (rng.random((24, 24)) ** 4).astype(np.float32)
        merged, mask = ae.blend_mask(Image.fromarray(img), torch.from_numpy(att).to(dev), 10, 3, Image.LANCZOS, 0)
        mota = O.lanczos_resize_u8(O.mask_to_u8(O.revise_mask(att, 3, 10)), w, h)
        assert np.array_equal(np.asarray(mask), mota)
        assert np.array_equal(np.asarray(merged), R.blend_mask_overlay(img, mota, 0.5))


@pytest.mark.parametrize("alpha", [0.5, 0.3, 1.0, 0.7, 0.123])
def test_overlay_list_form_both_styles_any_size(dev, alpha):
    """Sizes whose pixel count is not a multiple of 4 (the per-pixel tail), single pixels, 683-wide rows; images and
    maps at odd byte offsets of one buffer; RGB and BGR orders."""
    from attwarp_amd import pipeline
    rng = np.random.default_rng(int(alpha * 1000))
    sizes = [(1, 1), (3, 5), (7, 683), (64, 683), (64, 684), (129, 257), (300, 433)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    maps = [smooth_mask(rng, h, w) for h, w in sizes]
    maps[3][:] = 77                                                     # min == max
    flat = np.concatenate([x.ravel() for pair in zip(imgs, maps) for x in pair] + [np.zeros(1, np.uint8)])
    buf = T(np.concatenate([np.zeros(1, np.uint8), flat]), dev)        # everything one byte off
    views, off = [], 1
    for x in [x for pair in zip(imgs, maps) for x in pair]:
        views.append(buf[off:off + x.size].view(x.shape)); off += x.size
    dimgs, dmaps = views[0::2], views[1::2]
    assert any(t.data_ptr() % 4 for t in dimgs)
    got = pipeline.heatmap_overlay(dimgs, dmaps, alpha, "blend_mask")
    for g, img, m in zip(got, imgs, maps):
        assert np.array_equal(N(g), R.blend_mask_overlay(img, m, alpha))
    got = pipeline.heatmap_overlay(dimgs, dmaps, alpha, "save_warped", order="bgr")          # images taken as BGR
    for g, img, m in zip(got, imgs, maps):
        assert np.array_equal(N(g), R.save_warped_overlay(img, m, alpha))
    got = pipeline.heatmap_overlay(dimgs, dmaps, alpha, "save_warped", order="bgr", out_order="rgb")
    for g, img, m in zip(got, imgs, maps):
        assert np.array_equal(N(g), R.save_warped_overlay(img, m, alpha)[:, :, ::-1])
    got = pipeline.heatmap_overlay(dimgs, dmaps, alpha, "blend_mask", order="rgb", out_order="bgr")
    for g, img, m in zip(got, imgs, maps):
        assert np.array_equal(N(g), R.blend_mask_overlay(img, m, alpha)[:, :, ::-1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_overlay_float_maps(dev, dtype):
    """save_warped style on float maps: arithmetic in the map's dtype; NaN anywhere / infinite ranges -> index 0."""
    from attwarp_amd import pipeline
    rng = np.random.default_rng(7)
    sizes = [(50, 683), (33, 35), (2, 3), (128, 128), (20, 20), (21, 22), (9, 9)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    maps = [(rng.random((h, w)) ** 2 * 3 - 1).astype(dtype) for h, w in sizes]
    maps[3] = (maps[3] * dtype(1e-12)).astype(dtype)                    # a range below EPSILON
    maps[4][3, 4] = np.nan
    maps[5][0, 0] = np.inf
    maps[6][8, 8] = -np.inf
    got = pipeline.heatmap_overlay([T(i, dev) for i in imgs], [T(m, dev) for m in maps], 0.4, "save_warped", order="bgr")
    for k, (g, img, m) in enumerate(zip(got, imgs, maps)):
        assert np.array_equal(N(g), R.save_warped_overlay(img, m, 0.4)), k


def test_dense_and_list_forms_agree(dev):
    from attwarp_amd import pipeline
    rng = np.random.default_rng(3)
    B, H, W = 4, 75, 683
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    m8 = np.stack([smooth_mask(rng, H, W) for _ in range(B)])
    for style, maps in (("blend_mask", m8), ("save_warped", m8), ("save_warped", rng.random((B, H, W)).astype(np.float32))):
        dense = pipeline.heatmap_overlay(T(img, dev), T(maps, dev), 0.5, style)
        lst = pipeline.heatmap_overlay([T(i, dev) for i in img], [T(m, dev) for m in maps], 0.5, style)
        assert dense.shape == (B, H, W, 3)
        for b in range(B):
            assert torch.equal(dense[b], lst[b])


def _save_warped_case(tmp_path, pil, att, **kw):
    from attwarp_amd import new_method as nm
    ov, out, out0 = tmp_path / "ov.png", tmp_path / "w.png", tmp_path / "w0.png"
    for p in (ov, out, out0):
        if p.exists():
            p.unlink()
    ok = nm.save_warped_image(pil, att, None, str(ov), str(out), width=120, height=90, **kw)
    ok0 = nm.save_warped_image(pil, att, None, None, str(out0), width=120, height=90, **kw)
    return ok, ok0, ov, out, out0


def test_save_warped_image_writes_the_overlay(dev, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(11)
    h, w = 75, 683
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rgba = np.concatenate([img, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=2)
    m8 = smooth_mask(rng, h, w)
    cases = [("u8", Image.fromarray(img), m8, m8),
             ("f32", Image.fromarray(img), (m8 / 255.0).astype(np.float32), (m8 / 255.0).astype(np.float32)),
             ("f64", Image.fromarray(img), m8 / 300.0, m8 / 300.0),
             ("rgba", Image.fromarray(rgba, "RGBA"), m8, m8)]
    small8 = smooth_mask(rng, 40, 300)                                   # resized to the image's size first
    cases.append(("u8 resized", Image.fromarray(img), small8, O.resize_linear_cv2(small8, (w, h))))
    small32 = (rng.random((40, 300)) ** 2).astype(np.float32)
    cases.append(("f32 resized", Image.fromarray(img), small32, O.resize_linear_cv2(small32, (w, h))))
    for name, pil, att, att_at_size in cases:
        for alpha in (0.5, 0.35):
            ok, ok0, ov, out, out0 = _save_warped_case(tmp_path, pil, att, attention_alpha=alpha)
            assert ok and ok0, name
            want_bgr = R.save_warped_overlay(img[:, :, ::-1], att_at_size, alpha)
            got = np.asarray(Image.open(ov))
            assert got.shape == (h, w, 3) and np.array_equal(got, want_bgr[:, :, ::-1]), (name, alpha)
            # the warped output is what it is without the overlay
            assert np.array_equal(np.asarray(Image.open(out)), np.asarray(Image.open(out0))), name


def test_save_warped_image_overlay_errors_stop_before_the_warp(dev, tmp_path, capsys):
    from PIL import Image
    rng = np.random.default_rng(12)
    img = Image.fromarray(rng.integers(0, 256, (40, 50, 3), dtype=np.uint8))
    ok, ok0, ov, out, out0 = _save_warped_case(tmp_path, img, rng.random((40, 50)).astype(np.float16))
    assert not ok and ok0 and not ov.exists() and not out.exists() and out0.exists()
    assert "Error during processing" in capsys.readouterr().err
    ok, ok0, ov, out, out0 = _save_warped_case(tmp_path, img, rng.random((20, 25)))     # float64 map to be resized
    assert not ok and ok0 and not out.exists()


def test_overlay_ragged_batch(dev):
    """heatmap_overlay_ragged on a batch of warp_from_masks_ragged: the packed masks read in place, images at odd byte
    offsets of upload_images' buffer (683-wide rows among them) -> equals blend_mask image by image."""
    from PIL import Image
    from attwarp_amd import attention_extraction as ae, pipeline
    imgs, atts = main_batched_loop_inputs()
    rng = np.random.default_rng(13)
    imgs = imgs + [rng.integers(0, 256, (101, 683, 3), dtype=np.uint8), rng.integers(0, 256, (77, 61, 3), dtype=np.uint8)]
    atts = atts + [(rng.random((24, 24)) ** 3).astype(np.float32) for _ in range(2)]
    dimgs = pipeline.upload_images([Image.fromarray(i) for i in imgs], dev)
    assert any(t.data_ptr() % 4 for t in dimgs)
    a24 = torch.from_numpy(np.stack(atts)).to(dev)
    _, rb = pipeline.warp_from_masks_ragged(dimgs, a24, (90, 120), return_batch=True)
    assert rb is not None
    packed, views = pipeline.heatmap_overlay_ragged(rb)
    assert packed.dim() == 1 and len(views) == len(imgs)
    for b, img in enumerate(imgs):
        assert views[b].shape == img.shape and views[b].data_ptr() % 16 == 0
        merged, _ = ae.blend_mask(Image.fromarray(img), a24[b], 10, 3, Image.LANCZOS, 0)
        assert np.array_equal(N(views[b]), np.asarray(merged)), b
        assert np.array_equal(N(views[b]), R.blend_mask_overlay(img, N(rb.mota_of(b)), 0.5)), b
    _, v3 = pipeline.heatmap_overlay_ragged(rb, alpha=0.3, out_order="bgr")
    for b, img in enumerate(imgs):
        assert np.array_equal(N(v3[b]), R.blend_mask_overlay(img, N(rb.mota_of(b)), 0.3)[:, :, ::-1])


def test_overlay_of_ragged_stream_batches(dev):
    """Batches returned by RaggedMaskChainStream.push / flush own their masks: their overlays, enqueued after they come
    back, equal the overlays of the same batches run alone."""
    from attwarp_amd import pipeline
    rng = np.random.default_rng(14)
    sizes = [(70, 61), (52, 96), (96, 75), (40, 683)]
    batches = []
    for _ in range(6):
        imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for h, w in sizes]
        batches.append((imgs, torch.from_numpy((rng.random((4, 24, 24)) ** 3).astype(np.float32)).to(dev)))
    st = pipeline.RaggedMaskChainStream(out_size=(80, 88))
    done = [st.push(i, m) for i, m in batches]
    done = [d for d in done if d is not None] + st.flush()
    assert len(done) == 6
    got = [pipeline.heatmap_overlay_ragged(d)[1] for d in done]
    for (imgs, m24), g in zip(batches, got):
        _, rb = pipeline.warp_from_masks_ragged(imgs, m24, (80, 88), return_batch=True)
        want = pipeline.heatmap_overlay_ragged(rb)[1]
        for b in range(len(imgs)):
            assert torch.equal(g[b], want[b])
            assert np.array_equal(N(g[b]), R.blend_mask_overlay(N(imgs[b]), N(rb.mota_of(b)), 0.5))


def test_overlay_of_shared_mask_stream_batches(dev):
    """MaskChainStream(pattern="ragged"): the batches of one parity share one mask buffer.  Batch j's overlay enqueued
    right after step j - 3 (the step that up-sampled its mask) sees batch j's mask, before step j - 1 overwrites it."""
    from attwarp_amd import attention_extraction as ae, pipeline
    rng = np.random.default_rng(15)
    n, B, H, W = 5, 3, 64, 683
    images = [torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev) for _ in range(n)]
    masks = [torch.from_numpy((rng.random((B, 24, 24)) ** 3).astype(np.float32)).to(dev) for _ in range(n)]
    mc = pipeline.MaskChainStream(images, masks, out_size=(80, 88), pattern="ragged")
    def check(j):
        _, views = pipeline.heatmap_overlay_ragged(mc.ragged_batch(j))
        mota = N(ae.upsample_mask_lanczos(ae.revise_mask(masks[j % n], 3, 10), (W, H)))
        img = N(images[j % n])
        for b in range(B):
            assert np.array_equal(N(views[b]), R.blend_mask_overlay(img[b], mota[b], 0.5)), (j, b)
    mc.prime()                       # ran L(0), L(1), L(2): batch 2's mask is the latest of parity 0
    check(2)
    for k in range(4):
        mc.step()                    # step k ran L(k + 3)
        check(k + 3)


def test_integration_md_masked_png_snippet(dev, tmp_path):
    """INTEGRATION.md's driver block followed by its overlay block, exec'd as written: every sample gets a _masked.png that
    is not the original image and equals the restatement of blend_mask at the drivers' settings (grayscale = 0)."""
    import re, types
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    loop = re.search(r"```python\n(from attwarp_amd import pipeline\nimgs = pipeline.upload_images.*?)```", text, re.S).group(1)
    overlay = re.search(r"```python\n(_, merged = pipeline.heatmap_overlay_ragged.*?)```", text, re.S).group(1)
    rng = np.random.default_rng(63)
    sizes = [(61, 100), (90, 683), (64, 64)]
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in sizes]
    att = [torch.rand(24, 24, device=dev) ** 2 for _ in sizes]
    dirs = {k: tmp_path / k for k in ("warped", "att", "masked")}
    for d in dirs.values():
        d.mkdir()
    ns = dict(b_images=[Image.fromarray(h) for h in host], attn_maps=att, model=types.SimpleNamespace(device=dev), torch=torch, np=np,
              os=os, Image=Image, DEFAULT_HEIGHT=80, DEFAULT_WIDTH=88, enhance_coe=10, kernel_size=3, current_bs=len(sizes),
              sample_id=lambda j: f"img{j}", WARPED_IMAGES_DIR=str(dirs["warped"]), ATTENTION_MAPS_DIR=str(dirs["att"]),
              MASKED_IMAGES_DIR=str(dirs["masked"]))
    exec(compile(loop + overlay, "INTEGRATION.md", "exec"), ns)
    for j, (h, w) in enumerate(sizes):
        mota = O.lanczos_resize_u8(O.mask_to_u8(O.revise_mask(N(att[j]), 3, 10)), w, h)
        got = np.asarray(Image.open(dirs["masked"] / f"img{j}_masked.png"))
        assert got.shape == host[j].shape and not np.array_equal(got, host[j])
        assert np.array_equal(got, R.blend_mask_overlay(host[j], mota, R.blend_alpha(0)))
