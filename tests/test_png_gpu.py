"""GPU tests of the PNG encoder (attwarp_png_encode, attwarp_amd/png.py): every file equals the restatement of
tests/png_ref.py byte for byte AND decodes with Pillow to the pixels it was made from."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as K
import png_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def decode(png: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(png)))


def same_bytes(got: bytes, want: bytes, what):
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(f"{what}: {len(got)} bytes against the restatement's {len(want)}, first difference at byte {first}")


def check_file(png: bytes, img: np.ndarray, filt, order, what, want=None):
    same_bytes(png, R.encode(img, filt, order) if want is None else want, what)
    pix = img[:, :, ::-1] if order == "bgr" and img.shape[2] == 3 else img
    assert np.array_equal(decode(png).reshape(pix.shape), pix), what


def test_every_case_equals_the_restatement_and_decodes():
    """All cases of tests/png_cases.py (tiny and odd widths, segment geometry, run lengths, single symbol, the length
    limiter, stored fallback, every filter on three patterns, channel order) in ONE call, filters and orders per image."""
    from attwarp_amd import png
    cases = K.cases()
    tens = [torch.from_numpy(i).to(DEV) for _, i, _, _ in cases]
    b = png.PngBatch(tens, filter=[c[2] for c in cases], order=[c[3] for c in cases])
    files = png.download(*b.run())
    offs = b.offsets.cpu().numpy()
    assert offs[0] == 0 and (np.diff(offs) == [len(f) for f in files]).all() and offs[-1] <= b.bound
    assert b.bound == sum(R.bound(*i.shape) for _, i, _, _ in cases)
    for (name, img, filt, order), f in zip(cases, files):
        check_file(f, img, filt, order, name, K.reference(name, filt, order))


def test_bgr_equals_rgb_of_the_flipped_image():
    from attwarp_amd import png
    img = K.photo(23, 31, 3, 5)
    t = torch.from_numpy(img).to(DEV)
    flipped = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1])).to(DEV)
    for filt in ("sub", "paeth", "adaptive"):
        assert png.encode_png([t], filt, "bgr") == png.encode_png([flipped], filt, "rgb")


def test_odd_addresses_pitch_and_input_forms():
    from attwarp_amd import png
    img = K.photo(19, 27, 3, 2)
    H, W, C = img.shape
    pitch = W * C + 7
    flat = torch.zeros(3 + H * pitch, dtype=torch.uint8, device=DEV)
    view = flat[3:].as_strided((H, W, C), (pitch, C, 1))                      # odd byte address, rows 88 bytes apart
    view.copy_(torch.from_numpy(img))
    assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
    grey = K.photo(11, 13, 1, 3)
    wide = torch.from_numpy(np.ascontiguousarray(np.pad(grey[:, :, 0], ((0, 0), (2, 4))))).to(DEV)
    files = png.encode_png([view, wide[:, 2:15], torch.from_numpy(grey).to(DEV)], "paeth")
    check_file(files[0], img, "paeth", "rgb", "odd address and pitch")
    check_file(files[1], grey, "paeth", "rgb", "[H,W] slice of a wider tensor")
    assert files[2] == files[1]
    dense = np.stack([K.photo(9, 14, 3, s) for s in range(3)])
    for f, im in zip(png.encode_png(torch.from_numpy(dense).to(DEV)), dense):  # one [B,H,W,C] tensor
        check_file(f, im, "sub", "rgb", "dense batch")


def test_limits_raise_before_any_launch():
    from attwarp_amd import png
    ok = torch.zeros(2, png.PNG_MAX_ROW_BYTES - 1, dtype=torch.uint8, device=DEV)
    assert len(png.encode_png([ok])) == 1 and png.PNG_MAX_ROW_BYTES == R.MAX_ROW_BYTES    # a row at the limit encodes
    with pytest.raises(ValueError):
        png.PngBatch([torch.zeros(2, png.PNG_MAX_ROW_BYTES, dtype=torch.uint8, device=DEV)])
    with pytest.raises(ValueError):
        png.PngBatch([torch.zeros(2, png.PNG_MAX_ROW_BYTES // 3 + 1, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(ValueError):
        png.PngBatch([torch.zeros(4, 6, 2, dtype=torch.uint8, device=DEV)])                    # two channels
    with pytest.raises(ValueError):
        png.PngBatch([torch.zeros(0, 6, 3, dtype=torch.uint8, device=DEV)])                    # H = 0
    with pytest.raises(ValueError):
        png.PngBatch([torch.zeros(4, 12, 3, dtype=torch.uint8, device=DEV)[:, ::2]])           # pixels not dense
    with pytest.raises(ValueError):
        png.PngBatch([torch.zeros(4, 3, 6, dtype=torch.uint8, device=DEV).permute(0, 2, 1)])   # channels not innermost
    with pytest.raises(ValueError):
        png.PngBatch([ok], filter="best")


@pytest.fixture(scope="module")
def ragged():
    from attwarp_amd import png
    imgs = K.ragged_batch()
    tens = [torch.from_numpy(i).to(DEV) for i in imgs]
    filters = [png.FILTERS[i % len(png.FILTERS)] for i in range(len(imgs))]
    want = [R.encode(i, f) for i, f in zip(imgs, filters)]
    return imgs, tens, filters, want


def test_ragged_batch_of_forty(ragged):
    """Noise (stored blocks) and flat / smooth images (dynamic blocks) share the launch; offsets are contiguous and every
    file is what its image gives alone."""
    from attwarp_amd import png
    imgs, tens, filters, want = ragged
    assert imgs[0].shape[:2] == (1, 1) and imgs[-1].shape[:2] == (200, 333)
    b = png.PngBatch(tens, filter=filters)
    buf, offs = b.run()
    files = png.download(buf, offs)
    o = offs.cpu().numpy()
    assert o[0] == 0 and (np.diff(o) == [len(w) for w in want]).all()
    for i, (f, im, ft, w) in enumerate(zip(files, imgs, filters, want)):
        check_file(f, im, ft, "rgb", f"image {i} {im.shape} {ft}", w)
    stored = [R.idat_payload(f)[2] == 0 for f in files]
    assert any(stored) and not all(stored)
    for i in (7, 38):                                        # alone, and next to other neighbours
        assert png.encode_png([tens[i]], filters[i])[0] == files[i]
        assert png.encode_png([tens[39], tens[i], tens[0]], [filters[39], filters[i], filters[0]])[1] == files[i]


def test_graph_replay_gives_the_same_bytes(ragged):
    from attwarp_amd import png
    imgs, tens, filters, want = ragged
    b = png.PngBatch(tens, filter=filters)
    b.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.run()
    b.buffer.zero_()
    b.offsets.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert png.download(b.buffer, b.offsets) == want
    tens[5].copy_(torch.from_numpy(np.ascontiguousarray(imgs[5][::-1])))       # the sources are read at every replay
    g.replay()
    torch.cuda.synchronize()
    files = png.download(b.buffer, b.offsets)
    tens[5].copy_(torch.from_numpy(imgs[5]))
    assert files[5] == R.encode(imgs[5][::-1], filters[5]) and files[6:] == want[6:] and files[:5] == want[:5]


def _att(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.random((h, w)).astype(np.float32) ** 3
    a[h // 3: h // 2, w // 4: w // 2] += 2.0
    return a


def test_save_warped_image_hip_encoder_writes_the_same_pixels(tmp_path):
    from attwarp_amd import new_method as nm
    for k, (h, w) in enumerate([(37, 52), (64, 45)]):
        pil = Image.fromarray(K.photo(h, w, 3, 20 + k))
        att = _att(h, w, k) if k == 0 else _att(24, 24, k)                    # the second map is resized to the image
        names = {e: [str(tmp_path / f"{e}_{k}_{n}.png") for n in ("orig", "overlay", "warped")] for e in ("default", "pillow", "hip")}
        assert nm.save_warped_image(pil, att, *names["default"], width=48, height=40, transform="sqrt")
        assert nm.save_warped_image(pil, att, *names["pillow"], width=48, height=40, transform="sqrt", encoder="pillow")
        assert nm.save_warped_image(pil, att, *names["hip"], width=48, height=40, transform="sqrt", encoder="hip")
        for d, p, hp in zip(names["default"], names["pillow"], names["hip"]):
            assert open(d, "rb").read() == open(p, "rb").read()
            a, b = np.asarray(Image.open(p)), np.asarray(Image.open(hp))
            assert a.shape == b.shape and np.array_equal(a, b), hp
            same_bytes(open(hp, "rb").read(), R.encode(a), hp)
        assert np.array_equal(np.asarray(Image.open(names["pillow"][0])), np.asarray(pil))
        if k == 0:                                           # the default route still writes what the warp returns
            warped = nm.warp_image_by_attention(np.ascontiguousarray(np.asarray(pil)[:, :, ::-1]), att, 48, 40, "sqrt")
            assert np.array_equal(np.asarray(Image.open(names["default"][2])), warped[:, :, ::-1])
    assert nm.save_warped_image(pil, att, None, None, str(tmp_path / "x.png"), encoder="gpu") is False


def test_save_png_ragged(tmp_path):
    from attwarp_amd import pipeline
    rng = np.random.default_rng(31)
    sizes = [(40, 50), (33, 61), (64, 48), (57, 35)]
    imgs = [K.photo(h, w, 3, 40 + i) for i, (h, w) in enumerate(sizes)]
    dimgs = pipeline.upload_images(imgs, DEV)
    m24 = torch.from_numpy((rng.random((4, 24, 24), dtype=np.float32) ** 3)).to(DEV)
    out, rb = pipeline.warp_from_masks_ragged(dimgs, m24, (32, 44), return_batch=True)
    assert rb is not None
    for what in ("warped", "mota"):
        paths = [str(tmp_path / f"{what}_{i}.png") for i in range(4)]
        pipeline.save_png_ragged(rb, paths, what)
        for i, p in enumerate(paths):
            want = out[i].cpu().numpy() if what == "warped" else rb.mota_of(i).cpu().numpy()
            assert np.array_equal(np.asarray(Image.open(p)), want)
            same_bytes(open(p, "rb").read(), R.encode(want), p)
    over = pipeline.heatmap_overlay_ragged(rb)[1]
    from attwarp_amd import png
    for f, o in zip(png.encode_png(over, "up"), over):
        check_file(f, o.cpu().numpy(), "up", "rgb", "overlay view")
