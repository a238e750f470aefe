"""GPU tests of the JPEG encoder (attwarp_jpegenc_encode, attwarp_amd/jpeg.py): every file equals the restatement of
tests/jpegenc_ref.py byte for byte (which tests/test_jpegenc_ref_cpu.py proves equal to Pillow's), and this project's own
decoder reads it back to Pillow's pixels."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpegenc_cases as K
import jpegenc_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def same_bytes(got: bytes, want: bytes, what):
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(f"{what}: {len(got)} bytes against the restatement's {len(want)}, first difference at byte {first}")


def keywords(cases):
    return dict(quality=[c[2].get("quality", 75) for c in cases], subsampling=[c[2].get("subsampling", "4:2:0") for c in cases],
                restart_rows=[c[2].get("restart_rows", 0) for c in cases], order=[c[2].get("order", "rgb") for c in cases])


@pytest.fixture(scope="module")
def corpus():
    """The whole corpus encoded in ONE JpegBatch."""
    from attwarp_amd import jpeg, png
    cases = K.cases()
    tens = [torch.from_numpy(c[1]).to(DEV) for c in cases]
    b = jpeg.JpegBatch(tens, **keywords(cases))
    files = png.download(*b.run())
    return cases, tens, b, files


def test_every_case_equals_the_restatement(corpus):
    cases, tens, b, files = corpus
    offs = b.offsets.cpu().numpy()
    assert offs[0] == 0 and (np.diff(offs) == [len(f) for f in files]).all() and offs[-1] <= b.bound
    assert b.bound == sum(R.bound(*(c[1].shape[:2]), 1 if c[1].ndim == 2 else 3, c[2].get("quality", 75), c[2].get("subsampling", "4:2:0"),
                                  c[2].get("restart_rows", 0)) for c in cases)
    assert b.units == sum(K.measure(c[0])["units"] for c in cases)
    for (name, *_), f in zip(cases, files):
        same_bytes(f, K.reference(name), name)


def test_own_decoder_reads_every_file_to_pillows_pixels(corpus):
    """Files with and without restart markers: the marker-less ones take the decoder's sub-stream route."""
    from attwarp_amd import jpeg
    cases, tens, b, files = corpus
    assert any(c[2].get("restart_rows", 0) for c in cases) and not all(c[2].get("restart_rows", 0) for c in cases)
    for f, t in zip(files, jpeg.decode_jpeg(files, "RGB", device=DEV)):
        assert np.array_equal(t.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB")))


def test_a_case_alone_first_last_and_in_the_middle(corpus):
    from attwarp_amd import jpeg
    cases, tens, b, files = corpus
    names = [c[0] for c in cases]
    others = [names.index(n) for n in ("33x47_4:2:0", "rst_wrap", "1x1_grey")]
    for name in ("24x40_4:2:0", "ff_before_rst", "unit_plus_mcu_32", "many_units"):
        i = names.index(name)
        for idx in ([i], [i] + others, others + [i], others[:2] + [i] + others[2:]):
            sub = [cases[k] for k in idx]
            got = jpeg.encode_jpeg([tens[k] for k in idx], **keywords(sub))
            for k, g in zip(idx, got):
                same_bytes(g, files[k], (name, idx))


def test_out_at_every_residue_between_guards(corpus):
    """``out`` starting at each residue mod 4 between guard bytes, the scratch buffer inside guards too: the guards and the bytes
    behind the last file stay as they were."""
    from attwarp_amd import jpeg, png
    cases, tens, b, files = corpus
    pick = [i for i, c in enumerate(cases) if c[0] in ("17x9_4:2:0", "ff_before_eoi", "many_units_444", "40x25_4:2:2", "rst_wrap_420")]
    sub = [cases[i] for i in pick]
    G = 64
    for r in range(4):
        probe = jpeg.JpegBatch([tens[i] for i in pick], **keywords(sub))
        store = torch.full((G + r + probe.bound + G,), 0xA5, dtype=torch.uint8, device=DEV)
        jb = jpeg.JpegBatch([tens[i] for i in pick], out=store[G + r:G + r + probe.bound], **keywords(sub))
        n = jb.scratch.numel()
        guarded = torch.full((256 + n + 256,), 0x5A, dtype=torch.uint8, device=DEV)
        jb.scratch = guarded[256:256 + n]
        assert jb.scratch.data_ptr() % 16 == 0
        got = png.download(*jb.run())
        for i, g in zip(pick, got):
            same_bytes(g, files[i], (cases[i][0], r))
        used = int(jb.offsets[-1])
        host = store.cpu().numpy()
        assert (host[:G + r] == 0xA5).all() and (host[G + r + used:] == 0xA5).all()
        gh = guarded.cpu().numpy()
        assert (gh[:256] == 0x5A).all() and (gh[256 + n:] == 0x5A).all()


def test_graph_replay_gives_the_same_bytes(corpus):
    from attwarp_amd import jpeg, png
    cases, tens, _, files = corpus
    pick = [i for i, c in enumerate(cases) if c[0] in ("33x47_4:2:0", "ff_many", "many_units", "16x16_grey", "rst_wrap")]
    mine = [tens[i].clone() for i in pick]
    sub = [cases[i] for i in pick]
    b = jpeg.JpegBatch(mine, **keywords(sub))
    b.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.run()
    b.buffer.zero_()
    b.offsets.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert png.download(b.buffer, b.offsets) == [files[i] for i in pick]
    flipped = np.ascontiguousarray(cases[pick[2]][1][::-1])                     # the sources are read at every replay
    mine[2].copy_(torch.from_numpy(flipped))
    g.replay()
    torch.cuda.synchronize()
    got = png.download(b.buffer, b.offsets)
    assert got[2] == R.encode(flipped, **sub[2][2]) and got[:2] == [files[i] for i in pick[:2]] and got[3:] == [files[i] for i in pick[3:]]


def test_sources_orders_addresses_pitch_views_and_input_forms():
    from attwarp_amd import jpeg
    img = K.photo(19, 27, 3, 2)
    H, W, C = img.shape
    pitch = W * C + 6
    flat = torch.zeros(3 + H * pitch, dtype=torch.uint8, device=DEV)
    view = flat[3:].as_strided((H, W, C), (pitch, C, 1))                      # odd byte address, rows 87 bytes apart
    view.copy_(torch.from_numpy(img))
    assert view.data_ptr() % 2 == 1 and pitch % 4 != 0 and not view.is_contiguous()
    grey = K.photo(11, 13, 1, 3)
    wide = torch.from_numpy(np.ascontiguousarray(np.pad(grey, ((0, 0), (2, 4))))).to(DEV)
    big = torch.from_numpy(K.photo(40, 50, 3, 4)).to(DEV)
    files = jpeg.encode_jpeg([view, wide[:, 2:15], torch.from_numpy(grey[:, :, None].copy()).to(DEV), big[5:30, 7:40]], quality=90)
    same_bytes(files[0], R.encode(img, 90), "odd address and pitch")
    same_bytes(files[1], R.encode(grey, 90), "[H,W] slice of a wider tensor")
    assert files[2] == files[1]                                               # [H,W,1]
    same_bytes(files[3], R.encode(big.cpu().numpy()[5:30, 7:40], 90), "a view into a larger image")
    t = torch.from_numpy(img).to(DEV)
    flipped = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1])).to(DEV)
    for sub in jpeg.SUBSAMPLINGS:
        assert jpeg.encode_jpeg([t], 75, sub, order="bgr") == jpeg.encode_jpeg([flipped], 75, sub)
        assert jpeg.encode_jpeg([t], 75, R.SUBSAMPLING_IDS[sub]) == jpeg.encode_jpeg([t], 75, sub)          # Pillow's numbers
    dense = np.stack([K.photo(9, 14, 3, s) for s in range(3)])
    for f, im in zip(jpeg.encode_jpeg(torch.from_numpy(dense).to(DEV)), dense):   # one [B,H,W,C] tensor, a bare call
        g = io.BytesIO()
        Image.fromarray(im).save(g, "JPEG")
        same_bytes(f, g.getvalue(), "dense batch against a bare Image.save")


def test_limits_raise_before_any_launch():
    from attwarp_amd import jpeg
    ok = torch.zeros(8, 16, 3, dtype=torch.uint8, device=DEV)
    for bad in (dict(quality=0), dict(quality=101), dict(quality=75.0), dict(subsampling="4:1:1"), dict(subsampling=3), dict(restart_rows=-1),
                dict(order="gbr"), dict(quality=[75, 80])):
        with pytest.raises(ValueError):
            jpeg.JpegBatch([ok], **bad)
    for t in (torch.zeros(4, 6, 2, dtype=torch.uint8, device=DEV), torch.zeros(0, 6, 3, dtype=torch.uint8, device=DEV),
              torch.zeros(4, 12, 3, dtype=torch.uint8, device=DEV)[:, ::2], torch.zeros(4, 3, 6, dtype=torch.uint8, device=DEV).permute(0, 2, 1),
              torch.zeros(4, 6, 3, dtype=torch.int16, device=DEV), torch.zeros(2, jpeg.JPEGENC_MAX_DIM + 1, dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            jpeg.JpegBatch([t])
    row = torch.zeros(1, jpeg.JPEGENC_MAX_DIM, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        jpeg.JpegBatch([row], restart_rows=9)                                  # 9 x 8188 MCUs > 65535
    same_bytes(jpeg.encode_jpeg([row], restart_rows=8)[0], R.encode(np.zeros((1, jpeg.JPEGENC_MAX_DIM), np.uint8), restart_rows=8), "widest row")
    with pytest.raises(ValueError):
        jpeg.JpegBatch([ok], out=torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        jpeg.JpegBatch([])


def _att(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.random((h, w)).astype(np.float32) ** 3
    a[h // 3: h // 2, w // 4: w // 2] += 2.0
    return a


def test_save_warped_image_jpg_paths_write_pillows_bytes(tmp_path):
    from attwarp_amd import new_method as nm
    pil = Image.fromarray(K.photo(37, 52, 3, 20))
    att = _att(37, 52, 0)
    names = {e: [str(tmp_path / f"{e}_{n}") for n in ("orig.JPG", "overlay.png", "warped.jpeg")] for e in ("pillow", "hip")}
    assert nm.save_warped_image(pil, att, *names["pillow"], width=48, height=40, transform="sqrt", encoder="pillow")
    assert nm.save_warped_image(pil, att, *names["hip"], width=48, height=40, transform="sqrt", encoder="hip")
    allpng = [str(tmp_path / f"png_{n}.png") for n in ("orig", "overlay", "warped")]      # the same call with PNG paths only
    assert nm.save_warped_image(pil, att, *allpng, width=48, height=40, transform="sqrt", encoder="hip")
    for p, h, q in zip(names["pillow"], names["hip"], allpng):
        a, b = open(p, "rb").read(), open(h, "rb").read()
        if p.endswith(".png"):                                                # the PNG batch is unchanged: the bytes of an all-PNG call
            assert b[:8] == b"\x89PNG\r\n\x1a\n" and b == open(q, "rb").read()
            assert np.array_equal(np.asarray(Image.open(p)), np.asarray(Image.open(h)))
        else:
            same_bytes(b, a, h)
            assert b[:2] == b"\xff\xd8"
    assert nm.save_warped_image(pil, att, None, None, str(tmp_path / "only.jpg"), width=48, height=40, encoder="hip")
    assert nm.save_warped_image(pil, att, None, None, str(tmp_path / "only_p.jpg"), width=48, height=40, encoder="pillow")
    assert open(tmp_path / "only.jpg", "rb").read() == open(tmp_path / "only_p.jpg", "rb").read()


def test_save_jpeg_ragged(tmp_path):
    from attwarp_amd import pipeline
    rng = np.random.default_rng(31)
    sizes = [(40, 50), (33, 61), (64, 48), (57, 35)]
    imgs = [K.photo(h, w, 3, 40 + i) for i, (h, w) in enumerate(sizes)]
    dimgs = pipeline.upload_images(imgs, DEV)
    m24 = torch.from_numpy((rng.random((4, 24, 24), dtype=np.float32) ** 3)).to(DEV)
    out, rb = pipeline.warp_from_masks_ragged(dimgs, m24, (32, 44), return_batch=True)
    assert rb is not None
    for what, kw in (("warped", {}), ("mota", dict(quality=90, restart_rows=1)), ("warped", dict(subsampling="4:4:4", order="bgr"))):
        paths = [str(tmp_path / f"{what}_{i}.jpg") for i in range(4)]
        pipeline.save_jpeg_ragged(rb, paths, what, **kw)
        for i, p in enumerate(paths):
            want = out[i].cpu().numpy() if what == "warped" else rb.mota_of(i).cpu().numpy()
            same_bytes(open(p, "rb").read(), R.encode(want, **kw), p)
