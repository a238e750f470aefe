"""GPU tests of the JPEG decoder (attwarp_jpegdec_decode, attwarp_amd/jpeg.py): every pixel equals the restatement's
(tests/jpegdec_ref.py) and, for every file Pillow is the judge of, Pillow's; every status equals the restatement's; there
is no tolerance anywhere."""
import numpy as np
import pytest
import torch
from PIL import Image

import jpegdec_cases as C
import jpegdec_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = 256                                                    # guard bytes (the scratch buffer is 256-byte aligned)


def check_views(views, files, mode, order="rgb", pillow=True):
    for (name, f), v in zip(files, views):
        st, want, _ = D.decode(f, mode, order)
        got = v.cpu().numpy()
        assert st == D.OK and got.shape == want.shape and np.array_equal(got, want), (name, mode, order)
        if pillow:
            p = C.pillow(f, mode)
            assert np.array_equal(got, p[:, :, ::-1] if order == "bgr" and p.shape[2] == 3 else p), (name, mode, order)


def back_to_back(views, buffer):
    off = buffer.data_ptr()
    for v in views:
        assert v.is_contiguous() and v.data_ptr() == off
        off += v.numel()


@pytest.mark.parametrize("mode,order", [("RGB", "rgb"), ("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr")])
def test_whole_corpus_in_one_call(mode, order):
    from attwarp_amd import jpeg
    files = C.good()
    jf = jpeg.JpegFiles([f for _, f in files], mode, order, device=DEV)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    back_to_back(views, jf.buffer)
    check_views(views, files, mode, order)
    want = [D.decode(f)[2]["nunits"] for _, f in files]
    assert jf.units() == want and [r + 1 for r in jf.restarts()] == want and max(want) > 8


def test_malformed_files_among_good_ones_and_guard_bytes():
    from attwarp_amd import jpeg
    bad = C.malformed()
    good = [(n, C.good_file(n)) for n in ("ri_wrap", "noise_64x48_s1", "grey_17x15", "edge_40x31_s2")]
    files = []
    for i, (name, f, _) in enumerate(bad):                   # good files at the start, in between and at the end
        if i % 5 == 0:
            files.append(good[(i // 5) % len(good)])
        files.append((name, f))
    files.append(good[3])
    want = [D.decode(f)[0] for _, f in files]
    assert sum(w != 0 for w in want) >= 15
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV)
    out = torch.full((jf.out_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    scr = torch.full((jf.scratch.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    jf.buffer, jf.scratch = out[G:G + jf.out_bytes], scr[G:G + jf.scratch.numel()]
    views, status = jf.run()
    got = status.cpu().tolist()
    assert [D.STATUS_NAMES[s] for s in got] == [D.STATUS_NAMES[s] for s in want]
    for t in (out, scr):
        assert bool((t[:G] == 0xA5).all()) and bool((t[-G:] == 0xA5).all())
    back_to_back(views, jf.buffer)
    ok = [(nf, v) for nf, v, s in zip(files, views, got) if s == 0]
    hostile = {n for n, _, w in bad if w == 0}
    check_views([v for nf, v in ok if nf[0] not in hostile], [nf for nf, _ in ok if nf[0] not in hostile], "RGB")
    check_views([v for nf, v in ok if nf[0] in hostile], [nf for nf, _ in ok if nf[0] in hostile], "RGB", pillow=False)
    assert len([1 for nf, _ in ok if nf[0] in hostile]) == len(hostile) == 3
    # the same batch with the failing files' blocks pre-filled differently: nothing outside them depends on it
    first = out.clone()
    for v, s in zip(views, got):
        if s:
            v.fill_(0x3C)
    jf.run()
    off = 0
    a, b = first[G:G + jf.out_bytes], jf.buffer
    for (H, W, Cn), s in zip(jf.shapes, got):
        if s == 0:
            assert torch.equal(a[off:off + H * W * Cn], b[off:off + H * W * Cn])
        off += H * W * Cn
    first_bad = next(i for i, s in enumerate(want) if s)
    with pytest.raises(OSError, match=rf"file {first_bad} .*{D.STATUS_NAMES[want[first_bad]]}"):
        jpeg.decode_jpeg([f for _, f in files], device=DEV)


def test_two_runs_and_a_non_default_stream_give_the_same_bytes():
    from attwarp_amd import jpeg
    files = [(n, C.good_file(n)) for n in ("ri_wrap", "big_200x136", "q100_optimize", "ri_stuffed_end", "edge_2x1_s2")]
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV)
    views, status = jf.run()
    first = jf.buffer.clone()
    assert status.cpu().tolist() == [0] * len(files)
    check_views(views, files, "RGB")
    jf.buffer.fill_(0x5A)
    jf.run()
    assert torch.equal(jf.buffer, first)
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    jf.buffer.fill_(0x5A)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _, status = jf.run()
        s.synchronize()
    assert status.cpu().tolist() == [0] * len(files) and torch.equal(jf.buffer, first)


def test_run_is_capturable():
    from attwarp_amd import jpeg
    files = [(n, C.good_file(n)) for n in ("ri_wrap", "noise_17x33_s2", "grey_64x48_q100")]
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        jf.run()                                                         # (warm-up outside the capture)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            jf.run()
        jf.buffer.zero_()
        jf.status.fill_(-1)
        g.replay()
        s.synchronize()
    assert jf.status.cpu().tolist() == [0] * len(files)
    check_views(jf.views(), files, "RGB")


def test_mixed_png_and_jpeg_files_and_the_consumers(tmp_path):
    from attwarp_amd import dataloader, jpeg, pipeline
    imgs = [C.smooth_detail(61, 45, 1), C.noise(5, 7, 3, 2), C.smooth_detail(130, 111, 3), C.blocky(40, 64, 3, 4)]
    kinds = ("jpg", "png", "jpg", "png")
    paths = []
    for k, (im, kind) in enumerate(zip(imgs, kinds)):
        paths.append(tmp_path / f"{k}.{kind}")
        Image.fromarray(im).save(paths[-1], **({"quality": 85} if kind == "jpg" else {}))
    pil = [Image.open(p).convert("RGB") for p in paths]
    up = pipeline.upload_image_files(paths, device=DEV)
    ref = pipeline.upload_images(pil, device=DEV)
    assert len(up) == len(ref) and all(torch.equal(a, b) for a, b in zip(up, ref))
    with open(paths[0], "rb") as fh:
        data = fh.read()
    both = pipeline.upload_image_files([data, paths[1]], device=DEV)                  # bytes and paths alike
    assert torch.equal(both[0], ref[0]) and torch.equal(both[1], ref[1])
    with pytest.raises(ValueError, match="neither"):
        pipeline.upload_image_files([b"GIF89a" + bytes(20)], device=DEV)
    assert torch.equal(pipeline.clip_preprocess_ragged(up), pipeline.clip_preprocess_ragged(ref))
    assert torch.equal(dataloader.prepare_images(up, 64), dataloader.prepare_images(ref, 64))
    jp = [p for p, k in zip(paths, kinds) if k == "jpg"]
    assert all(torch.equal(a, b) for a, b in zip(jpeg.read_jpeg(jp, device=DEV), pipeline.upload_jpeg_files(jp, device=DEV)))
    assert torch.equal(jpeg.read_jpeg(jp, device=DEV)[1], ref[2])
