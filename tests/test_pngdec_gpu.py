"""GPU tests of the PNG decoder (attwarp_pngdec_decode, attwarp_amd/png.py): every pixel equals Pillow's, every status the
restatement's (tests/pngdec_ref.py); there is no tolerance anywhere."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as PC
import pngdec_cases as C
import pngdec_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def check_views(views, files, mode, order="rgb"):
    for (name, f), v in zip(files, views):
        want = C.pillow(f, mode)
        if order == "bgr":
            want = want[:, :, ::-1]
        got = v.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (name, mode, order)


def back_to_back(views, buffer):
    off = buffer.data_ptr()
    for v in views:
        assert v.is_contiguous() and v.data_ptr() == off
        off += v.numel()


@pytest.mark.parametrize("mode,order", [("RGB", "rgb"), ("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr")])
def test_whole_corpus_in_one_call(mode, order):
    from attwarp_amd import png
    files = C.good()
    pf = png.PngFiles([f for _, f in files], mode, order, device=DEV)
    views, status = pf.run()
    assert status.cpu().tolist() == [0] * len(files)
    back_to_back(views, pf.buffer)
    check_views(views, files, mode, order)
    # the route every file took, its chain and the sync points kept: pixels alone cannot tell a silent serial fallback
    got, want = pf.routes(), C.routes()
    assert got == want, [(n, g, w) for (n, _), g, w in zip(files, got, want) if g != w]
    assert sum(r[0] == 0 for r in want) > 40 and max(r[2] for r in want) == png.PNGDEC_MAX_UNITS


def test_unit_route_equals_serial_route_and_two_runs_agree():
    from attwarp_amd import _lib, png
    names = ("own_500_sub", "photo_full_flush_one", "false_sync", "photo_sync_flush_idat7")
    files = [(n, C.good_file(n)) for n in names]
    pf = png.PngFiles([f for _, f in files], device=DEV)
    views, status = pf.run()
    first = pf.buffer.clone()
    assert status.cpu().tolist() == [0] * len(files)
    check_views(views, files, "RGB")
    # 32 segments + the final block on the chain, one more position kept in front of the Adler-32; two independent halves;
    # the false candidate never arrived at; the dependent second half sent down the serial route
    assert pf.routes() == [(0, 33, 34), (0, 2, 2), (0, 1, 2), (1, 0, 2)]
    pf.buffer.fill_(0x5A)
    pf.run()
    assert torch.equal(pf.buffer, first)                                 # run() twice: the same bytes
    pf.buffer.fill_(0x5A)
    with _lib.debug_override(pngdec_route=1):                            # every image from the start, one wave
        _, status = pf.run()
    assert status.cpu().tolist() == [0] * len(files) and torch.equal(pf.buffer, first)
    assert pf.routes() == [(1, 0, 34), (1, 0, 2), (1, 0, 2), (1, 0, 2)]


def test_malformed_files_among_good_ones_and_guard_bytes():
    from attwarp_amd import png
    bad = C.malformed()
    good = [(n, C.good_file(n)) for n in ("own_500_sub", "photo_level9_idat1", "pil_RGBA_opt", "photo_full_flush_one")]
    files, want = [], []
    for i, (name, f, _) in enumerate(bad):                               # good files at the start, in between and at the end
        if i % 6 == 0:
            files.append(good[(i // 6) % len(good)])
            want.append(0)
        files.append((name, f))
        want.append(D.decode(f)[0])
    files.append(good[3])
    want.append(0)
    assert all(w != 0 for (n, _), w in zip(files, want) if n in {b[0] for b in bad})
    pf = png.PngFiles([f for _, f in files], device=DEV)
    G = 64
    out = torch.full((pf.out_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    scr = torch.full((pf.scratch.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    pf.buffer, pf.scratch = out[G:G + pf.out_bytes], scr[G:G + pf.scratch.numel()]
    views, status = pf.run()
    got = status.cpu().tolist()
    assert [D.STATUS_NAMES[s] for s in got] == [D.STATUS_NAMES[s] for s in want]
    for t in (out, scr):
        assert bool((t[:G] == 0xA5).all()) and bool((t[-G:] == 0xA5).all())
    back_to_back(views, pf.buffer)
    ok = [(nf, v) for nf, v, s in zip(files, views, got) if s == 0]
    check_views([v for _, v in ok], [nf for nf, _ in ok], "RGB")
    first_bad = next(i for i, s in enumerate(want) if s)
    with pytest.raises(OSError, match=rf"file {first_bad} .*{D.STATUS_NAMES[want[first_bad]]}"):
        png.decode_png([f for _, f in files], device=DEV)
    crc = next(f for n, f, _ in bad if n == "wrong_crc")                 # the same file with the check off
    _, st = png.PngFiles([crc], check_crc=False, device=DEV).run()
    assert st.cpu().tolist() == [0]


def test_round_trip_with_the_encoder_on_the_device():
    from attwarp_amd import png
    src = [torch.from_numpy(i).to(DEV) for i in PC.ragged_batch()]
    files = png.download(*png.PngBatch(src).run())
    back = png.decode_png(files, mode="keep", device=DEV)
    assert all(torch.equal(a, b) for a, b in zip(src, back))            # compared where they are: no pixel comes down


def test_consumers_take_the_views(tmp_path):
    from attwarp_amd import dataloader, pipeline
    imgs = [PC.photo(5, 7, 3, 1), PC.photo(61, 45, 3, 2), PC.photo(130, 211, 3, 3)]
    pil = [Image.fromarray(i) for i in imgs]
    paths = []
    for k, im in enumerate(pil):
        paths.append(tmp_path / f"{k}.png")
        im.save(paths[-1])
    up = pipeline.upload_png_files(paths, device=DEV)
    assert [tuple(u.shape) for u in up] == [i.shape for i in imgs]
    assert torch.equal(pipeline.clip_preprocess_ragged(up), pipeline.clip_preprocess_ragged(pil))
    assert torch.equal(dataloader.prepare_images(up, 64), dataloader.prepare_images(pil, 64))
    from attwarp_amd import png
    assert all(torch.equal(a, b) for a, b in zip(png.read_png(paths, device=DEV), up))


def test_run_is_capturable():
    from attwarp_amd import png
    files = [(n, C.good_file(n)) for n in ("own_500_sub", "photo_rle1_one")]
    pf = png.PngFiles([f for _, f in files], device=DEV)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        pf.run()                                                         # (warm-up outside the capture)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            pf.run()
        pf.buffer.zero_()
        g.replay()
        s.synchronize()
    check_views(pf.views(), files, "RGB")
