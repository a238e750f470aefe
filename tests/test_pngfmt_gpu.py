"""GPU tests of the PNG decoder's formats path (all_formats=True: palette, 1 / 2 / 4 / 16 bits, Adam7): every
pixel equals Pillow's, every status the restatement's (tests/pngfmt_ref.py); there is no tolerance anywhere."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as PC
import pngdec_cases as DC
import pngdec_ref as D
import pngfmt_cases as C
import pngfmt_ref as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def wanted():
    """{(name, mode): Pillow's pixels} of the corpus, computed once."""
    return {(k.name, m): C.pillow(k.file, m) for k in C.good() for m in ("RGB", "L", "keep")}


def check_views(views, cases, mode, order, wanted):
    for k, v in zip(cases, views):
        want = wanted[(k.name, mode)]
        if order == "bgr" and want.shape[2] == 3:
            want = want[:, :, ::-1]
        got = v.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (k.name, mode, order)


@pytest.mark.parametrize("mode,order", [("RGB", "rgb"), ("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr"), ("keep", "bgr")])
def test_whole_corpus_in_one_call(mode, order, wanted):
    from attwarp_amd import png
    cases = C.good()
    pf = png.PngFiles([k.file for k in cases], mode, order, device=DEV, all_formats=True)
    assert pf.header.formats == 1
    views, status = pf.run()
    assert status.cpu().tolist() == [0] * len(cases)
    off = pf.buffer.data_ptr()
    for v in views:
        assert v.is_contiguous() and v.data_ptr() == off
        off += v.numel()
    check_views(views, cases, mode, order, wanted)
    assert all(r[0] in (0, 1) for r in pf.routes()) and len(pf.kept()) == len(cases)


def test_malformed_files_among_good_ones_and_guard_bytes(wanted):
    from attwarp_amd import png
    bad = C.malformed() + [(n, f) for n, f, _ in DC.malformed() if n in ("wrong_adler", "wrong_crc", "filter5")]
    good = [k for k in C.small_good() if k.name in ("adam7_rgb8_9x9", "palette_boundary_adam7", "carry_grey1_h129", "grey16_values")]
    names, files, want = [], [], []
    for i, (name, f) in enumerate(bad):                                   # good files at the start, in between and at the end
        if i % 3 == 0:
            k = good[(i // 3) % len(good)]
            names.append(k.name); files.append(k.file); want.append(0)
        names.append(name); files.append(f); want.append(F.decode(f)[0])
    names.append(good[3].name); files.append(good[3].file); want.append(0)
    assert sum(w != 0 for w in want) == len(bad) and {D.STATUS_NAMES[w] for w in want} >= {"E_FILTER", "E_UNDERFLOW", "E_OVERFLOW", "E_TRUNCATED",
                                                                                          "E_ADLER", "E_CRC"}
    pf = png.PngFiles(files, device=DEV, all_formats=True)
    G = 64
    out = torch.full((pf.out_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    scr = torch.full((pf.scratch.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    pf.buffer, pf.scratch = out[G:G + pf.out_bytes], scr[G:G + pf.scratch.numel()]
    views, status = pf.run()
    got = status.cpu().tolist()
    assert [D.STATUS_NAMES[s] for s in got] == [D.STATUS_NAMES[s] for s in want]
    for t in (out, scr):
        assert bool((t[:G] == 0xA5).all()) and bool((t[-G:] == 0xA5).all())
    for n, v, s in zip(names, views, got):
        if s == 0:
            assert np.array_equal(v.cpu().numpy(), wanted[(n, "RGB")]), n
    first_bad = next(i for i, s in enumerate(want) if s)
    with pytest.raises(OSError, match=rf"file {first_bad} .*{D.STATUS_NAMES[want[first_bad]]}"):
        png.decode_png(files, device=DEV, all_formats=True)


def test_new_kernel_equals_the_old_one_on_the_plain_corpus():
    from attwarp_amd import png
    plain = [f for _, f in DC.good()]
    for mode, order in (("RGB", "rgb"), ("L", "rgb"), ("keep", "bgr")):
        alone = png.PngFiles(plain, mode, order, device=DEV, all_formats=True)
        assert alone.header.formats == 0
        a, sa = alone.run()
        mixed = png.PngFiles(plain + [C.pillow_written()[1].file], mode, order, device=DEV, all_formats=True)
        assert mixed.header.formats == 1
        b, sb = mixed.run()
        assert sa.cpu().tolist() == [0] * len(plain) and sb.cpu().tolist() == [0] * (len(plain) + 1)
        assert torch.equal(alone.buffer[:alone.out_bytes], mixed.buffer[:alone.out_bytes])
        assert alone.routes() == mixed.routes()[:len(plain)]


def test_plain_files_with_the_keyword_take_the_parents_table():
    from attwarp_amd import png
    plain = [f for _, f in DC.good()]
    a = png.PngFiles(plain, "RGB", "bgr", device=DEV, all_formats=True)
    b = png.PngFiles(plain, "RGB", "bgr", device=DEV)
    assert a.table_host.tobytes() == b.table_host.tobytes() and a.header.formats == 0
    assert torch.equal(a.run()[0][7], b.run()[0][7]) and torch.equal(a.buffer, b.buffer)


def test_mixed_png_and_jpeg_list_comes_back_in_input_order():
    from attwarp_amd import pipeline
    pngs = [k for k in C.small_good() if k.name in ("pil_P_bits4", "adam7_rgba16_9x9", "pil_1", "tail_d2_c3_w7")]
    jpgs = []
    for seed in (1, 2):
        buf = io.BytesIO()
        Image.fromarray(PC.photo(24 + seed, 40, 3, seed)).save(buf, "JPEG", quality=90)
        jpgs.append(buf.getvalue())
    files = [pngs[0].file, jpgs[0], pngs[1].file, pngs[2].file, jpgs[1], pngs[3].file, DC.good_file("geo_rgba")]
    got = pipeline.upload_image_files(files, device=DEV, all_formats=True)
    for f, v in zip(files, got):
        want = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        assert np.array_equal(v.cpu().numpy(), want)
    with pytest.raises(ValueError, match="file 0: bit depth"):             # (the first PNG of the list has 16 bits)
        pipeline.upload_image_files(files, device=DEV)


def test_two_runs_a_side_stream_and_a_replayed_graph_give_the_same_bytes(wanted):
    from attwarp_amd import png
    cases = [k for k in C.small_good() if k.name in ("carry_adam7_9x521", "palette_boundary", "carry_rgba16_h129", "adam7_grey1_9x9",
                                                      "pil_I16", "rgb16_photo_idat7", "tail_d1_c0_w17")]
    assert len(cases) == 7
    pf = png.PngFiles([k.file for k in cases], device=DEV, all_formats=True)
    views, status = pf.run()
    assert status.cpu().tolist() == [0] * len(cases)
    check_views(views, cases, "RGB", "rgb", wanted)
    first = pf.buffer.clone()
    pf.buffer.fill_(0x5A)
    pf.run()
    assert torch.equal(pf.buffer, first)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        pf.buffer.fill_(0x5A)
        pf.run()
        s.synchronize()
        assert torch.equal(pf.buffer, first)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            pf.run()
        for _ in range(2):
            pf.buffer.fill_(0x5A)
            pf.status.fill_(-1)
            g.replay()
            s.synchronize()
            assert torch.equal(pf.buffer, first) and pf.status.cpu().tolist() == [0] * len(cases)


def test_consumers_take_the_views(tmp_path):
    from attwarp_amd import dataloader, pipeline, png
    rng = np.random.default_rng(5)
    pal = Image.frombytes("P", (45, 61), rng.integers(0, 16, (61, 45), dtype=np.uint8).tobytes())
    pal.putpalette(C.random_palette(16, 1).tobytes())
    bilevel = Image.fromarray(rng.integers(0, 2, (130, 211), dtype=np.uint8) * 255).convert("1")
    deep = Image.fromarray(rng.integers(0, 300, (17, 23), dtype=np.uint16))
    paths, pil = [], []
    for k, (im, kw) in enumerate(((pal, dict(bits=4)), (bilevel, {}), (deep, {}))):
        paths.append(tmp_path / f"{k}.png")
        im.save(paths[-1], **kw)
        pil.append(Image.open(paths[-1]).convert("RGB"))
    up = pipeline.upload_png_files(paths, device=DEV, all_formats=True)
    assert [tuple(u.shape) for u in up] == [(61, 45, 3), (130, 211, 3), (17, 23, 3)]
    assert torch.equal(pipeline.clip_preprocess_ragged(up), pipeline.clip_preprocess_ragged(pil))
    assert torch.equal(dataloader.prepare_images(up, 64), dataloader.prepare_images(pil, 64))
    assert all(torch.equal(a, b) for a, b in zip(png.read_png(paths, device=DEV, all_formats=True), up))


def test_without_the_keyword_the_files_still_raise():
    from attwarp_amd import pipeline, png
    byname = {k.name: k.file for k in C.small_good()}
    for name, word in (("palette_boundary", "colour type"), ("adam7_rgb8_3x3", "interlace"), ("pil_1", "depth"), ("grey16_values", "depth")):
        for call in (lambda f: png.PngFiles([f], device=DEV), lambda f: png.decode_png([f], device=DEV),
                     lambda f: pipeline.upload_png_files([f], device=DEV), lambda f: pipeline.upload_image_files([f], device=DEV)):
            with pytest.raises(ValueError, match=word):
                call(byname[name])
