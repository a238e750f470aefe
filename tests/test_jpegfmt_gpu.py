"""GPU tests of the JPEG decoder's layout family (``all_layouts=True``: attwarp_jpegdec_decode_layouts, attwarp_amd/jpeg.py,
DESIGN.md 3.19): every pixel of every file equals Pillow's and the restatement's (tests/jpegfmt_ref.py, pinned to Pillow on
the CPU), every status equals the restatement's, by every route; there is no tolerance anywhere."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpegdec_cases as C
import jpegdec_ref as D
import jpegfmt_cases as F
import jpegfmt_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = 256                                                    # guard bytes (the scratch buffer is 256-byte aligned)
MODES = [(m, o) for m in ("RGB", "L", "keep") for o in ("rgb", "bgr")]


def check_views(views, files, mode, order="rgb"):
    for (name, f), v in zip(files, views):
        st, want, _ = R.decode(f, mode, order)
        got = v.cpu().numpy()
        assert st == D.OK and got.shape == want.shape and np.array_equal(got, want), (name, mode, order)
        p = R.pillow(f, mode)
        assert np.array_equal(got, p[:, :, ::-1] if order == "bgr" and p.shape[2] == 3 else p), (name, mode, order)


def back_to_back(views, buffer):
    off = buffer.data_ptr()
    for v in views:
        assert v.is_contiguous() and v.data_ptr() == off
        off += v.numel()


@pytest.mark.parametrize("mode,order", MODES)
def test_whole_corpus_in_one_call(mode, order):
    from attwarp_amd import jpeg
    files = F.good()
    jf = jpeg.JpegFiles([f for _, f in files], mode, order, device=DEV, all_layouts=True)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    check_views(views, files, mode, order)
    assert jf.parts is not None and sorted(i for idx, _ in jf.parts for i in idx) == list(range(len(files)))   # (plain files among them)
    layouts = [part for _, part in jf.parts if part.all_layouts]
    assert len(layouts) == 1 and len(jf.parts) == 2
    back_to_back(layouts[0].views(), layouts[0].buffer)
    want = [R.decode(f)[2]["nunits"] for _, f in files]
    assert jf.units() == want and [r + 1 for r in jf.restarts()] == want and max(want) > 8
    if (mode, order) == ("RGB", "rgb"):                       # the one-call entry points give the same tensors
        again = jpeg.decode_jpeg([f for _, f in files], device=DEV, all_layouts=True)
        assert all(torch.equal(a, b) for a, b in zip(again, views))


def _routes(files, mode="keep", **kw):
    from attwarp_amd import jpeg
    out = {}
    for route, args in (("substreams", dict(substreams="auto")), ("sequential", dict(substreams=False)),
                        ("short segments", dict(substreams=True, segment_bytes=32, max_rounds=4096))):
        jf = jpeg.JpegFiles([f for _, f in files], mode, device=DEV, all_layouts=True, **args, **kw)
        views, status = jf.run()
        out[route] = (jf, [v.cpu().numpy() for v in views], status.cpu().tolist())
    return out


def test_substreams_sequential_and_restart_routes_agree():
    from attwarp_amd import jpeg
    files = F.long_plain() + [(n, F.good_file(n)) for n in ("coef_410_67x37", "cmyk_s1_33x20", "edit_1x4_16x128", "coef_cmyk_c1x2_35x37")]
    files = [nf for nf in files if R.parse(nf[1])["color"] != "ycc" or R.parse(nf[1])["samp"][0] not in ((1, 1), (2, 1), (2, 2))]
    routes = _routes(files)
    for route, (jf, views, status) in routes.items():
        assert status == [0] * len(files), route
        assert jf.all_layouts and jf.parts is None
        for (name, f), got in zip(files, views):
            assert np.array_equal(got, R.pillow(f, "keep")), (route, name)
    info = routes["substreams"][0].substream_info()
    for (name, _), (nseg, rounds, accepted), planned in zip(files, info, routes["substreams"][0].substreams()):
        assert nseg == planned and (accepted == 1 and rounds >= 1 if name.startswith("long_") else True), (name, nseg, rounds, accepted)
    assert all(i[0] >= 4 for i, (n, _) in zip(info, files) if n.startswith("long_"))
    # the rounds do not grow with the segments, not even where all components share their tables (Pillow's CMYK: 38 segments)
    assert max(i[0] for i in info) >= 36 and all(i[1] <= 12 for i in info), info
    assert all(i == (0, 0, 0) for i in routes["sequential"][0].substream_info())
    short = routes["short segments"][0].substream_info()
    assert all(a == 1 for (_, _, a), (n, _) in zip(short, files) if n.startswith("long_")) and max(s[0] for s in short) > 200
    # the restart route: the same pictures' layouts written with a marker per MCU row or per MCU decode as Pillow decodes them
    rst = [(n, f) for n, f in F.good() if "_ri_" in n and "layout" in jpeg.parse_jpeg(f, 0, all_layouts=True)]
    assert len(rst) >= 30
    for route, (jf, views, status) in _routes(rst, "RGB").items():
        assert status == [0] * len(rst) and max(jf.units()) >= 6 and jf.substreams() == [0] * len(rst), route
        for (name, f), got in zip(rst, views):
            assert np.array_equal(got, R.pillow(f, "RGB")), (route, name)


def test_malformed_files_among_good_ones_and_guard_bytes():
    from attwarp_amd import jpeg
    bad = F.malformed()
    good = [(n, F.good_file(n)) for n in ("long_cmyk_s2", "coef_410_ri_1", "edit_440_8x16", "coef_ycck_y2x2_1x1")]
    files = []
    for i, (name, f) in enumerate(bad):                      # good files at the start, in between and at the end
        if i % 5 == 0:
            files.append(good[(i // 5) % len(good)])
        files.append((name, f))
    files.append(good[3])
    want = [R.decode(f)[0] for _, f in files]
    assert sum(w != 0 for w in want) >= 25 and set(want) >= {D.OK, D.E_TRUNCATED, D.E_HUFFMAN, D.E_RESTART, D.E_NO_EOI}
    firsts = []
    for args in (dict(), dict(substreams=False), dict(substreams=True, segment_bytes=64)):
        jf = jpeg.JpegFiles([f for _, f in files], device=DEV, all_layouts=True, **args)
        assert jf.all_layouts and jf.parts is None
        out = torch.full((jf.out_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
        scr = torch.full((jf.scratch.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
        jf.buffer, jf.scratch = out[G:G + jf.out_bytes], scr[G:G + jf.scratch.numel()]
        views, status = jf.run()
        got = status.cpu().tolist()
        assert [D.STATUS_NAMES[s] for s in got] == [D.STATUS_NAMES[s] for s in want], args
        for t in (out, scr):
            assert bool((t[:G] == 0xA5).all()) and bool((t[-G:] == 0xA5).all())
        back_to_back(views, jf.buffer)
        ok = [(nf, v) for nf, v, s in zip(files, views, got) if s == 0]
        check_views([v for _, v in ok], [nf for nf, _ in ok], "RGB")
        firsts.append((jf, views, got, out.clone()))
    # the same batch with the failing files' blocks pre-filled differently: nothing outside them depends on it
    jf, views, got, first = firsts[0]
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
        jpeg.decode_jpeg([f for _, f in files], device=DEV, all_layouts=True)


def test_a_mixed_list_comes_back_in_input_order(tmp_path):
    from attwarp_amd import jpeg, pipeline
    import jpegprog_cases as P
    png = io.BytesIO()
    Image.fromarray(C.noise(21, 13, 3, 40)).save(png, "PNG")
    prog = P.good()[0][1]
    files = [F.good_file("long_cmyk_s2"), C.good_file("noise_17x33_s2"), png.getvalue(), prog, F.good_file("coef_410_33x17"),
             C.good_file("grey_17x15"), F.good_file("keep_rgb_23x19"), C.good_file("ri_wrap"), F.good_file("edit_ycck_s2"), prog]
    want = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
    up = pipeline.upload_image_files(files, device=DEV, progressive=True, all_layouts=True)
    assert len(up) == len(want) and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(up, want))
    jpegs = [f for f in files if f is not files[2]]
    for mode in ("RGB", "L", "keep"):
        jf = jpeg.JpegFiles(jpegs, mode, device=DEV, progressive=True, all_layouts=True)
        views, status = jf.run()
        assert len(jf.parts) == 3 and status.cpu().tolist() == [0] * len(jpegs)
        assert [tuple(v.shape) for v in views] == jf.shapes and [s[2] for s in jf.shapes] == ([3] * 9 if mode == "RGB" else [1] * 9 if mode == "L" else
                                                                                             [4, 3, 3, 3, 1, 3, 3, 4, 3])
        for f, v in zip(jpegs, views):
            assert np.array_equal(v.cpu().numpy(), R.pillow(f, mode))
    paths = []
    for k, f in enumerate(jpegs[:5]):
        paths.append(tmp_path / f"{k}.jpg")
        paths[-1].write_bytes(f)
    rd = jpeg.read_jpeg(paths, device=DEV, progressive=True, all_layouts=True)
    up = pipeline.upload_jpeg_files(paths, device=DEV, progressive=True, all_layouts=True)
    assert all(torch.equal(a, b) for a, b in zip(rd, up)) and all(np.array_equal(a.cpu().numpy(), R.pillow(f)) for a, f in zip(rd, jpegs))
    with pytest.raises(ValueError, match="out must be None"):
        jpeg.JpegFiles(jpegs, device=DEV, progressive=True, all_layouts=True, out=torch.empty(1 << 20, dtype=torch.uint8, device=DEV))


def test_plain_lists_take_the_parents_path_and_the_keyword_is_needed():
    from attwarp_amd import jpeg
    files = [(n, C.good_file(n)) for n in ("ri_wrap", "noise_64x48_s1", "grey_17x15", "big_200x136")]
    a = jpeg.JpegFiles([f for _, f in files], device=DEV)
    b = jpeg.JpegFiles([f for _, f in files], device=DEV, all_layouts=True)
    assert b.parts is None and not b.all_layouts and b._entry == a._entry == "attwarp_jpegdec_decode"
    assert a.table_host.tobytes() == b.table_host.tobytes() and torch.equal(a.stream, b.stream)
    va, sa = a.run()
    vb, sb = b.run()
    assert torch.equal(a.buffer, b.buffer) and torch.equal(sa, sb) and sa.cpu().tolist() == [0] * 4
    for name in ("cmyk_s2_33x20", "edit_440_8x16", "keep_rgb_16x16"):
        with pytest.raises(ValueError, match="components|sampling layout|RGB-coded"):
            jpeg.decode_jpeg([files[0][1], F.good_file(name)], device=DEV)


def test_two_runs_and_a_non_default_stream_give_the_same_bytes():
    from attwarp_amd import jpeg
    files = [(n, F.good_file(n)) for n in ("long_410", "cmyk_s2_ri_row", "coef_y3x1_51x21", "long_ycck_k2x2", "coef_rgb_g2x1_2x1")]
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, all_layouts=True)
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
    files = [(n, F.good_file(n)) for n in ("long_cmyk_s2", "coef_410_ri_row", "edit_411_97x9", "long_440")]
    jf = jpeg.JpegFiles([f for _, f in files], "keep", device=DEV, all_layouts=True)
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
    check_views(jf.views(), files, "keep")
