"""GPU tests of the PNG decoder's wave route (inflate="wave"): pixels equal Pillow's; filtered bytes, output
and status equal a run of the lane route over the same list bit for bit; windows, rounds and acceptance equal the
restatement's (tests/pngwave_ref.py), which decided them on the CPU.  Equality everywhere."""
import functools

import numpy as np
import pytest
import torch

import pngdec_cases as C
import pngdec_limit_cases as L
import pngdec_ref as D
import pngfmt_cases as FC
import pngwave_cases as WC
import pngwave_ref as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def restated(f, seg=W.SEGMENT_BYTES, mr=W.MAX_ROUNDS, force_serial=False):
    return W.decode_file(f, seg, mr, force_serial)[1]


def good_files():
    return [(n, f) for n, f, _ in L.limit_good()] + WC.good()


def check_views(views, files, mode, order="rgb", pillow=C.pillow):
    for (name, f), v in zip(files, views):
        want = pillow(f, mode)
        if order == "bgr":
            want = want[:, :, ::-1]
        got = v.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (name, mode, order)


def filtered(pf):
    """Per image the filtered bytes a run left in the scratch buffer (the PdImage records say where)."""
    h = pf.header
    rec = np.frombuffer(pf.table_host[int(h.off_images):int(h.off_images) + 56 * pf.B].tobytes(), np.uint8).reshape(pf.B, 56)
    off, n = rec[:, 8:16].copy().view(np.uint64)[:, 0], rec[:, 28:32].copy().view(np.uint32)[:, 0]
    scr = pf.scratch.cpu().numpy()
    return [scr[int(o):int(o) + int(k)].tobytes() for o, k in zip(off, n)]


def differing(files, got, want):
    return [(n, g, w) for (n, _), g, w in zip(files, got, want) if g != w]


@functools.lru_cache(maxsize=None)
def lane_run(mode, order):
    from attwarp_amd import png
    files = good_files()
    pf = png.PngFiles([f for _, f in files], mode, order, device=DEV)
    _, status = pf.run()
    return pf.buffer.clone(), status.cpu().tolist(), filtered(pf), pf.routes(), pf.kept()


@pytest.mark.parametrize("mode,order", [("RGB", "rgb"), ("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr"), ("L", "bgr"), ("keep", "bgr")])
def test_whole_corpus_in_one_call(mode, order):
    from attwarp_amd import png
    files = good_files()
    assert len(files) == 263 + len(WC.NAMES)
    out0, st0, filt0, routes0, kept0 = lane_run(mode, order)
    pf = png.PngFiles([f for _, f in files], mode, order, device=DEV, inflate="wave")
    views, status = pf.run()
    st = status.cpu().tolist()
    assert st == st0 == [0] * len(files), [(n, D.STATUS_NAMES[s]) for (n, _), s in zip(files, st) if s]
    check_views(views, files, mode, order)
    assert torch.equal(pf.buffer, out0)
    assert not differing(files, filtered(pf), filt0)
    assert pf.routes() == routes0 and pf.kept() == kept0
    want = [restated(f) for _, f in files]
    assert not differing(files, pf.wave_info(), want)
    serial = [r[0] == 1 for r in routes0]
    assert sum(serial) > 200 and all(w[2] == int(s) for w, s in zip(want, serial))   # every image of the serial route: accepted


def test_forced_serial_route_sends_every_file_through_the_wave():
    from attwarp_amd import _lib, png
    files = good_files()
    out0 = lane_run("RGB", "rgb")[0]
    pf = png.PngFiles([f for _, f in files], device=DEV, inflate="wave")
    with _lib.debug_override(pngdec_route=1):
        _, status = pf.run()
    assert status.cpu().tolist() == [0] * len(files) and torch.equal(pf.buffer, out0)
    assert [r[:2] for r in pf.routes()] == [(1, 0)] * len(files)
    info = pf.wave_info()
    assert not differing(files, info, [restated(f, force_serial=True) for _, f in files])
    assert all(i[2] == 1 for i in info)                                  # every good file is accepted: none may fall back
    assert sum(i[0] == 0 for i in info) < 60                             # (no window: a stream of stored blocks alone)


def test_malformed_files_among_good_ones_and_guard_bytes():
    from attwarp_amd import png
    bad = [(n, f) for n, f, _ in L.limit_malformed()] + [(n, f) for n, f, _ in C.malformed()] + [(n, f) for n, f, _ in WC.malformed()]
    assert len(L.limit_malformed()) == 35
    good = [(n, WC.case(n).file) for n in ("token48_edges", "match_chain_64", "ring_wraps_twice", "blocks_70")]
    files, is_bad = [], []
    for i, nf in enumerate(bad):                                         # good files at the start, in between and at the end
        if i % 5 == 0:
            files.append(good[(i // 5) % len(good)])
            is_bad.append(False)
        files.append(nf)
        is_bad.append(True)
    files.append(good[0])
    is_bad.append(False)
    lane = png.PngFiles([f for _, f in files], device=DEV)
    _, st0 = lane.run()
    st0 = st0.cpu().tolist()
    assert [s != 0 for s in st0] == is_bad
    pf = png.PngFiles([f for _, f in files], device=DEV, inflate="wave", segment_bytes=16)
    G = 64
    out = torch.full((pf.out_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    scr = torch.full((pf.scratch.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    pf.buffer, pf.scratch = out[G:G + pf.out_bytes], scr[G:G + pf.scratch.numel()]
    views, status = pf.run()
    got = status.cpu().tolist()
    assert [D.STATUS_NAMES[s] for s in got] == [D.STATUS_NAMES[s] for s in st0], differing(files, got, st0)
    assert got[[n for n, _ in files].index("reach_before_first_byte")] == D.E_DISTANCE
    for t in (out, scr):
        assert bool((t[:G] == 0xA5).all()) and bool((t[-G:] == 0xA5).all())
    info = pf.wave_info()
    assert not differing(files, info, [restated(f, 16) for _, f in files])
    assert all(i[2] == 0 for i, b in zip(info, is_bad) if b)
    # (token48_edges holds 00 00 FF FF by chance, a false sync point: the unit route decodes it, as without the keyword)
    assert [i[2] for i, b in zip(info, is_bad) if not b] == [int(r[0] == 1) for r, b in zip(pf.routes(), is_bad) if not b]
    assert sum(i[2] for i in info) >= 6
    ok = [(nf, v) for nf, v, b in zip(files, views, is_bad) if not b]
    check_views([v for _, v in ok], [nf for nf, _ in ok], "RGB")
    assert pf.routes() == lane.routes() and pf.kept() == lane.kept()


@pytest.mark.parametrize("seg,mr", [(16, 64), (256, 64), (16, 63), (64, 1)])
def test_other_parameters(seg, mr):
    from attwarp_amd import png
    files = WC.good() + [(n, L.case(n).file) for n in ("lit15", "dist15", "len258_dist32768", "stored_65535", L.seeded()[5][0])]
    pf = png.PngFiles([f for _, f in files], device=DEV, inflate="wave", segment_bytes=seg, max_rounds=mr)
    views, status = pf.run()
    assert status.cpu().tolist() == [0] * len(files)
    check_views(views, files, "RGB")                                      # accepted or fallen back: the pixels do not change
    want = [restated(f, seg, mr) for _, f in files]
    info = pf.wave_info(resolution=True)
    assert not differing(files, [i[:3] for i in info], want)
    by = dict(zip([n for n, _ in files], info))
    if (seg, mr) == (16, 64):
        assert by["out_of_phase_64"] == (1, 64, 1, 1) and by["match_chain_64"][2:] == (1, 64) and by["windows_3"][0] == 3
    if (seg, mr) == (16, 63):
        assert by["out_of_phase_64"][:3] == (1, 63, 0)                       # one round short: the lane route decoded it
    if mr == 1:
        assert sum(i[2] for i in info) < len(files) and by["short_block"][:3] == (1, 1, 1)


def test_mixed_call_in_input_order():
    from attwarp_amd import png
    fmt = {k.name: k for k in FC.small_good()}
    pal = next(k for k in FC.pillow_written() if k.ctype == 3)
    lace = fmt["adam7_rgb8_9x9"]
    files = [("own_500_sub", C.good_file("own_500_sub")), (pal.name, pal.file), ("ring_wraps_twice", WC.case("ring_wraps_twice").file),
             (lace.name, lace.file), ("photo_level9_idat1", C.good_file("photo_level9_idat1")), ("match_chain_64", WC.case("match_chain_64").file)]
    pf = png.PngFiles([f for _, f in files], device=DEV, all_formats=True, inflate="wave")
    assert pf.header.formats == 1
    views, status = pf.run()
    assert status.cpu().tolist() == [0] * len(files)
    check_views(views, files, "RGB", pillow=FC.pillow)
    info, routes = pf.wave_info(), pf.routes()
    assert routes[0][0] == 0 and info[0] == (0, 0, 0)                     # this project's own file: the unit route, no wave
    assert all(i[2] == 1 for i, r in zip(info, routes) if r[0] == 1) and sum(r[0] == 1 for r in routes) >= 4
    got = png.decode_png([f for _, f in files], device=DEV, all_formats=True, inflate="wave")
    assert all(torch.equal(a, b) for a, b in zip(got, views))


def test_run_is_capturable_and_replays_agree():
    from attwarp_amd import png
    files = [(n, WC.case(n).file) for n in ("token48_edges", "windows_3", "stored_65535_then_dist32768")] + [("own_500_sub", C.good_file("own_500_sub"))]
    pf = png.PngFiles([f for _, f in files], device=DEV, inflate="wave")
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
        first = pf.buffer.clone()
        pf.buffer.zero_()
        pf.scratch.zero_()
        g.replay()
        s.synchronize()
    assert torch.equal(pf.buffer, first)
    check_views(pf.views(), files, "RGB")
    assert [i[2] for i in pf.wave_info()] == [int(r[0] == 1) for r in pf.routes()] and [r[0] for r in pf.routes()][1:] == [1, 1, 0]


def test_interface():
    from attwarp_amd import png
    files = [f for _, f in good_files()[:40]]
    lane, wave = png.PngFiles(files, device=DEV), png.PngFiles(files, device=DEV, inflate="wave", segment_bytes=32, max_rounds=7)
    h, w = lane.header, wave.header
    assert h.reserved2 == 0 and w.reserved2 == 1 | 32 << 8 | 7 << 20
    assert int(w.scratch_bytes) == int(h.scratch_bytes) + 16 * len(files) and int(h.table_bytes) == int(w.table_bytes)
    a, b = lane.table_host.copy(), wave.table_host.copy()
    hdr = png._lib.PngDecHeader
    for t in (a, b):                                                      # but for the mark and the scratch size, byte for byte one table
        t[hdr.reserved2.offset:hdr.reserved2.offset + 4] = 0
        t[hdr.scratch_bytes.offset:hdr.scratch_bytes.offset + 8] = 0
    assert np.array_equal(a, b)
    explicit = png.PngFiles(files, device=DEV, inflate="lane")
    assert np.array_equal(explicit.table_host, lane.table_host)
    with pytest.raises(ValueError, match="inflate"):
        png.PngFiles(files, device=DEV, inflate="warp")
    with pytest.raises(ValueError, match="segment_bytes"):
        png.PngFiles(files, device=DEV, inflate="wave", segment_bytes=48)
    with pytest.raises(ValueError, match="max_rounds"):
        png.PngFiles(files, device=DEV, inflate="wave", max_rounds=65)
    with pytest.raises(ValueError, match="inflate='lane'"):
        lane.wave_info()
