"""GPU tests of the PNG decoder at its code, scan, chunk, row and carry limits (tests/pngdec_limit_cases.py; the corpus itself
is proved on the CPU by test_pngdec_limits_ref_cpu.py): every pixel equals Pillow's, every status, route, chain and kept
position the restatement's (tests/pngdec_ref.py).  Equality everywhere."""
import functools

import numpy as np
import pytest
import torch

import pngdec_cases as C
import pngdec_limit_cases as L
import pngdec_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROUTE_ID = {"unit": 0, "serial": 1, None: 2}


@functools.lru_cache(maxsize=None)
def restated(f, check_crc=True):
    """(status, (route, chain, kept count), kept positions) of one file in the restatement."""
    st, _, info = D.decode(f, check_crc=check_crc)
    s = D.parse(f)["stream"]
    return st, (ROUTE_ID[info["route"]], info["chain"], info["nunits"]), (D.find_markers(s) if D.zlib_header(s) == D.OK else [])


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


def good_files():
    return [(n, f) for n, f, _ in L.limit_good()]


def differing(files, got, want):
    return [(n, g, w) for (n, _), g, w in zip(files, got, want) if g != w]


@pytest.mark.parametrize("mode,order", [("RGB", "rgb"), ("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr")])
def test_whole_limit_corpus_in_one_call(mode, order):
    from attwarp_amd import png
    files = good_files()
    assert len(files) > 200                                              # the chain kernel's grid of 64 images crosses 64 and 128
    pf = png.PngFiles([f for _, f in files], mode, order, device=DEV)
    views, status = pf.run()
    st = status.cpu().tolist()
    assert st == [0] * len(files), [(n, D.STATUS_NAMES[s]) for (n, _), s in zip(files, st) if s]
    back_to_back(views, pf.buffer)
    check_views(views, files, mode, order)
    want = [restated(f) for _, f in files]
    assert not differing(files, pf.routes(), [w[1] for w in want])
    got = dict(zip([n for n, _ in files], pf.kept()))
    assert not differing(files, list(got.values()), [w[2] for w in want])
    stated = {n: k for n, k in L.scan_kept().items() if n in got}        # (and the builders' own lists, where there are any)
    assert len(stated) == 23 and {n: got[n] for n in stated} == stated


def test_serial_route_gives_the_same_bytes():
    from attwarp_amd import _lib, png
    files = good_files()
    pf = png.PngFiles([f for _, f in files], device=DEV)
    _, status = pf.run()
    first = pf.buffer.clone()
    assert status.cpu().tolist() == [0] * len(files) and sum(r[0] == 0 for r in pf.routes()) >= 40    # (20 scan files, 20 seeded ones at least)
    pf.buffer.fill_(0x5A)
    with _lib.debug_override(pngdec_route=1):
        _, status = pf.run()
    assert status.cpu().tolist() == [0] * len(files) and torch.equal(pf.buffer, first)
    assert [r[:2] for r in pf.routes()] == [(1, 0)] * len(files)


def test_malformed_limit_files_among_good_ones_and_guard_bytes():
    from attwarp_amd import png
    bad = L.limit_malformed()
    good = [(n, L.case(n).file) for n in ("carry_c4_s2", L.seeded()[3][0], "scan_tile_true_2047", "idat_len_257", "dist15")]
    files, is_bad = [], []
    for i, (name, f, _) in enumerate(bad):                               # good files at the start, in between and at the end
        if i % 4 == 0:
            files.append(good[(i // 4) % len(good)])
            is_bad.append(False)
        files.append((name, f))
        is_bad.append(True)
    files.append(good[0])
    is_bad.append(False)
    want = [restated(f) for _, f in files]
    assert all((w[0] != 0) == b for w, b in zip(want, is_bad))
    pf = png.PngFiles([f for _, f in files], device=DEV)
    G = 64
    out = torch.full((pf.out_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    scr = torch.full((pf.scratch.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    pf.buffer, pf.scratch = out[G:G + pf.out_bytes], scr[G:G + pf.scratch.numel()]
    views, status = pf.run()
    got = status.cpu().tolist()
    assert [D.STATUS_NAMES[s] for s in got] == [D.STATUS_NAMES[w[0]] for w in want], differing(files, got, [w[0] for w in want])
    for t in (out, scr):
        assert bool((t[:G] == 0xA5).all()) and bool((t[-G:] == 0xA5).all())
    back_to_back(views, pf.buffer)
    ok = [(nf, v) for nf, v, s in zip(files, views, got) if s == 0]
    check_views([v for _, v in ok], [nf for nf, _ in ok], "RGB")
    assert not differing(files, pf.routes(), [w[1] for w in want])
    assert not differing(files, pf.kept(), [w[2] for w in want])
    kept = dict(zip([n for n, _ in files], pf.kept()))
    assert kept["scan_trunc_plus1"] == L.scan_kept()["scan_trunc_plus1"] and kept["scan_trunc_plus0"] == L.scan_kept()["scan_trunc_plus0"]
    # the CRC files with the check off: status 0 where only the CRC was wrong
    crc = [(n, f) for n, f, _ in bad if n.startswith("crc_")]
    assert [n for n, _ in crc] == ["crc_flip_first", "crc_flip_last", "crc_wrong_on_empty_chunk"]
    pf = png.PngFiles([f for _, f in crc], check_crc=False, device=DEV)
    views, status = pf.run()
    want = [restated(f, False) for _, f in crc]
    assert status.cpu().tolist() == [w[0] for w in want] and want[2][0] == 0 and want[0][0] != 0 and want[1][0] != 0
    check_views(views[2:], crc[2:], "RGB")


def test_row_limit_files():
    from attwarp_amd import png
    cases = L.limit_rowmax()
    files = [(k.name, k.file) for k in cases]
    pf = png.PngFiles([f for _, f in files], "keep", device=DEV)
    assert pf.header.lds_bytes == png.PNGDEC_MAX_ROW_BYTES == 49152
    views, status = pf.run()
    assert status.cpu().tolist() == [0, 0]
    back_to_back(views, pf.buffer)
    check_views(views, files, "keep")
    assert pf.routes() == [(0, k.expect["chain"], k.expect["nkept"]) for k in cases] == [(0, 65, 65)] * 2
    assert pf.kept() == [D.find_markers(D.parse(f)["stream"]) for _, f in files]
