"""CPU tests of the PNG decoder's restatement (tests/pngdec_ref.py) against zlib and Pillow on every file of
tests/pngdec_cases.py, of the routes the files take, and of what the host refuses before any launch."""
import itertools
import zlib

import numpy as np
import pytest
from PIL import Image

import pngdec_cases as C
import pngdec_ref as D


@pytest.fixture(scope="module")
def decoded():
    """{name: (status, RGB image, info)} of every good file, computed once."""
    return {n: D.decode(f, "RGB") for n, f in C.good()}


def test_every_good_file_equals_zlib_and_pillow(decoded):
    for name, f in C.good():
        st, img, info = decoded[name]
        assert st == D.OK, (name, D.STATUS_NAMES[st])
        p = D.parse(f)
        filt = zlib.decompress(p["stream"])
        assert info["adler"] == zlib.adler32(filt), name
        assert np.array_equal(img, C.pillow(f, "RGB")), name
    for name, f in C.good()[::7]:                     # the other modes on a sample that holds every colour type
        for mode, order in (("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr")):
            st, img, _ = D.decode(f, mode, order)
            want = C.pillow(f, mode)
            assert st == D.OK and np.array_equal(img, want[:, :, ::-1] if order == "bgr" else want), (name, mode)


def test_colour_types_in_every_mode():
    for name in ("pil_L_l6", "pil_LA_opt", "pil_RGB_l9", "pil_RGBA_l1", "geo_rgba", "geo_grey_alpha"):
        f = C.good_file(name)
        for mode in ("RGB", "L", "keep"):
            st, img, _ = D.decode(f, mode)
            assert st == D.OK and np.array_equal(img, C.pillow(f, mode)), (name, mode)


def test_luma_is_pillows_at_every_rounding_boundary():
    edge = [0, 1, 127, 128, 254, 255]
    sweep = np.arange(256)
    rows = []
    for a, b in itertools.product(edge, edge):
        for k in range(3):
            px = np.zeros((256, 3), np.uint8)
            px[:, k] = sweep
            px[:, (k + 1) % 3], px[:, (k + 2) % 3] = a, b
            rows.append(px)
    rgb = np.stack(rows)
    want = np.asarray(Image.fromarray(rgb).convert("L"))
    assert np.array_equal(D.luma(rgb), want)


def test_routes(decoded):
    info = lambda n: decoded[n][2]
    for tag in ("one", "idat7", "idat1"):
        assert info(f"photo_sync_flush_{tag}") == dict(info(f"photo_sync_flush_{tag}"), route="serial", nunits=2)   # dependent second half
        assert info(f"photo_full_flush_{tag}") == dict(info(f"photo_full_flush_{tag}"), route="unit", nunits=2, chain=2)
        assert info(f"photo_level9_{tag}")["route"] == "serial" and info(f"photo_level9_{tag}")["nunits"] == 1
    i = info("false_sync")                            # the candidate inside the stored data is never arrived at
    assert (i["route"], i["nunits"], i["chain"]) == ("unit", 2, 1)
    i = info("many_false")                            # 480 patterns in one stored block: the cap keeps 256, none is real
    assert (i["route"], i["nunits"], i["chain"]) == ("unit", D.MAX_UNITS, 1)
    i = info("many_flush")                            # 311 real boundaries: the last kept unit decodes on to the end
    assert (i["route"], i["nunits"], i["chain"]) == ("unit", D.MAX_UNITS, D.MAX_UNITS)
    i = info("own_500_sub")                           # 32 segments + the final empty block; the marker before the Adler is garbage
    assert (i["route"], i["nunits"], i["chain"]) == ("unit", 34, 33)
    # one unit per dynamic segment (it ends behind an empty stored block) plus the final block; stored segments add none
    import png_cases as PC
    import png_ref as R
    for name, img, filt, order in PC.cases():
        if name in ("one_segment", "segment_plus_row", "last_segment_one_row", "noise_stored", "all_zero"):
            fl = R.filtered_stream(img, filt, order)
            dyn = sum((R.encode_segment(fl[r0:r0 + nr].tobytes())[0] & 7) == 4 for r0, nr in R.segments(*fl.shape))
            assert info("own_" + name)["chain"] == dyn + 1, name
    # a second half that reaches back is what makes the sync-flush file dependent
    s = D.parse(C.good_file("photo_sync_flush_one"))["stream"]
    kept = D.find_markers(s)
    u = D.inflate(s, kept[1], 37 * 160, set(kept), write=False)
    assert u.status == D.OK and u.dependent == 1 and u.final == 1


def test_forced_serial_route_gives_the_same_bytes():
    for name in ("own_500_sub", "photo_full_flush_one", "false_sync", "own_noise_stored"):
        f = C.good_file(name)
        a, b = D.decode(f, "RGB"), D.decode(f, "RGB", force_serial=True)
        assert a[0] == b[0] == D.OK and np.array_equal(a[1], b[1]) and b[2]["route"] == "serial"


def test_token_walk_far_and_overlapping_matches():
    s = D.parse(C.good_file("far_match"))["stream"]
    r = D.inflate(s, 2, 2 * 32768)
    assert r.status == D.OK and (258, 32768) in r.seen and {d for _, d in r.seen} == {32768}
    s = D.parse(C.good_file("distance1"))["stream"]
    r = D.inflate(s, 2, 30 * 121)
    assert r.status == D.OK and any(d == 1 and l > 1 for l, d in r.seen)
    assert len(D.parse(C.good_file("geo_row32768"))["stream"]) and D.parse(C.good_file("geo_row32768"))["W"] + 1 == 32768


def test_malformed_statuses():
    names = [n for n, _, _ in C.malformed()]
    assert 15 <= len(names) <= 24 and len(set(names)) == len(names)
    seen = set()
    for name, f, want in C.malformed():
        st, img, info = D.decode(f)
        assert st != D.OK and img is None, name
        if want is not None:
            assert st == want, (name, D.STATUS_NAMES[st])
        seen.add(st)
        p = D.parse(f)
        if st not in (D.E_CRC, D.E_FILTER, D.E_OVERFLOW):     # zlib itself rejects the rest, or gives another size
            try:
                assert len(zlib.decompress(p["stream"])) != 37 * 160, name
            except zlib.error:
                pass
    assert {D.E_ZLIB_HEADER, D.E_SYMBOL, D.E_CRC, D.E_TRUNCATED, D.E_BLOCK_TYPE, D.E_STORED_LEN, D.E_CODE_LENGTHS, D.E_DISTANCE, D.E_OVERFLOW, D.E_UNDERFLOW,
            D.E_ADLER, D.E_FILTER} <= seen
    st, _, _ = D.decode(next(f for n, f, _ in C.malformed() if n == "wrong_crc"), check_crc=False)
    assert st == D.OK


def test_marker_scan_keeps_the_first_positions():
    s = b"\x78\x01" + (b"\x00\x00\xff\xff" + b"\x55") * 300
    kept = D.find_markers(s)
    assert len(kept) == D.MAX_UNITS and kept[:3] == [2, 6, 11] and kept == sorted(kept)
    assert D.find_markers(b"\x78\x01\x00\x00\xff\xff") == [2]                     # a position at the stream's end starts nothing


def test_host_refuses_before_any_launch():
    """ValueError from the chunk walk alone: no device, no library call."""
    from attwarp_amd import png
    for name, f, word in C.refused():
        with pytest.raises(ValueError, match=word):
            D.parse(f)
        with pytest.raises(ValueError):
            png.parse_png(f)
        with pytest.raises(ValueError):
            png.PngFiles([C.good_file("geo_1x1"), f])
    for name, f in C.good()[::5]:
        p = D.parse(f)
        W, H, ctype, spans = png.parse_png(f)
        assert (W, H, ctype) == (p["W"], p["H"], p["color_type"]) and [(l, c) for _, l, c in spans] == [(len(c), crc) for c, crc in p["chunks"]]
        assert b"".join(f[o:o + l] for o, l, _ in spans) == p["stream"]


def test_status_names_mirror_the_header():
    import os
    import re
    from attwarp_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "attwarp.h")).read()
    codes = dict((n, int(v)) for n, v in re.findall(r"ATTWARP_PNGDEC_(OK|E_\w+) = (\d+)", hdr))
    assert [codes[n] for n in _lib.PNGDEC_STATUS_NAMES] == list(range(13)) and list(_lib.PNGDEC_STATUS_NAMES) == D.STATUS_NAMES
    assert int(re.search(r"#define ATTWARP_PNGDEC_MAX_UNITS (\d+)", hdr).group(1)) == _lib.PNGDEC_MAX_UNITS == D.MAX_UNITS
    assert int(re.search(r"#define ATTWARP_PNGDEC_MAX_ROW_BYTES (\d+)", hdr).group(1)) == _lib.PNGDEC_MAX_ROW_BYTES == D.MAX_ROW_BYTES
