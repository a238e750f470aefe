"""CPU tests of the JPEG decoder's restatement (tests/jpegdec_ref.py) against Pillow on every good file of
tests/jpegdec_cases.py, of the statuses of the malformed ones, of what the host refuses before any launch and of the
planning, which depends on the headers alone."""
import ctypes

import numpy as np
import pytest

import jpegdec_cases as C
import jpegdec_ref as D


def test_every_good_file_equals_pillow():
    assert 55 <= len(C.good()) <= 75
    for name, f in C.good():
        for mode in ("RGB", "L"):
            st, img, _ = D.decode(f, mode)
            assert st == D.OK, (name, D.STATUS_NAMES[st])
            want = C.pillow(f, mode)
            assert img.shape == want.shape and np.array_equal(img, want), (name, mode)
    for name, f in C.good()[::5]:
        st, img, _ = D.decode(f, "RGB", "bgr")
        assert np.array_equal(img, C.pillow(f, "RGB")[:, :, ::-1]), name
        st, img, _ = D.decode(f, "keep")
        assert np.array_equal(img, C.pillow(f, "keep")), name
    assert max(max(W, H) for W, H in ((D.parse(f)["W"], D.parse(f)["H"]) for _, f in C.good())) <= 200


def test_the_corpus_holds_what_it_claims():
    parsed = {n: D.parse(f) for n, f in C.good()}
    samplings = {(p["ncomp"], p["hs"], p["vs"]) for p in parsed.values()}
    assert samplings == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    for W, H in C.SIZES:
        assert any((p["W"], p["H"]) == (W, H) for p in parsed.values())
    for sub in ((1, 1), (2, 1), (2, 2)):                     # the sizes at which the edge rules of the up-sampling meet
        for size in ((1, 1), (2, 1), (1, 2), (17, 33), (40, 31)):
            assert any((p["W"], p["H"], p["hs"], p["vs"]) == size + sub for p in parsed.values() if p["ncomp"] == 3)
    # ZRL occurs, and codes longer than the 8-bit look-up
    before = dict(D.SEEN)
    assert D.entropy(parsed["zrl"])[0] == D.OK and D.SEEN["zrl"] > before["zrl"]
    assert D.entropy(parsed["q100_optimize"])[0] == D.OK and D.SEEN["long"] > before["long"]
    # stuffed bytes, one of them as the last data byte of a unit
    assert any(b"\xff\x00" in p["stream"] for p in parsed.values())
    s = parsed["ri_stuffed_end"]["stream"]
    assert any(s[i:i + 2] == b"\xff\x00" and s[i + 2] == 0xFF and 0xD0 <= s[i + 3] <= 0xD7 for i in range(len(s) - 3))
    # restart intervals
    g = {n: D.geometry(p) for n, p in parsed.items()}
    assert parsed["ri_1"]["ri"] == 1 and g["ri_1"]["nunits"] == g["ri_1"]["nmcu"] == 6
    assert parsed["ri_row"]["ri"] == g["ri_row"]["mcux"] and g["ri_row"]["nunits"] == g["ri_row"]["mcuy"]
    assert g["ri_not_dividing"]["nmcu"] % parsed["ri_not_dividing"]["ri"] != 0
    assert parsed["ri_larger"]["ri"] > g["ri_larger"]["nmcu"] and g["ri_larger"]["nunits"] == 1
    assert g["ri_wrap"]["nunits"] == 24 and g["ri_wrap_grey"]["nunits"] == 35
    assert parsed["grey_2x2_factors"]["ncomp"] == 1 and b"\x01\x22\x00" in C.good_file("grey_2x2_factors")
    assert b"\xff\xc1" in C.good_file("sof1")[:200] and b"\xff\xc0" not in C.good_file("sof1")[:200]


def test_malformed_statuses():
    names = [n for n, _, _ in C.malformed()]
    assert len(set(names)) == len(names)
    seen = set()
    for name, f, want in C.malformed():
        st, img, info = D.decode(f)
        assert st == want, (name, D.STATUS_NAMES[st])
        assert (img is None) == (st != D.OK)
        seen.add(st)
    assert seen == {D.OK, D.E_TRUNCATED, D.E_HUFFMAN, D.E_COEFF, D.E_RESTART, D.E_NO_EOI}


def test_hostile_values_are_defined():
    by = {n: f for n, f, _ in C.malformed()}
    st, planes, _ = D.entropy(D.parse(by["dc_predictor_overflow"]))
    dcs = planes[0][0, :, 0].astype(int).tolist()
    assert st == D.OK and dcs == [32767, -2, 32765, -2, -20002, -3618]       # the low 16 bits of 32767, 65534, 98301, ...
    # up to a constant 8 a plain clamp is what Pillow computes, too; from 16 on its range-limit table wraps
    q100 = C.good_file("q100_s0")
    f8 = C.edit(q100, lambda s: C.replace(s, 0xDB, lambda pl: b"".join(pl[q:q + 1] + bytes([8]) * 64 for q in range(0, len(pl), 65))))
    assert np.array_equal(D.decode(f8)[1], C.pillow(f8))
    for k in (16, 255):
        st, img, _ = D.decode(by[f"quant_{k}"])
        assert st == D.OK and img.shape == (20, 33, 3) and img.min() == 0 and img.max() == 255


def test_host_refuses_before_any_launch():
    """ValueError / OSError from the marker walk alone: no device, no library call."""
    from attwarp_amd import jpeg
    assert len(C.refused()) >= 24
    for name, f, exc, word in C.refused():
        with pytest.raises(exc, match=word):
            D.parse(f)
        with pytest.raises(exc, match=word):
            jpeg.parse_jpeg(f)
    for name, f in C.good():
        p, q = D.parse(f), jpeg.parse_jpeg(f)
        for key in ("W", "H", "ncomp", "hs", "vs", "ri"):
            assert p[key] == q[key], (name, key)
        assert [list(t) for t in q["qt"]] == p["qt"], name
        assert [(list(a), list(b)) for a, b in q["dc"]] == [(list(a), list(b)) for a, b in p["dc"]], name
        assert [(list(a), list(b)) for a, b in q["ac"]] == [(list(a), list(b)) for a, b in p["ac"]], name
        assert bytes(f[q["data_off"]:]) == p["stream"], name


def test_planning_equals_the_restatement():
    """attwarp_jpegdec_plan on the host: units, blocks and offsets follow from the headers alone."""
    from attwarp_amd import _lib, jpeg
    files = [f for _, f in C.good()] + [f for _, f, _ in C.malformed()]
    parsed, table, hdr = jpeg.plan(files, "keep", "rgb")
    geo = [D.geometry(D.parse(f)) for f in files]
    assert [p["units"] for p in parsed] == [g["nunits"] for g in geo]
    assert hdr.B == len(files) and hdr.total_units == sum(g["nunits"] for g in geo)
    assert hdr.out_bytes == sum(p["W"] * p["H"] * p["ncomp"] for p in parsed)
    assert hdr.stream_bytes == sum(len(D.parse(f)["stream"]) for f in files)
    assert max(g["nunits"] for g in geo) > 8
    assert hdr.scratch_bytes % 256 == 0 and hdr.scratch_bytes >= sum(g["nblocks"] * 192 for g in geo)
    for f in (C.good_file("ri_1"),):
        with pytest.raises(ValueError):
            jpeg.plan([f], "CMYK", "rgb")
    for name, f, exc, _ in C.refused()[:3]:
        with pytest.raises(exc):
            jpeg.plan([C.good_file("ri_1"), f])
    # the C planner refuses what the marker walk would have refused, for callers that fill the records themselves
    rec = (_lib.JpegDecImage * 1)()
    rec[0].H, rec[0].W, rec[0].ncomp, rec[0].hs, rec[0].vs = 16, 16, 3, 1, 2
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    assert lib.attwarp_jpegdec_plan(rec, 1, buf, len(buf)) != 0 and b"sampling" in lib.attwarp_last_error()
    rec[0].hs, rec[0].vs = 2, 2
    rec[0].dc_counts[0][0] = 3
    assert lib.attwarp_jpegdec_plan(rec, 1, buf, len(buf)) != 0 and b"over-subscribed" in lib.attwarp_last_error()
    rec[0].dc_counts[0][0] = 0
    rec[0].H, rec[0].W, rec[0].restart_interval = 65535, 65535, 1
    assert lib.attwarp_jpegdec_plan(rec, 1, buf, len(buf)) != 0 and b"restart intervals" in lib.attwarp_last_error()


def test_status_names_mirror_the_header():
    import os
    import re
    from attwarp_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "attwarp.h")).read()
    codes = dict((n, int(v)) for n, v in re.findall(r"ATTWARP_JPEGDEC_(OK|E_\w+) = (\d+)", hdr))
    assert [codes[n] for n in _lib.JPEGDEC_STATUS_NAMES] == list(range(6)) and list(_lib.JPEGDEC_STATUS_NAMES) == D.STATUS_NAMES
    assert int(re.search(r"#define ATTWARP_JPEGDEC_MAX_UNITS (\d+)", hdr).group(1)) == _lib.JPEGDEC_MAX_UNITS == D.MAX_UNITS
    assert int(re.search(r"#define ATTWARP_JPEGDEC_MAX_BLOCKS (\d+)", hdr).group(1)) == _lib.JPEGDEC_MAX_BLOCKS == D.MAX_BLOCKS
    modes = dict((n, int(v)) for n, v in re.findall(r"ATTWARP_JPEGDEC_(RGB|L|KEEP) = (\d+)", hdr))
    assert {k.upper(): v for k, v in _lib.JPEGDEC_MODE_IDS.items()} == modes
