"""The host side of ``all_scans=True`` (attwarp_amd/jpeg.py, attwarp_jpegdec_plan_layout_scans) without a GPU: what parse_jpeg
makes of every file of tests/jpegscan_cases.py against the restatement, the planner's checks one by one through the C ABI,
that lists without a file of the new kind plan to the same bytes with and without the keyword, that without it every file
raises what it raised before, and the shared host / device text of jpegscan_blocks.hpp run as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/jpegscan_host_main.cpp) over the whole corpus, malformed files
included."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpegdec_cases as B
import jpegfmt_cases as L
import jpegprog_cases as PC
import jpegscan_cases as C
import jpegscan_ref as R
from attwarp_amd import _lib, jpeg

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_parse_jpeg_fields_equal_the_restatement():
    for name, f in C.good() + C.malformed():
        p, q = R.parse(f), jpeg.parse_jpeg(f, 0, all_scans=True)
        assert q["scanned"] is True and q["sequential"] == p["sequential"] and "progressive" not in q and "layout" not in q, name
        hmax, vmax = max(h for h, _ in p["samp"]), max(v for _, v in p["samp"])
        assert (q["W"], q["H"], q["ncomp"], q["hs"], q["vs"], q["ri"], q["units"]) == (p["W"], p["H"], p["ncomp"], hmax, vmax, 0, p["units"]), name
        assert q["samp"] == p["samp"] and q["color"] == p["color"] and q["levels"] == p["levels"] and q["data_off"] == p["first"], name
        assert [list(t) for t in q["qt"]] == p["qt"] and q["dc"] == q["ac"] == [], name
        assert len(q["scans"]) == len(p["scans"]), name
        for a, b in zip(q["scans"], p["scans"]):
            assert tuple(a[k] for k in ("comps", "ss", "se", "ah", "al", "ri", "off", "units")) == tuple(b[k] for k in ("comps", "ss", "se", "ah", "al", "ri", "off", "units")), name
            assert bool(a.get("sequential")) == b["seq"] and [(list(c), list(s)) for c, s in a["tables"]] == b["dc"] + b["ac"], name
            assert a["end"] == next((x for x in R.P.markers(f) if x >= a["off"]), len(f)), name
    seq = jpeg.parse_jpeg(C.good_file("seq_420_16x16_ri_mcu"), all_scans=True)               # a plain layout in three scans belongs here too
    assert seq["samp"] == [(2, 2), (1, 1), (1, 1)] and seq["color"] == "ycc" and seq["levels"] == [0, 0, 0] and seq["sequential"]


def test_files_of_the_three_older_kinds_parse_and_plan_as_with_both_older_keywords():
    base = [f for _, f in B.good()][:12]
    prog = [f for _, f in PC.good()][:6]
    lay = [L.good_file(n) for n in ("cmyk_s2_33x20", "coef_410_33x17", "long_440", "keep_rgb_23x19")]
    for f in base + prog + lay:
        assert jpeg.parse_jpeg(f, 3, all_scans=True) == jpeg.parse_jpeg(f, 3, progressive=True, all_layouts=True)
    for files, kw in ((base, dict()), (base, dict(mode="L", order="bgr", substreams=False)), (prog, dict(progressive=True)), (prog, dict(progressive=True, levels=False)),
                      (lay, dict(all_layouts=True, mode="keep"))):
        a, b = jpeg.plan(files, **kw), jpeg.plan(files, **dict(kw, all_scans=True))
        c = jpeg.plan(files, **dict(kw, progressive=True, all_layouts=True))
        assert a[0] == b[0] == c[0] and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()


def test_without_the_keyword_every_good_file_raises_what_it_raised_before():
    both = dict(progressive=True, all_layouts=True)
    seen = set()
    for name, f in C.good():
        p = R.parse(f)
        plain = p["color"] == "ycc" and p["samp"][1:] == [(1, 1), (1, 1)] and p["samp"][0] in ((1, 1), (2, 1), (2, 2))
        if p["sequential"]:
            word = "more than one scan" if plain else None
            for kw in (dict(), both):
                with pytest.raises(ValueError) as e:
                    jpeg.parse_jpeg(f, 2, **kw)
                assert kw == dict() or "the scan does not hold all components in frame order (more than one scan)" in str(e.value), name
                assert word is None or word in str(e.value), name
            seen.add("seq")
        else:
            with pytest.raises(ValueError, match="progressive frame"):
                jpeg.parse_jpeg(f, 2)
            with pytest.raises(ValueError, match="all_layouts covers sequential files only"):
                jpeg.parse_jpeg(f, 2, **both)
            seen.add("prog")
        with pytest.raises(ValueError):
            jpeg.plan([f], **both)
    assert seen == {"seq", "prog"}


def test_a_scan_plan_has_its_own_table_and_refuses_a_mixed_list():
    files = [C.good_file(n) for n in ("pil_cmyk_s2_33x20", "seq_420_16x16_ri_mcu", "limit_64_scans", "edit_440_24x32")]
    parsed, table, hdr = jpeg.plan(files, "keep", all_scans=True)
    magics = {jpeg.plan([B.good()[0][1]])[2].magic, jpeg.plan([L.good_file("cmyk_s2_33x20")], all_layouts=True)[2].magic}
    assert hdr.magic not in magics and hdr.B == 4 and hdr.table_bytes == table.size and hdr.total_units == 4 and hdr.reserved == 0
    assert hdr.out_bytes == sum(p["W"] * p["H"] * p["ncomp"] for p in parsed) and [p["segments"] for p in parsed] == [0] * 4
    assert jpeg.plan(files, "keep", all_scans=True)[1].tobytes() == table.tobytes()          # the headers and the lengths alone
    flat = jpeg.plan(files, "keep", all_scans=True, levels=False)
    assert flat[1].tobytes() != table.tobytes() and flat[2].scratch_bytes == hdr.scratch_bytes
    with pytest.raises(ValueError, match="JpegFiles splits"):
        jpeg.plan(files + [B.good()[0][1]], all_scans=True)
    for entry, own in (("attwarp_jpegdec_decode", "attwarp_jpegdec_plan"), ("attwarp_jpegdec_decode_layouts", "attwarp_jpegdec_plan_layouts"),
                       ("attwarp_jpegdec_decode_scans", "attwarp_jpegdec_plan_scans")):
        with pytest.raises(_lib.AttWarpError, match="not a table of " + own):                # checked before anything is launched
            _lib.call(entry, table.ctypes.data, 256, 256, 256, 256, 1 << 30, 256, None)
    for other in (jpeg.plan([B.good()[0][1]])[1], jpeg.plan([L.good_file("cmyk_s2_33x20")], all_layouts=True)[1],
                  jpeg.plan([PC.good()[0][1]], progressive=True)[1]):
        with pytest.raises(_lib.AttWarpError, match="not a table of attwarp_jpegdec_plan_layout_scans"):
            _lib.call("attwarp_jpegdec_decode_layout_scans", other.ctypes.data, 256, 256, 256, 256, 1 << 30, 256, None)


# ---- the planner's checks, one by one through the C ABI ------------------------------------------------------------------------------
def _image(**kw):
    rec = np.zeros(1, dtype=np.dtype(_lib.JpegDecLayoutImage))
    rec["H"], rec["W"], rec["ncomp"], rec["color"], rec["stream_len"] = 20, 33, 4, _lib.JPEGDEC_COLOR_IDS["cmyk"], 1000
    rec["h"], rec["v"] = [2, 1, 1, 1], [2, 1, 1, 1]
    rec["qt"][:] = 1
    for key, value in kw.items():
        rec[key] = value
    return rec


def _scans(*entries):
    """entries: dict(comp=[...], ss, se, ah, al, sequential, restart_interval, stream_off, image) with defaults of a DC first pass."""
    rec = np.zeros(len(entries), dtype=np.dtype(_lib.JpegDecLayoutScan))
    for i, e in enumerate(entries):
        comp = e.get("comp", [0, 1, 2, 3])
        rec["ncomp"][i] = e.get("ncomp", len(comp))
        rec["comp"][i] = (list(comp) + [0] * 4)[:4]
        for key in ("ss", "se", "ah", "al", "sequential", "restart_interval", "stream_off", "image"):
            rec[key][i] = e.get(key, 0)
        for t in range(4):
            jpeg._put_tables(rec["dc_counts"][i][t:t + 1], rec["dc_symbols"][i][t:t + 1], [R.P.DC_TABLE])
            jpeg._put_tables(rec["ac_counts"][i][t:t + 1], rec["ac_symbols"][i][t:t + 1], [R.P.AC_TABLE])
    return rec


def _plan(images, scans, by_level=1, short=0):
    lib = _lib.load()
    n = lib.attwarp_jpegdec_layout_scans_table_bytes(images.ctypes.data, len(images), len(scans))
    assert n > 0
    table = np.zeros(n, np.uint8)
    _lib.call("attwarp_jpegdec_plan_layout_scans", images.ctypes.data, len(images), scans.ctypes.data, len(scans), table.ctypes.data, n - short, by_level)
    return table


GOOD = [dict(), dict(comp=[0], ss=1, se=63), dict(comp=[1, 3], sequential=1, se=63)]


@pytest.mark.parametrize("scans,word", [
    ([dict(ss=2, se=1)], "bad progression"), ([dict(se=64, ss=1, comp=[0])], "bad progression"), ([dict(se=5)], "bad progression"),
    ([dict(ss=1, se=5, comp=[0, 1])], "bad progression"), ([dict(al=14)], "bad progression"), ([dict(ah=2, al=0)], "bad progression"),
    ([dict(comp=[1, 0])], "frame order"), ([dict(comp=[0, 0])], "frame order"), ([dict(comp=[0, 4])], "frame order"), ([dict(comp=[-1])], "frame order"),
    ([dict(ncomp=0)], "0 components"), ([dict(ncomp=5)], "5 components"), ([dict(sequential=1, se=62)], "sequential scan"),
    ([dict(sequential=1, se=63, al=1)], "sequential scan"), ([dict(restart_interval=65536)], "restart interval"),
    ([dict(stream_off=1001)], "outside the image"), ([dict(image=1)], "out of order"), ([dict()] * 65 + [dict(image=1)], "more than 64 scans"),
    ([dict(comp=[0], restart_interval=1)] * 64, "units over its scans")], ids=lambda v: v if isinstance(v, str) else "")
def test_the_planner_checks_what_the_kernels_bounds_rest_on(scans, word):
    _plan(_image(), _scans(*GOOD))
    img = _image(H=4096, W=4096) if word == "units over its scans" else _image()
    if word == "more than 64 scans":                         # (65 scans of one image among two: the table's size admits 128)
        img = np.concatenate([_image(), _image()])
    with pytest.raises(_lib.AttWarpError, match=word):
        _plan(img, _scans(*scans))


def test_the_planner_checks_tables_images_and_arguments():
    for field, at, value, word in (("dc_counts", (0, 2, 0), 3, "over-subscribed"), ("dc_symbols", (0, 1, 3), 16, "DC category"),
                                   ("ac_counts", (1, 0, 0), 3, "over-subscribed")):
        rec = _scans(*GOOD)
        rec[field][at] = value
        with pytest.raises(_lib.AttWarpError, match=word):
            _plan(_image(), rec)
    rec = _scans(*GOOD)
    rec["ac_counts"][0, 0, 0] = 3                           # a DC scan names no AC table: not looked at
    _plan(_image(), rec)
    for kw, word in ((dict(restart_interval=4), "belongs to the scans"), (dict(h=[4, 1, 1, 1], v=[2, 1, 1, 2]), "blocks per MCU"),
                     (dict(h=[3, 2, 1, 1]), "fractional"), (dict(ncomp=2), "2 components"), (dict(color=1), "colour rule")):
        with pytest.raises(_lib.AttWarpError, match=word):
            _plan(_image(**kw), _scans(*GOOD))
    with pytest.raises(_lib.AttWarpError, match="needed"):
        _plan(_image(), _scans(*GOOD), short=1)
    lib = _lib.load()
    assert lib.attwarp_jpegdec_layout_scans_table_bytes(_image().ctypes.data, 1, 0) == 0
    assert lib.attwarp_jpegdec_layout_scans_table_bytes(_image().ctypes.data, 1, 65) == 0
    two = np.concatenate([_image(), _image()])
    with pytest.raises(_lib.AttWarpError, match="image 1 has no scan"):
        _plan(two, _scans(dict(), dict(comp=[0], ss=1, se=63)))
    a, b = _plan(_image(), _scans(*GOOD)), _plan(_image(), _scans(*GOOD), by_level=0)      # one level, or one per scan position
    assert a.tobytes() != b.tobytes()


# ---- the shared core as a program of its own, under the sanitizers ------------------------------------------------------------------------
def corpus(files):
    out = [struct.pack("<I", len(files))]
    for f in files:
        p = R.parse(f)
        nf, data = p["ncomp"], p["data"][p["first"]:]
        hv = [h for h, _ in p["samp"]] + [1] * (4 - nf) + [v for _, v in p["samp"]] + [1] * (4 - nf)
        out.append(struct.pack("<III8IIII", p["W"], p["H"], nf, *hv, _lib.JPEGDEC_COLOR_IDS[p["color"]], len(p["scans"]), len(data)) + data)
        for s in p["scans"]:
            out.append(struct.pack("<I4I9I", len(s["comps"]), *(s["comps"] + [0] * 4)[:4], s["ss"], s["se"], s["ah"], s["al"], int(s["seq"]), s["ri"],
                                   s["off"] - p["first"], len(s["dc"]), len(s["ac"])))
            for counts, syms in s["dc"] + s["ac"]:
                out.append(bytes(counts) + bytes(syms).ljust(256, b"\0"))
    return b"".join(out)


def test_host_core_under_sanitizers_equals_the_restatement(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "jpegscan_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "jpegscan_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    cases = C.good() + C.malformed()
    (tmp_path / "corpus.bin").write_bytes(corpus([f for _, f in cases]))
    r = subprocess.run([str(exe), str(tmp_path / "corpus.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    for (name, f), line in zip(cases, lines):
        st, _, info = R.decode(f)
        assert tuple(int(x) for x in line.split()) == (st, info["crc"], info["units"]), name
