"""The host side of ``all_layouts=True`` (attwarp_amd/jpeg.py, attwarp_jpegdec_plan_layouts) without a GPU: what parse_jpeg
makes of every file of tests/jpegfmt_cases.py, its refusals with their messages, that nothing changes without the keyword
or for lists of plain files with it, the planner's own checks, and the shared host / device text of jpegfmt_blocks.hpp run
as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (tests/jpegfmt_host_main.cpp) over the
whole corpus, the malformed files included."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpegdec_cases as C
import jpegdec_ref as D
import jpegfmt_cases as F
import jpegfmt_ref as R
from attwarp_amd import _lib, jpeg

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def is_plain(p):
    return p["color"] == "grey" or (p["color"] == "ycc" and p["samp"][1:] == [(1, 1), (1, 1)] and p["samp"][0] in ((1, 1), (2, 1), (2, 2)))


def test_parse_jpeg_fields_equal_the_restatement():
    kinds = set()
    for name, f in F.good() + F.malformed():
        p, q = R.parse(f), jpeg.parse_jpeg(f, 0, all_layouts=True)
        g = R.geometry(p)
        assert (q["W"], q["H"], q["ncomp"], q["ri"], q["units"]) == (p["W"], p["H"], p["ncomp"], p["ri"], g["nunits"]), name
        assert [list(t) for t in q["qt"]] == p["qt"], name
        assert [(list(c), list(s)) for c, s in q["dc"] + q["ac"]] == p["dc"] + p["ac"], name
        assert bytes(memoryview(f)[q["data_off"]:]) == p["stream"], name
        if is_plain(p):
            assert "layout" not in q and (q["hs"], q["vs"]) == p["samp"][0], name
        else:
            assert q["layout"] is True and q["samp"] == p["samp"] and q["color"] == p["color"] and (q["hs"], q["vs"]) == (g["hmax"], g["vmax"]), name
        kinds.add(q.get("color", "plain"))
    assert kinds == {"plain", "ycc", "rgb", "cmyk", "ycck"}


@pytest.mark.parametrize("name,f,kw,word", F.refused(), ids=[r[0] for r in F.refused()])
def test_refused_even_with_the_keyword(name, f, kw, word):
    with pytest.raises(ValueError, match="jpeg: file 4: .*" + word.replace("(", r"\(").replace(")", r"\)")):
        jpeg.parse_jpeg(f, 4, **kw)


def test_without_the_keyword_every_refusal_is_the_parents():
    for name, f, exc, word in C.refused():
        with pytest.raises(exc, match=word):
            jpeg.parse_jpeg(f)
        with pytest.raises(exc, match=word):
            jpeg.plan([f])
    messages = {"four_components": "4 components (1 or 3)", "sampling_1x2": "sampling layout [(1, 2), (1, 1), (1, 1)] (4:4:4, 4:2:2, 4:2:0)",
                "adobe_rgb": "RGB-coded file (YCbCr only)", "ids_rgb": "RGB-coded file (YCbCr only)"}
    files = {n: f for n, f, _, _ in C.refused()}
    for name, text in messages.items():
        with pytest.raises(ValueError) as e:
            jpeg.parse_jpeg(files[name], 2)
        assert str(e.value) == f"jpeg: file 2: {text}", name
    for name, f in F.good():                                  # and every file of another layout stays refused
        if not is_plain(R.parse(f)):
            with pytest.raises(ValueError):
                jpeg.parse_jpeg(f)


def test_plain_lists_plan_byte_for_byte_as_without_the_keyword():
    files = [f for _, f in C.good()][:24] + [F.good_file("jfif_adobe0_is_ycc")]
    plain = [f for f in files if f is not files[-1]]
    for kw in (dict(), dict(mode="L", order="bgr", substreams=False), dict(mode="keep", segment_bytes=64)):
        a, b = jpeg.plan(plain, **kw), jpeg.plan(plain, all_layouts=True, **kw)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
    a = jpeg.plan(files, all_layouts=True)                    # (JFIF wins over the Adobe transform: a baseline table too)
    base = jpeg.plan(plain)                                   # (a header is a view of its table: both stay referenced)
    assert a[2].magic == base[2].magic and not any("layout" in p for p in a[0])
    prog = [f for _, f in __import__("jpegprog_cases").good()][:4]
    a, b = jpeg.plan(prog, progressive=True), jpeg.plan(prog, progressive=True, all_layouts=True)
    assert a[1].tobytes() == b[1].tobytes()


def test_a_layout_plan_has_its_own_table_and_refuses_a_mixed_list():
    files = [F.good_file(n) for n in ("cmyk_s2_33x20", "coef_410_33x17", "long_440", "keep_rgb_23x19")]
    parsed, table, hdr = jpeg.plan(files, "keep", all_layouts=True)
    base = jpeg.plan([C.good()[0][1]])
    assert hdr.magic != base[2].magic and hdr.B == 4 and hdr.table_bytes == table.size
    assert hdr.out_bytes == sum(p["W"] * p["H"] * p["ncomp"] for p in parsed)
    lens = [len(f) - p["data_off"] for f, p in zip(files, parsed)]
    want = [-(-n // 256) if p["ri"] == 0 and n >= 512 else 0 for n, p in zip(lens, parsed)]
    assert [p["segments"] for p in parsed] == want and want[2] > 0 and hdr.reserved == sum(1 for w in want if w)
    rgb = jpeg.plan(files, "RGB", all_layouts=True)
    assert rgb[2].out_bytes == sum(p["W"] * p["H"] * 3 for p in parsed)
    again = jpeg.plan(files, "keep", all_layouts=True)
    assert again[1].tobytes() == table.tobytes()              # the table depends on the headers and the lengths alone
    with pytest.raises(ValueError, match="JpegFiles splits"):
        jpeg.plan(files + [C.good()[0][1]], all_layouts=True)


def _records(n=1, **kw):
    p = jpeg.parse_jpeg(F.good_file("cmyk_s2_33x20"), 0, all_layouts=True)
    rec = np.zeros(n, dtype=np.dtype(_lib.JpegDecLayoutImage))
    rec["H"], rec["W"], rec["ncomp"], rec["color"], rec["stream_len"] = p["H"], p["W"], 4, _lib.JPEGDEC_COLOR_IDS["cmyk"], 100
    rec["h"], rec["v"] = [2, 1, 1, 1], [2, 1, 1, 1]
    rec["qt"][:, :4] = p["qt"]
    for b in range(n):
        jpeg._put_tables(rec["dc_counts"][b], rec["dc_symbols"][b], p["dc"])
        jpeg._put_tables(rec["ac_counts"][b], rec["ac_symbols"][b], p["ac"])
    for key, value in kw.items():
        rec[key] = value
    return rec


def _plan(rec, sb=0, mr=0):
    lib = _lib.load()
    n = lib.attwarp_jpegdec_layouts_table_bytes(rec.ctypes.data, len(rec))
    table = np.zeros(n, np.uint8)
    _lib.call("attwarp_jpegdec_plan_layouts", rec.ctypes.data, len(rec), table.ctypes.data, n, sb, mr)
    return table


@pytest.mark.parametrize("kw,word", [
    (dict(ncomp=2), "2 components"), (dict(ncomp=5), "5 components"), (dict(h=[5, 1, 1, 1]), "outside 1..4"), (dict(v=[1, 0, 1, 1]), "outside 1..4"),
    (dict(h=[4, 1, 1, 1], v=[2, 1, 1, 2]), "blocks per MCU"), (dict(h=[3, 2, 1, 1]), "fractional"), (dict(color=1), "colour rule"),
    (dict(color=7), "colour rule"), (dict(mode=3), "mode"), (dict(order=2), "order"), (dict(H=0), "size"), (dict(W=70000), "size"),
    (dict(restart_interval=-1), "restart interval"), (dict(H=65535, W=65535), "blocks"), (dict(H=4096, W=4112, restart_interval=1), "restart intervals"),
    (dict(stream_len=1 << 31), "2 GiB")], ids=lambda v: v if isinstance(v, str) else "")
def test_the_planner_checks_what_the_kernels_index_by(kw, word):
    _plan(_records())
    with pytest.raises(_lib.AttWarpError, match=word):
        _plan(_records(**kw))


def test_the_planner_checks_tables_and_arguments():
    rec = _records()
    rec["ac_counts"][0, 3, 0] = 3
    with pytest.raises(_lib.AttWarpError, match="over-subscribed"):
        _plan(rec)
    rec = _records()
    rec["dc_symbols"][0, 2, 1] = 16
    with pytest.raises(_lib.AttWarpError, match="DC category"):
        _plan(rec)
    rec = _records()
    rec["qt"][0, 3, 5] = 256
    with pytest.raises(_lib.AttWarpError, match="quantisation"):
        _plan(rec)
    for sb, mr in ((48, 8), (1024, 8), (256, 0), (256, 1 << 17)):
        with pytest.raises(_lib.AttWarpError, match="segment_bytes|max_rounds"):
            _plan(_records(), sb, mr)
    lib = _lib.load()
    assert lib.attwarp_jpegdec_layouts_table_bytes(_records().ctypes.data, 0) == 0
    table = _plan(_records(2), 256, 64)
    with pytest.raises(_lib.AttWarpError, match="needed"):
        _lib.call("attwarp_jpegdec_plan_layouts", _records(2).ctypes.data, 2, table.ctypes.data, table.size - 1, 0, 0)
    for entry, own in (("attwarp_jpegdec_decode", "attwarp_jpegdec_plan"), ("attwarp_jpegdec_decode_layouts", "attwarp_jpegdec_plan_layouts")):
        other = table if entry == "attwarp_jpegdec_decode" else jpeg.plan([C.good()[0][1]])[1]
        with pytest.raises(_lib.AttWarpError, match="not a table of " + own):     # checked before anything is launched
            _lib.call(entry, other.ctypes.data, 256, 256, 256, 256, 1 << 30, 256, None)


def corpus(files, S, max_rounds):
    out = [struct.pack("<III", len(files), S, max_rounds)]
    for f in files:
        p = R.parse(f)
        hv = [h for h, _ in p["samp"]] + [1] * (4 - p["ncomp"]) + [v for _, v in p["samp"]] + [1] * (4 - p["ncomp"])
        out.append(struct.pack("<III8III", p["W"], p["H"], p["ncomp"], *hv, _lib.JPEGDEC_COLOR_IDS[p["color"]], p["ri"]))
        for c in range(p["ncomp"]):
            for counts, syms in (p["dc"][c], p["ac"][c]):
                out.append(bytes(counts) + bytes(syms).ljust(256, b"\0"))
        out.append(struct.pack("<I", len(p["stream"])) + p["stream"])
    return b"".join(out)


def test_host_core_under_sanitizers_equals_the_restatement(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "jpegfmt_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "jpegfmt_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    plain = [(n, f) for n, f in C.good() if n in ("noise_64x48_s1", "grey_64x48_q100", "ri_wrap", "big_200x136")]     # the baseline layouts are layouts too
    cases = F.good() + F.malformed() + plain
    (tmp_path / "corpus.bin").write_bytes(corpus([f for _, f in cases], 256, 64))
    r = subprocess.run([str(exe), str(tmp_path / "corpus.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases) + 1 and lines[-1].startswith("arith ")
    accepted, rounds, period = {}, {}, {}
    for (name, f), line in zip(cases, lines):
        st, _, info = R.decode(f)
        got = tuple(int(x) for x in line.split())
        assert got[:4] == (0, st, info["crc"], info["nunits"]), name
        assert got[4] == got[5], name                         # what the sub-streams accept, they decode as the sequential walk
        accepted[name], rounds[name], period[name] = got[4], got[6], got[7]
    assert all(accepted[n] for n, _ in F.long_plain()), accepted
    # Pillow's CMYK files use ONE pair of tables for all four components: no decoder can tell their slots apart, the state
    # carries none (period 1), and the rounds do not grow with the segments (38 here) as they would if it did
    assert period["long_cmyk_s2"] == period["long_cmyk_s0"] == 1 and period["long_410"] == 12 - 2 and period["long_440"] == 4
    assert len(R.parse(F.good_file("long_cmyk_s2"))["stream"]) // 256 >= 36 and all(rounds[n] <= 12 for n, _ in F.long_plain()), rounds
    assert not any(accepted[n] for n, _ in F.malformed() if R.decode(dict(F.malformed())[n])[0] not in (D.OK, D.E_NO_EOI))
