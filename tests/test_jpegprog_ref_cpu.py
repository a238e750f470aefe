"""CPU tests (no device) of the progressive JPEG restatement (tests/jpegprog_ref.py) and of the host's part of the decoder
(attwarp_amd.jpeg.parse_jpeg / plan with ``progressive=True``): every good file is proven from its own bytes against
Pillow, the transcoder independently of the restatement, every case reaches the branch it is named for, and the marker
walk and the planner agree with the restatement."""
import io

import numpy as np
import pytest
from PIL import Image

import jpegprog_cases as C
import jpegprog_ref as R


def pil(f, mode):
    a = np.asarray(Image.open(io.BytesIO(f)).convert(mode))
    return a if a.ndim == 3 else a[:, :, None]


@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_restatement_equals_pillow_on_pillows_own_files(mode):
    for name, f in C.pillow():
        st, px, _ = R.decode(f, mode)
        assert st == R.OK and np.array_equal(px, pil(f, mode)), name


def test_transcoded_files_equal_pillow_and_their_baseline_source():
    for name, f, src in C.transcoded() + [("scan_limit",) + C.scan_limit()]:
        for mode in ("RGB", "L"):
            st, px, _ = R.decode(f, mode)
            mine = pil(f, mode)
            assert st == R.OK and np.array_equal(px, mine), name
            assert np.array_equal(mine, pil(src, mode)), name       # pins the transcoder without the restatement


def test_progressive_and_baseline_encodings_of_one_array_decode_alike():
    a = C.noise(33, 20, 3, 5)
    for kw in (dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(subsampling=2, optimize=True)):
        assert np.array_equal(pil(C.save(a, quality=75, progressive=True, **kw), "RGB"), pil(C.save(a, quality=75, **kw), "RGB"))


def test_levels_of_pillows_scripts():
    files = dict(C.pillow())
    assert R.decode(files["17x33_420_q75"])[2]["levels"] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2]
    assert R.decode(files["grey_40x52_q75"])[2]["levels"] == [0, 0, 0, 1, 1, 2]


def _counters(f):
    R._CACHE.pop(bytes(f), None)
    R.reset_counters()
    st = R.decode(f)[0]
    return st, dict(R.COUNT)


def test_every_case_reaches_its_branch():
    files = dict(C.pillow())
    st, c = _counters(files["grey_40x52_q100"])
    assert st == 0 and c["corr_place"] and c["corr_eob"] and c["plus"] and c["minus"] and c["dc_refine_set"] and c["eob_first"]
    st, c = _counters(files["grey_40x52_q75"])
    assert st == 0 and c["zrl_first"]
    tr = {n: f for n, f, _ in C.transcoded()}
    st, c = _counters(tr["three_refinements"])
    assert st == 0 and c["corr_zrl"] and c["corr_eob"] and c["corr_place"]
    f, p, planes = C.eob_run_case()
    st, c = _counters(f)
    assert st == 0 and c["max_eobrun"] == 32767 and c["corr_eob"] >= 2
    got = R.decode(f)[2]["planes"]
    assert np.array_equal(got[0], planes[0])
    assert np.array_equal(R.decode(f, "L")[1], pil(f, "L"))
    name, h = C.hostile()[0]
    st, px, info = R.decode(h)
    assert st == 0 and int(info["planes"][0][0, 0, 0]) != 0
    p = R.parse(h)
    assert p["scans"][0]["al"] == 13


def test_malformed_statuses():
    want = {"cut_in_dc_first": R.E_TRUNCATED, "cut_in_ac_first": R.E_TRUNCATED, "cut_in_ac_refine": R.E_TRUNCATED,
            "cut_in_dc_refine": R.E_TRUNCATED, "no_eoi": R.E_NO_EOI, "rst_removed": R.E_RESTART, "rst_doubled": R.E_RESTART,
            "rst_renumbered": R.E_RESTART, "no_code_dc": R.E_HUFFMAN, "no_code_ac": R.E_HUFFMAN, "run_past_se": R.E_COEFF,
            "zrl_past_se": R.E_COEFF, "refine_s2": R.E_COEFF, "two_scans_fail": R.E_COEFF}
    got = {n: R.decode(f)[0] for n, f in C.malformed()}
    assert got == want


def test_refusals_by_their_word_in_the_restatement_and_the_host():
    from attwarp_amd import jpeg
    for name, f, word in C.refused():
        with pytest.raises(ValueError, match=word):
            R.parse(f)
        with pytest.raises(ValueError, match=word):
            jpeg.parse_jpeg(f, 0, progressive=True)
    assert len(R.parse(C.scan_limit()[0])["scans"]) == R.MAX_SCANS == jpeg.JPEGDEC_MAX_SCANS
    # a multi-scan sequential file stays refused, with and without the keyword
    f = {n: x for n, x, _ in C.transcoded()}["dc_separate"]
    seq = f.replace(b"\xff\xc2", b"\xff\xc0", 1)
    for kw in ({}, {"progressive": True}):
        with pytest.raises(ValueError, match="more than one scan"):
            jpeg.parse_jpeg(seq, 0, **kw)


def test_without_the_keyword_every_progressive_file_is_refused():
    from attwarp_amd import jpeg
    for name, f in C.good() + C.malformed():
        with pytest.raises(ValueError, match="progressive"):
            jpeg.parse_jpeg(f)
    with pytest.raises(ValueError, match="progressive"):
        jpeg.plan([C.good()[0][1]])


def test_host_walk_and_planner_against_the_restatement():
    from attwarp_amd import _lib, jpeg
    named = C.good() + C.malformed()
    files = [f for _, f in named]
    for name, f in named:
        a, b = jpeg.parse_jpeg(f, 0, progressive=True), R.parse(f)
        assert a["progressive"] and a["levels"] == b["levels"] == jpeg.scan_levels(a["scans"]) and a["units"] == b["units"], name
        assert (a["W"], a["H"], a["ncomp"], a["hs"], a["vs"], a["data_off"]) == (b["W"], b["H"], b["ncomp"], b["hs"], b["vs"], b["first"])
        assert [list(q) for q in a["qt"]] == b["qt"]
        for x, y in zip(a["scans"], b["scans"]):
            assert all(x[k] == y[k] for k in ("comps", "ss", "se", "ah", "al", "ri", "off", "units")), name
            assert [(list(c), list(s)) for c, s in x["tables"]] == [(list(c), list(s)) for c, s in y["tables"]], name
            assert jpeg.scan_geometry(a, x["comps"])[:2] == R.scan_mcus(b, y["comps"])[:2]
    # 17 pixels wide at 4:2:0: three covered luma blocks per row in rows of four
    p = R.parse(dict(C.pillow())["17x33_420_q75"])
    assert R.scan_mcus(p, [0])[:2] == (3, 15) and R.scan_mcus(p, [0, 1, 2])[:2] == (2, 6) and R.scan_mcus(p, [1])[:2] == (2, 6)
    # the planned table: header sums, one record per scan sorted by (level, image, position), waves per level
    for by_level in (True, False):
        parsed, table, h = jpeg.plan(files, progressive=True, levels=by_level)
        assert h.B == len(files) and h.total_units == len(files) and h.reserved == 0
        assert h.out_bytes == sum(p["W"] * p["H"] * 3 for p in parsed)
        off = int(h.off_images) + len(files) * (_lib.JPEGDEC_RECORD_BYTES + 32)
        assert off == _lib.load().attwarp_jpegdec_table_bytes(table.ctypes.data, len(files))       # the record size the views rest on
        head = table[off:off + 16].view(np.int32)
        nscans, nlevels, units = int(head[1]), int(head[2]), int(head[3])
        lv = [[l if by_level else i for i, l in enumerate(p["levels"])] for p in parsed]
        assert nscans == sum(len(p["scans"]) for p in parsed) and units == sum(p["units"] for p in parsed)
        assert nlevels == max(max(l) for l in lv) + 1
        waves = table[off + 48 + 4 * 65:off + 48 + 8 * 65].view(np.int32)
        for l in range(nlevels):
            assert int(waves[l]) == sum(s["units"] for p, ls in zip(parsed, lv) for s, x in zip(p["scans"], ls) if x == l)
    with pytest.raises(ValueError, match="JpegFiles splits"):
        jpeg.plan([files[0], C._colour_source()], progressive=True)


def test_units_over_all_scans_are_limited():
    from attwarp_amd import jpeg
    # 2048 x 2048 grey, a restart interval of one block in two scans: 2 x 65536 units
    p = dict(W=2048, H=2048, ncomp=1, hs=1, vs=1, ri=0, qt=[[1] * 64])
    f = R.transcode(p, None, [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0)], ri=[1, 1], encode=False)
    with pytest.raises(ValueError, match="size limit"):
        jpeg.parse_jpeg(f, 0, progressive=True)
    with pytest.raises(ValueError, match="size limit"):
        R.parse(f)
