"""The layout scans' sub-stream core (attwarp_amd/csrc/jpegscan_sync_blocks.hpp) on the CPU under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/jpegscan_sync_host_main.cpp is compiled as a stand-alone program and
run as a child process over the corpus of tests/jpegscan_sync_cases.py and the malformed files, at 32 and 128 bytes per
segment.  The program itself compares, after every scan, the coefficients of the sub-stream routes with those of
js_decode_unit's walk and refuses a scan that is accepted where the walk reports a status; here its statuses and CRCs are
held against jpegscan_ref's and its records (route, segments, rounds, accepted) against jpegscan_sync_ref's, exactly.  Also
the planner through the C ABI, which needs no device: the table without sub-streams, the cut rule at its edges, the period
it stores, its refusals, and the declarations."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpegscan_ref as R
import jpegscan_sync_cases as SC
import jpegscan_sync_ref as Y
from attwarp_amd import _lib, jpeg
from test_jpegscan_host_cpu import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path_factory.mktemp("jpegscan_sync") / "jpegscan_sync_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "jpegscan_sync_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    return exe


def run(program, tmp_path, named, segment_bytes, max_rounds):
    (tmp_path / "corpus.bin").write_bytes(corpus([f for _, f in named]))
    r = subprocess.run([str(program), str(tmp_path / "corpus.bin"), str(segment_bytes), str(max_rounds)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = [[int(x) for x in line.split()] for line in r.stdout.strip().split("\n")]
    assert len(lines) == len(named)
    return lines


@pytest.mark.parametrize("segment_bytes", [32, 128])
def test_host_core_under_sanitizers_equals_the_restatement(program, tmp_path, segment_bytes):
    named = SC.good() + SC.malformed()
    cut = accepted = 0
    routes = set()
    for (name, f), line in zip(named, run(program, tmp_path, named, segment_bytes, 64)):
        st, _, info = R.decode(f)
        assert (line[0], line[1]) == (st, info["crc"]), name
        want, _, exact = Y.records(f, segment_bytes, 64)
        rec = np.array(line[2:]).reshape(len(want), 5)
        ran = True
        for i, ((route, nseg, rounds, acc, crc), w, ex) in enumerate(zip(rec.tolist(), want, exact)):
            ran = ran and (st != R.E_RESTART) and (i == 0 or rec[i - 1][4] != 0)     # the program stops behind the first failing scan
            if not ran:
                assert (route, nseg, rounds, acc, crc) == (0, 0, 0, 0, 0), (name, i)
                continue
            assert ex and (route, nseg, rounds, acc) == w, (name, i, w)
            if st == 0:
                assert crc != 0 and acc == (route != 0), (name, i)          # every cut scan of a good file is accepted
            cut += route != 0
            accepted += acc
            routes.add(route)
        if st == 0:
            assert rec[-1][4] == info["crc"], name
    assert routes == {0, 1, 2, 3, 4} and cut > (100 if segment_bytes == 32 else 20), (cut, accepted, routes)


def test_a_scan_that_needs_more_rounds_falls_back(program, tmp_path):
    named = [("ten_blocks", SC.ten_blocks()), ("padded_411", SC.padded_plane())]
    for (name, f), line in zip(named, run(program, tmp_path, named, 32, 1)):
        st, _, info = R.decode(f)
        assert (line[0], line[1]) == (st, info["crc"]), name
        rec = np.array(line[2:]).reshape(-1, 5)
        assert [tuple(r[:4]) for r in rec.tolist()] == Y.records(f, 32, 1)[0], name
        first = [r for r in rec if r[0] in (1, 3) and r[1] > 2]
        assert first and all(r[2] == 1 and r[3] == 0 for r in first), name      # one round cannot settle three segments
        assert all(r[3] == 1 for r in rec if r[0] in (2, 4)), name             # the refinements take no rounds


# ---- the planner through the C ABI --------------------------------------------------------------------------------------------------
def planner_calls(files, during, **kw):
    """jpeg.plan(files, all_scans=True, **kw) -> its result; during(size, planner) runs while the records the two calls point
    to are alive."""
    inner = jpeg.planned_table

    def spy(size, planner, *a, **k):
        during(size, planner)
        return inner(size, planner, *a, **k)

    jpeg.planned_table = spy
    try:
        return jpeg.plan(files, all_scans=True, **kw)
    finally:
        jpeg.planned_table = inner


def trailer(table, header):
    """(ncut, info_off, level_cut0, level_tables, per scan record (seg_off, mask_off, nseg, segment_bytes, max_rounds, slot, cut, period))
    of a table planned with sub-streams, read off its bytes: behind the JsScan records."""
    off_plain = header["plain_bytes"]
    raw = bytes(table[off_plain:])
    magic, ncut, info_off = np.frombuffer(raw[:16], "<u4,<u4,<u8")[0]
    assert magic == 0x4745504F
    cut0 = np.frombuffer(raw[16:16 + 66 * 4], "<u4")
    tabs = np.frombuffer(raw[16 + 66 * 4:16 + 132 * 4], "<u4")
    recs = np.frombuffer(raw[16 + 132 * 4:], np.dtype([("seg_off", "<u8"), ("mask_off", "<u8"), ("nseg", "<u4"), ("segment_bytes", "<u4"),
                                                        ("max_rounds", "<u4"), ("slot", "<u4"), ("cut", "<u4"), ("period", "<u4"), ("pad", "<u4", 6)]))
    return int(ncut), int(info_off), cut0, tabs, recs


def test_header_and_library_declare_the_entry_points():
    text = open(os.path.join(ROOT, "include", "attwarp.h")).read()
    for name in ("attwarp_jpegdec_plan_layout_scans_ex", "attwarp_jpegdec_layout_scans_table_bytes_ex"):
        assert re.search(r"ATTWARP_API\s+\w+\s+" + name + r"\(", text), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load_tuning(), name), name


@pytest.mark.parametrize("levels", [True, False])
def test_ex_without_substreams_is_plan_layout_scans_byte_for_byte(levels):
    lib = _lib.load()
    files = [f for _, f in SC.good()[:6]] + [SC.sequential(), SC.two_bands()]
    seen = {}

    def during(size, planner):
        assert planner[0] == "attwarp_jpegdec_plan_layout_scans" and size[0] == "attwarp_jpegdec_layout_scans_table_bytes"
        _, rp, B, srec, nscans, _, by_level = planner
        n = lib.attwarp_jpegdec_layout_scans_table_bytes_ex(rp, ctypes.c_int(B), ctypes.c_int(nscans), ctypes.c_int(0), ctypes.c_int(0))
        buf = (ctypes.c_uint8 * n)(*([0x5A] * n))
        assert lib.attwarp_jpegdec_plan_layout_scans_ex(rp, ctypes.c_int(B), ctypes.c_void_p(srec), ctypes.c_int(nscans), buf, ctypes.c_size_t(n),
                                                        ctypes.c_int(by_level), ctypes.c_int(0), ctypes.c_int(0), None) == 0
        seen["ex"] = bytes(buf)

    _, table, header = planner_calls(files, during, levels=levels)
    n = len(seen["ex"])
    assert seen["ex"] == bytes(table)
    assert lib.attwarp_jpegdec_scan_info_offset(table.ctypes.data) == 0
    on = jpeg.plan(files, all_scans=True, levels=levels, scan_substreams=True, segment_bytes=32)
    assert bytes(on[1])[64:n] == bytes(table)[64:n]         # behind the first header (sizes), every record is the parent's
    assert lib.attwarp_jpegdec_scan_info_offset(on[1].ctypes.data) >= int(header.scratch_bytes) and int(on[2].scratch_bytes) > int(header.scratch_bytes)


def test_the_planner_cuts_what_the_rule_says_and_stores_the_period():
    files = [SC.smallest(True), SC.smallest(False), SC.sequential(), SC.ten_blocks()] + [f for _, f, _ in SC.table_sequences()]
    parsed, table, header = jpeg.plan(files, all_scans=True, scan_substreams=True, segment_bytes=32)
    assert parsed[0]["scan_segments"][1] == 2 and parsed[1]["scan_segments"][1] == 0          # 64 bytes / 63 bytes
    assert parsed[2]["scan_segments"] == [0, 0, 0]                                            # a sequential scan is never cut
    _, off, hoff = jpeg.plan(files, all_scans=True)
    ncut, info_off, cut0, tabs, recs = trailer(np.frombuffer(bytes(table), np.uint8), dict(plain_bytes=len(bytes(off))))
    flat = [n for p in parsed for n in p["scan_segments"]]
    assert ncut == sum(n > 0 for n in flat) and info_off == jpeg._lib.load().attwarp_jpegdec_scan_info_offset(table.ctypes.data)
    by_slot = {int(r["slot"]): r for r in recs}
    assert sorted(by_slot) == list(range(len(flat)))
    want_period = [q for f in files for _, _, q in Y.plan(R.parse(f), 32)]
    for i, n in enumerate(flat):
        r = by_slot[i]
        assert (int(r["nseg"]), int(r["segment_bytes"]), int(r["max_rounds"]), int(r["period"])) == (n, 32, jpeg.MAX_ROUNDS, want_period[i]), i
        assert (int(r["seg_off"]) >= info_off + 32 * len(flat)) == (n > 0) and int(r["seg_off"]) % 256 == 0, i
    assert {4, 5, 2, 1} <= set(want_period)
    levels = max(max(p["levels"]) for p in parsed) + 1
    assert cut0[0] == 0 and cut0[levels] == ncut and all(1 <= t <= 4 for t in tabs[:levels]) and tabs[0] == 4
    cuts = sorted(int(r["cut"]) for r in recs[:ncut])
    assert cuts == sorted(i for i, r in enumerate(recs) if r["nseg"] > 0)
    auto = jpeg.plan(files, all_scans=True, scan_substreams="auto", segment_bytes=32)[0]
    for pa, pt in zip(auto, parsed):                         # "auto": the kinds of AUTO_LAYOUT_SCAN_KINDS as with True, no other scan
        assert pa["scan_segments"] == [n if not s.get("sequential") and jpeg.scan_kind(s) in jpeg.AUTO_LAYOUT_SCAN_KINDS else 0
                                       for s, n in zip(pt["scans"], pt["scan_segments"])]
    for bad in ("yes", 0, 1, None):
        with pytest.raises(ValueError):
            jpeg.plan(files, all_scans=True, scan_substreams=bad)
    with pytest.raises(ValueError):
        jpeg.plan(files, all_scans=True, scan_substreams=True, segment_bytes=48)


def test_the_planner_refuses_bad_arguments():
    files = [SC.ten_blocks()]
    ran = []
    planner_calls(files, lambda size, planner: ran.append(_refusals(size, planner)), scan_substreams=True, segment_bytes=32)
    assert ran == [True]


def _refusals(size, planner):
    assert planner[0] == "attwarp_jpegdec_plan_layout_scans_ex" and size[0] == "attwarp_jpegdec_layout_scans_table_bytes_ex"
    _, rp, B, srec, nscans, _, by_level, sb, mr, slen = planner
    lib = _lib.load()
    n = lib.attwarp_jpegdec_layout_scans_table_bytes_ex(rp, B, nscans, sb, mr)
    plain = lib.attwarp_jpegdec_layout_scans_table_bytes(rp, B, nscans)
    assert n > plain > 0
    table = np.zeros(n, np.uint8)
    lens = np.ctypeslib.as_array(ctypes.cast(slen, ctypes.POINTER(ctypes.c_uint64)), (nscans,)).copy()

    def call(table_bytes=n, sb=sb, mr=mr, data=lens):
        _lib.call("attwarp_jpegdec_plan_layout_scans_ex", rp, B, srec, nscans, table.ctypes.data, table_bytes, by_level, sb, mr,
                  None if data is None else data.ctypes.data)

    call()
    for kw, word in ((dict(sb=48), "power of two"), (dict(sb=16), "power of two"), (dict(sb=1024), "power of two"), (dict(mr=0), "max_rounds"),
                     (dict(mr=65537), "max_rounds"), (dict(data=None), "null data_bytes"), (dict(table_bytes=n - 1), "needed"),
                     (dict(table_bytes=plain), "needed")):
        with pytest.raises(_lib.AttWarpError, match=word):
            call(**kw)
    over = lens.copy()
    over[0] = 1 << 40
    with pytest.raises(_lib.AttWarpError, match="jpegdec_plan_layout_scans_ex: scan 0: data outside the image's"):
        call(data=over)
    none = np.zeros_like(lens)                               # no data: nothing is cut, the trailer says so
    call(data=none)
    assert trailer(table, dict(plain_bytes=plain))[0] == 0
    return True
