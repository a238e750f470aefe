"""The progressive scans' sub-stream core (attwarp_amd/csrc/jpegprog_sync_blocks.hpp) on the CPU under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/jpegprog_sync_host_main.cpp is compiled as a stand-alone program and
run as a child process over both corpora, the limit files and the malformed files, at 32 and 128 bytes per segment.  The
program itself compares, after every scan, the coefficients of the sub-stream routes with those of the sequential walk and
refuses a scan that is accepted where the walk reports a status; here its statuses and CRCs are held against the
restatement's (jpegprog_ref.py) and its records (route, segments, rounds, accepted) against jpegprog_sync_ref.py's, exactly.  Also the planner, which needs no device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpegprog_cases as C
import jpegprog_ref as R
import jpegprog_sync_cases as SC
import jpegprog_sync_ref as Y
from test_jpegprog_host_cpu import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path_factory.mktemp("jpegprog_sync") / "jpegprog_sync_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "jpegprog_sync_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    return exe


def named_files():
    return (C.good() + SC.limits() + SC.larger() + C.malformed() +
            [("eob_run", C.eob_run_case()[0]), ("eob_run_textured", SC.eob_run_textured()), ("most_segments", SC.most_segments(0)),
             ("one_segment_more", SC.most_segments(1))])


def run(program, tmp_path, named, segment_bytes, max_rounds):
    (tmp_path / "corpus.bin").write_bytes(corpus([f for _, f in named]))
    r = subprocess.run([str(program), str(tmp_path / "corpus.bin"), str(segment_bytes), str(max_rounds)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = [[int(x) for x in line.split()] for line in r.stdout.strip().split("\n")]
    assert len(lines) == len(named)
    return lines


@pytest.mark.parametrize("segment_bytes", [32, 128])
def test_host_core_under_sanitizers_equals_the_restatement(program, tmp_path, segment_bytes):
    named = named_files()
    cut = accepted = 0
    routes = set()
    for (name, f), line in zip(named, run(program, tmp_path, named, segment_bytes, 4096)):
        st, _, info = R.decode(f)
        assert (line[0], line[1]) == (st, info["crc"]), name
        big = name in ("eob_run", "eob_run_textured")          # (their rounds in Python take too long: the records by the plan alone)
        want = [(r, n, None, None) for r, n in Y.plan(R.parse(f), segment_bytes)] if big else Y.records(f, segment_bytes, 4096)[0]
        rec = np.array(line[2:]).reshape(len(want), 5)
        ran = True
        for i, ((route, nseg, rounds, acc, crc), w) in enumerate(zip(rec.tolist(), want)):
            ran = ran and (st != R.E_RESTART) and (i == 0 or rec[i - 1][4] != 0)     # the program stops behind the first failing scan
            if not ran:
                assert (route, nseg, rounds, acc, crc) == (0, 0, 0, 0, 0), (name, i)
                continue
            assert (route, nseg) == w[:2], (name, i)
            if not big:
                assert (rounds, acc) == w[2:], (name, i, w)
            if st == 0:
                assert crc != 0 and acc == (route != 0), (name, i)          # every cut scan of a good file is accepted
            cut += route != 0
            accepted += acc
            routes.add(route)
        if st == 0:
            assert rec[-1][4] == info["crc"], name
    assert routes == {0, 1, 2, 3, 4} and accepted >= cut - 8 and cut > (150 if segment_bytes == 32 else 20), (cut, accepted)


def test_a_scan_that_needs_more_rounds_falls_back(program, tmp_path):
    named = SC.larger()[:2]
    for (name, f), line in zip(named, run(program, tmp_path, named, 32, 1)):
        st, _, info = R.decode(f)
        assert (line[0], line[1]) == (st, info["crc"]), name
        rec = np.array(line[2:]).reshape(-1, 5)
        assert [tuple(r[:4]) for r in rec.tolist()] == Y.records(f, 32, 1)[0], name
        first = [r for r in rec if r[0] in (1, 3) and r[1] > 2]
        assert first and all(r[2] == 1 and r[3] == 0 for r in first), name      # one round cannot settle three segments
        assert all(r[3] == 1 for r in rec if r[0] in (2, 4)), name             # the refinements take no rounds


def test_planner_cuts_what_the_issue_says():
    from attwarp_amd import jpeg
    files = [SC.smallest(True), SC.smallest(False), SC.most_segments(0), SC.most_segments(1), dict(C.pillow())["17x33_420_rows"]]
    parsed, table, header = jpeg.plan(files, progressive=True, scan_substreams=True, segment_bytes=32)
    assert parsed[0]["scan_segments"][1] == 2 and parsed[1]["scan_segments"][1] == 0
    assert parsed[2]["scan_segments"][1] == 16384 and parsed[3]["scan_segments"][1] == 0
    assert not any(parsed[4]["scan_segments"][i] for i, s in enumerate(parsed[4]["scans"]) if s["units"] > 1)
    _, off, hoff = jpeg.plan(files, progressive=True)
    assert len(bytes(table)) > len(bytes(off)) and int(header.scratch_bytes) > int(hoff.scratch_bytes)
    auto = jpeg.plan(files, progressive=True, scan_substreams="auto", segment_bytes=32)[0]
    for pa, pt in zip(auto, parsed):                         # "auto": the kinds of AUTO_SCAN_KINDS as with True, no other scan
        assert pa["scan_segments"] == [n if jpeg.scan_kind(s) in jpeg.AUTO_SCAN_KINDS else 0 for s, n in zip(pt["scans"], pt["scan_segments"])]
    default = jpeg.plan(files, progressive=True, scan_substreams=True)[0]
    assert default[2]["scan_segments"][1] == -(-16384 * 32 // jpeg.SEGMENT_BYTES)
    for bad in ("yes", 0, 1, None):
        with pytest.raises(ValueError):
            jpeg.plan(files, progressive=True, scan_substreams=bad)
    with pytest.raises(ValueError):
        jpeg.plan(files, progressive=True, scan_substreams=True, segment_bytes=48)


def identity_files():
    return [f for _, f in C.pillow()[2:45:7]] + [f for _, f, _ in C.transcoded()[:8]] + [SC.two_bands(), SC.smallest(True)]


def keyword_off_tables(files, levels, lib):
    """plan(files, progressive=True) without the keyword -> (its table, the table `lib`'s attwarp_jpegdec_plan_scans writes for the
    same records, the table attwarp_jpegdec_plan_scans_ex writes for (0, 0, NULL) or None where `lib` has no such entry point)."""
    import ctypes
    from attwarp_amd import jpeg
    seen = {}
    inner = jpeg.planned_table

    def spy(size, planner, *a, **k):
        assert planner[0] == "attwarp_jpegdec_plan_scans" and size[0] == "attwarp_jpegdec_scans_table_bytes"
        _, rp, B, srec, nscans, _, by_level = planner
        lib.attwarp_jpegdec_scans_table_bytes.restype = ctypes.c_size_t
        n = lib.attwarp_jpegdec_scans_table_bytes(rp, ctypes.c_int(B), ctypes.c_int(nscans))
        buf = (ctypes.c_uint8 * n)(*([0xA5] * n))
        assert lib.attwarp_jpegdec_plan_scans(rp, ctypes.c_int(B), ctypes.c_void_p(srec), ctypes.c_int(nscans), buf, ctypes.c_size_t(n), ctypes.c_int(by_level)) == 0
        seen["plain"] = bytes(buf)
        seen["ex"] = None
        if hasattr(lib, "attwarp_jpegdec_plan_scans_ex"):
            lib.attwarp_jpegdec_scans_table_bytes_ex.restype = ctypes.c_size_t
            assert lib.attwarp_jpegdec_scans_table_bytes_ex(rp, ctypes.c_int(B), ctypes.c_int(nscans), ctypes.c_int(0), ctypes.c_int(0)) == n
            buf2 = (ctypes.c_uint8 * n)(*([0x5A] * n))
            assert lib.attwarp_jpegdec_plan_scans_ex(rp, ctypes.c_int(B), ctypes.c_void_p(srec), ctypes.c_int(nscans), buf2, ctypes.c_size_t(n),
                                                     ctypes.c_int(by_level), ctypes.c_int(0), ctypes.c_int(0), None) == 0
            seen["ex"] = bytes(buf2)
        return inner(size, planner, *a, **k)

    jpeg.planned_table = spy
    try:
        _, table, _ = jpeg.plan(files, progressive=True, levels=levels)
    finally:
        jpeg.planned_table = inner
    return bytes(table), seen["plain"], seen["ex"]


@pytest.mark.parametrize("levels", [True, False])
def test_keyword_off_table_is_the_parents_byte_for_byte(levels):
    """The table of plan(progressive=True) without the keyword = attwarp_jpegdec_plan_scans' = attwarp_jpegdec_plan_scans_ex's for
    (0, 0, NULL), and its CRC-32 is the one recorded from the library of the commit before the sub-streams
    (tests/golden/jpegprog_plan_scans_crc.json: the parent's attwarp_jpegdec_plan_scans over the same records)."""
    import json
    import zlib
    from attwarp_amd import _lib
    table, plain, ex = keyword_off_tables(identity_files(), levels, _lib.load())
    assert ex is not None and table == plain == ex
    with open(os.path.join(HERE, "golden", "jpegprog_plan_scans_crc.json")) as fh:
        golden = json.load(fh)
    assert len(table) == golden[f"levels_{int(levels)}"]["bytes"] and zlib.crc32(table) == golden[f"levels_{int(levels)}"]["crc32"]
