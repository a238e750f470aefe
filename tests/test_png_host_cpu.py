"""The PNG encoder's host side without a GPU.  (1) The host / device pieces of attwarp_amd/csrc/png_blocks.hpp
(png_length_symbol, png_filter, crc_mulmod, crc_xpow8, crc_bytes, png_rows_per_segment) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/png_host_main.cpp is compiled as a stand-alone program and run as a child process; it must
end clean.  (2) The planner's refusals (attwarp_png_bound / attwarp_png_table_bytes / attwarp_png_plan, called with fake
pointers: nothing is launched): 2 GiB, B > 2^20, more than 2^24 segments, the pitch, and the largest shapes below each limit."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import png_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_host_pieces_under_sanitizers(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "png_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "png_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[:2] == ["png_host", "ok"] and int(words[2]) > 256 ** 3


# ---- the planner ----------------------------------------------------------------------------------------------------------------
def records(shapes, pitch=None):
    from attwarp_amd import _lib
    rec = np.zeros(len(shapes), dtype=np.dtype(_lib.PngImage))
    s = np.asarray(shapes, np.int64).reshape(-1, 3)
    rec["src"] = 0x1000                                      # never dereferenced: nothing is launched
    rec["H"], rec["W"], rec["C"] = s[:, 0], s[:, 1], s[:, 2]
    rec["pitch"] = s[:, 1] * s[:, 2] if pitch is None else pitch
    rec["order"], rec["filter"] = _lib.RGB, _lib.PNG_FILTER_IDS["sub"]
    return rec


def table_bytes(rec):
    from attwarp_amd import _lib
    return _lib.load().attwarp_png_table_bytes(ctypes.c_void_p(rec.ctypes.data), len(rec))


def plan(rec):
    from attwarp_amd import _lib
    n = table_bytes(rec)
    assert n > 0
    table = np.zeros(n, np.uint8)
    _lib.call("attwarp_png_plan", ctypes.c_void_p(rec.ctypes.data), len(rec), table.ctypes.data, n)
    h = _lib.PngHeader.from_address(table.ctypes.data)
    return (h.B, h.nseg, h.out_bytes, h.table_bytes), table


def bound(H, W, C):
    """R.bound in closed form (for the bisection; the results are checked against R.bound itself)."""
    rb = 1 + W * C
    return R.FILE_OVERHEAD + H * rb + 5 * -(-H // R.rows_per_segment(rb))


def test_two_gib_bound():
    from attwarp_amd import _lib
    lib = _lib.load()
    W = R.MAX_ROW_BYTES - 1
    assert lib.attwarp_png_bound(90000, W, 1) == 0 and R.bound(90000, W, 1) >= 1 << 31
    assert table_bytes(records([(90000, W, 1)])) == 0 and b"2 GiB" in lib.attwarp_last_error()
    with pytest.raises(_lib.AttWarpError):
        _lib.call("attwarp_png_plan", ctypes.c_void_p(records([(90000, W, 1)]).ctypes.data), 1, np.zeros(64, np.uint8).ctypes.data, 64)
    # the tallest image below the limit, for the widest grey and RGB rows and for H x 1 (1024 rows per segment)
    for W, C in ((R.MAX_ROW_BYTES - 1, 1), ((R.MAX_ROW_BYTES - 1) // 3, 3), (1, 1)):
        H, hi = 1, 1 << 31                                     # bisect: bound(H) < 2^31 <= bound(hi)
        while hi - H > 1:
            mid = (H + hi) // 2
            H, hi = (mid, hi) if bound(mid, W, C) < 1 << 31 else (H, mid)
        assert R.bound(H, W, C) < 1 << 31 <= R.bound(H + 1, W, C)
        assert lib.attwarp_png_bound(H, W, C) == R.bound(H, W, C) and lib.attwarp_png_bound(H + 1, W, C) == 0
        assert table_bytes(records([(H + 1, W, C)])) == 0
        (B, nseg, out_bytes, nbytes), _ = plan(records([(H, W, C)]))
        assert (B, nseg, out_bytes) == (1, len(R.segments(H, 1 + W * C)), R.bound(H, W, C))


def test_batch_size_limit():
    from attwarp_amd import _lib
    lib = _lib.load()
    B = 1 << 20
    assert table_bytes(records([(1, 1, 1)] * (B + 1))) == 0 and b"2^20" in lib.attwarp_last_error()
    (b, nseg, out_bytes, nbytes), table = plan(records([(1, 1, 1)] * B))      # the largest batch: 2^20 files of 75 bytes at most
    assert (b, nseg, out_bytes) == (B, B, B * R.bound(1, 1, 1))
    assert table_bytes(records([(1, 1, 1)])[:0]) == 0                          # B = 0


def test_segment_count_limit():
    """More than 2^24 segments in one call are refused by attwarp_png_table_bytes, which only counts.  Exactly 2^24 are
    accepted there; PLANNING them would take a table of 2^24 x 32 bytes = 512 MiB (plus 80 MiB of image records), so the
    largest planned batch here stays at 2^21 segments (64 MiB) and the count alone is checked at the limit."""
    from attwarp_amd import _lib
    lib = _lib.load()
    B = 1 << 20
    rows = R.SEG_MAX_ROWS                                     # H x 1 grey: 1024 rows per segment
    assert len(R.segments(16 * rows, 2)) == 16 and len(R.segments(16 * rows + 1, 2)) == 17
    rec = records([(16 * rows, 1, 1)] * B)                   # 2^24 segments exactly
    n = table_bytes(rec)
    assert n >= (1 << 24) * 32 + B * 80
    rec["H"][B // 2] += 1                                    # one more
    assert table_bytes(rec) == 0 and b"segments" in lib.attwarp_last_error()
    (b, nseg, out_bytes, nbytes), table = plan(records([(2 * rows, 1, 1)] * B))
    assert (b, nseg, out_bytes) == (B, 2 * B, B * R.bound(2 * rows, 1, 1))


def test_pitch_limit():
    from attwarp_amd import _lib
    lib = _lib.load()
    for H, W, C in ((3, 5, 3), (2, R.MAX_ROW_BYTES - 1, 1), (7, 1, 1)):
        (b, nseg, out_bytes, nbytes), _ = plan(records([(H, W, C)], pitch=W * C))          # rows back to back
        assert out_bytes == R.bound(H, W, C)
        assert table_bytes(records([(H, W, C)], pitch=W * C - 1)) == 0 and b"pitch" in lib.attwarp_last_error()
    ok = records([(3, 5, 3), (3, 5, 3)])
    ok["pitch"][1] = 14                                      # the second image of a batch
    assert table_bytes(ok) == 0


def test_row_limit_and_mixed_batch_bound():
    shapes = [(2, R.MAX_ROW_BYTES - 1, 1), (2, (R.MAX_ROW_BYTES - 1) // 3, 3), (1025, 1, 1), (1, 1, 3)]
    (b, nseg, out_bytes, nbytes), _ = plan(records(shapes))
    assert out_bytes == sum(R.bound(*s) for s in shapes) and nseg == sum(len(R.segments(H, 1 + W * C)) for H, W, C in shapes)
    for bad in ((2, R.MAX_ROW_BYTES, 1), (2, (R.MAX_ROW_BYTES - 1) // 3 + 1, 3)):
        assert table_bytes(records([shapes[0], bad])) == 0
