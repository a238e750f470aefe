"""The host side of the PNG encoder's match="lz" route without a GPU.  (1) The host / device pieces of
attwarp_amd/csrc/png_lz_blocks.hpp (distance symbols against RFC 1951's table for every distance, the extra-bit tables, the
hash, the token word, the tie rule) on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: tests/pnglz_host_main.cpp
is compiled as a stand-alone program and run as a child process; it must end clean.  (2) The planners through the C ABI with
fake pointers (nothing is launched): attwarp_png_plan == attwarp_png_plan_ex(NULL) == attwarp_png_plan_ex(all RLE) byte for
byte, what an LZ image adds to the table, and the refusals."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import png_ref as R
import pnglz_ref as Z
from test_png_host_cpu import records

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
E_INVALID = -1                                               # ATTWARP_E_INVALID of include/attwarp.h
SHAPES = [(500, 600, 1), (3, 5, 3), (1025, 1, 1), (400, 300, 3), (1, 1, 1)]


def test_host_pieces_under_sanitizers(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "pnglz_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "pnglz_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[:2] == ["pnglz_host", "ok"] and int(words[2]) > 32768 + (1 << 20)


def test_restated_distance_symbols_are_rfc_1951s():
    for s in range(30):
        top = Z.DIST_BASE[s + 1] - 1 if s < 29 else 32768
        assert Z.dist_symbol(Z.DIST_BASE[s]) == (s, Z.DIST_EXTRA[s], 0)
        assert Z.dist_symbol(top) == (s, Z.DIST_EXTRA[s], (1 << Z.DIST_EXTRA[s]) - 1)
    assert Z.HEADER_BITS == 1338


def plan_ex(rec, match):
    """-> (header fields, table bytes) of attwarp_png_plan_ex; match: None (NULL) or one int per image."""
    from attwarp_amd import _lib
    lib = _lib.load()
    m = None if match is None else np.asarray(match, np.int32)
    mp = None if m is None else ctypes.c_void_p(m.ctypes.data)
    rp = ctypes.c_void_p(rec.ctypes.data)
    n = lib.attwarp_png_table_bytes_ex(rp, len(rec), mp)
    assert n > 0, lib.attwarp_last_error()
    table = np.full(n, 0xEE, np.uint8)
    _lib.call("attwarp_png_plan_ex", rp, len(rec), mp, table.ctypes.data, n)
    h = _lib.PngHeader.from_address(table.ctypes.data)
    return (h.B, h.nseg, h.reserved, h.table_bytes, h.scratch_bytes, h.out_bytes, h.off_segs), table


def test_plan_equals_plan_ex_without_lz():
    from attwarp_amd import _lib
    lib = _lib.load()
    rec = records(SHAPES)
    rp = ctypes.c_void_p(rec.ctypes.data)
    n = lib.attwarp_png_table_bytes(rp, len(rec))
    plain = np.full(n, 0x11, np.uint8)
    _lib.call("attwarp_png_plan", rp, len(rec), plain.ctypes.data, n)
    (_, nseg, nlz, nbytes, _, _, _), null = plan_ex(rec, None)
    _, zeros = plan_ex(rec, [0] * len(SHAPES))
    assert nlz == 0 and nbytes == n == null.size == zeros.size
    assert plain.tobytes() == null.tobytes() == zeros.tobytes()
    assert nseg == sum(len(R.segments(H, 1 + W * C)) for H, W, C in SHAPES)


def test_lz_images_add_the_order_list_and_nothing_else():
    rec = records(SHAPES)
    match = [1, 0, 1, 0, 1]
    (B, nseg, nlz0, n0, scratch0, out0, off_segs), base = plan_ex(rec, None)
    (_, nseg1, nlz, n1, scratch1, out1, off1), table = plan_ex(rec, match)
    per = [len(R.segments(H, 1 + W * C)) for H, W, C in SHAPES]
    assert (nseg1, scratch1, out1, off1) == (nseg, scratch0, out0, off_segs)        # bound and scratch slots do not change
    assert nlz == sum(p for p, m in zip(per, match) if m) and n1 == n0 + -(-nseg * 4 // 8) * 8
    order = table[off_segs + nseg * 32:off_segs + nseg * 32 + nseg * 4].view(np.int32).tolist()
    image_of = [b for b, p in enumerate(per) for _ in range(p)]
    rle = [s for s in range(nseg) if not match[image_of[s]]]
    lz = [s for s in range(nseg) if match[image_of[s]]]
    assert order == rle + lz                                                        # RLE segments first, each part in segment order
    same = table[:n0].copy()
    same[12:16] = base[12:16]                                                        # header.reserved (the LZ segment count) ...
    same[16:24] = base[16:24]                                                       # ... and table_bytes
    off_images = 16 * -(-ctypes.sizeof(__import__("attwarp_amd")._lib.PngHeader) // 16)
    for b, m in enumerate(match):                                                   # ... and the images' match byte
        assert table[off_images + 80 * b + 73] == m
        same[off_images + 80 * b + 73] = 0
    assert same.tobytes() == base.tobytes()


def test_refusals():
    from attwarp_amd import _lib
    lib = _lib.load()
    rec = records(SHAPES[:2])
    rp = ctypes.c_void_p(rec.ctypes.data)
    for bad in ([0, 2], [-1, 0], [1, 7]):
        m = np.asarray(bad, np.int32)
        mp = ctypes.c_void_p(m.ctypes.data)
        assert lib.attwarp_png_table_bytes_ex(rp, 2, mp) == 0 and b"match" in lib.attwarp_last_error()
        buf = np.zeros(4096, np.uint8)
        assert lib.attwarp_png_plan_ex(rp, 2, mp, buf.ctypes.data, 4096) == E_INVALID and not buf.any()
    m = np.asarray([1, 1], np.int32)
    mp = ctypes.c_void_p(m.ctypes.data)
    n = lib.attwarp_png_table_bytes_ex(rp, 2, mp)
    with pytest.raises(_lib.AttWarpError):                                          # a table that is too small for the order list
        _lib.call("attwarp_png_plan_ex", rp, 2, mp, np.zeros(n, np.uint8).ctypes.data, n - 1)
    assert lib.attwarp_png_table_bytes_ex(rp, 0, mp) == 0


def test_header_and_library_agree():
    """The new entry points are declared in include/attwarp.h, line for line as the library defines them, and exported with
    the argument lists of attwarp_amd/_lib.py."""
    from attwarp_amd import _lib
    lib = _lib.load()
    lines = [" ".join(l.split()) for l in open(os.path.join(os.path.dirname(HERE), "include", "attwarp.h")).read().splitlines()]
    want = {"attwarp_png_table_bytes_ex": "ATTWARP_API size_t attwarp_png_table_bytes_ex(const attwarp_png_image* images, int B, const int32_t* match);",
            "attwarp_png_plan_ex": "ATTWARP_API int attwarp_png_plan_ex(const attwarp_png_image* images, int B, const int32_t* match, void* table, "
                                   "size_t table_bytes);"}
    source = " ".join(open(os.path.join(CSRC, "png.hip")).read().split())
    for name, decl in want.items():
        assert lines.count(decl) == 1, name
        assert 'extern "C" ' + decl[len("ATTWARP_API "):-1] + " {" in source, name              # the definition has the same list
        assert getattr(lib, name)
    assert len(_lib.SIGNATURES["attwarp_png_table_bytes_ex"][1]) == 3 and len(_lib.SIGNATURES["attwarp_png_plan_ex"][1]) == 5
    assert lines.count("enum { ATTWARP_PNG_MATCH_RLE = 0, ATTWARP_PNG_MATCH_LZ = 1 };") == 1
