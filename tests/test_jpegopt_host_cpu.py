"""The optimised Huffman tables' host side without a GPU.  (1) The table builder of attwarp_amd/csrc/jpegopt_blocks.hpp (the
text the table kernel runs) on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: tests/jpegopt_host_main.cpp is
compiled as a stand-alone program and run as a child process over the histograms of jpegopt_cases.table_histograms(); it must
end clean and print the tables of the restatement.  (2) The planner: attwarp_jpegenc_plan_ex with no optimised image is
attwarp_jpegenc_plan byte for byte, the optimised table's records, attwarp_jpegenc_bound_ex, and the refusals (fake
pointers: nothing is launched)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpegenc_ref as R
import jpegopt_cases as C
import jpegopt_ref as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_table_builder_under_sanitizers(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "jpegopt_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "jpegopt_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    hists = C.table_histograms()
    text = f"{len(hists)}\n" + "\n".join(" ".join(str(int(v)) for v in h) for _, h, _ in hists) + "\n"
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"jpegopt_host ok {len(hists)}" and len(lines) == 3 * len(hists) + 1
    for i, (name, hist, libjpeg_answers) in enumerate(hists):
        head, dht, codes = (ln.split() for ln in lines[3 * i:3 * i + 3])
        info = {}
        bits, vals = O.optimal_table(hist, info=info)
        assert head == ["table", str(i), str(info["depth"]), str(len(vals))], name
        got_bits, got_vals = [int(v) for v in dht[6:22]], [int(v) for v in dht[22:]]
        # validity, which is all that can be asked where libjpeg has no answer: a complete code of at most 16 bits
        assert sum(got_bits) == len(got_vals) and sorted(got_vals) == np.flatnonzero(hist).tolist() and O.kraft_gap(got_bits) == 1, name
        # the restatement's table (libjpeg's wherever libjpeg succeeds; the same procedure over longer counts where it does not)
        assert bytes(int(v) for v in dht[1:]) == O.dht_segment((i & 1) << 4 | (i >> 1 & 1), bits, vals), (name, libjpeg_answers)
        assert [int(v) for v in codes[1:]] == O.code_words(bits, vals), name


# ---- the planner ------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (33, 47, 3), (40, 25, 3), (500, 500, 3), (17, 9, 1)]
KW = dict(quality=[1, 30, 75, 95, 100], subsampling=[0, 1, 2, 0, 1], restart_rows=[0, 1, 2, 0, 1])


def records(shapes, quality=75, subsampling=2, restart_rows=0):
    from attwarp_amd import _lib
    rec = np.zeros(len(shapes), dtype=np.dtype(_lib.JpegEncImage))
    s = np.asarray(shapes, np.int64).reshape(-1, 3)
    rec["src"] = 0x1000                                      # never dereferenced: nothing is launched
    rec["H"], rec["W"], rec["C"] = s[:, 0], s[:, 1], s[:, 2]
    rec["pitch"] = s[:, 1] * s[:, 2]
    rec["order"], rec["quality"], rec["subsampling"], rec["restart_rows"] = _lib.RGB, quality, subsampling, restart_rows
    return rec


def plan_ex(rec, optimize):
    from attwarp_amd import _lib
    lib = _lib.load()
    flags = None if optimize is None else np.asarray(optimize, np.int32)
    fp = None if flags is None else ctypes.c_void_p(flags.ctypes.data)
    n = lib.attwarp_jpegenc_table_bytes_ex(ctypes.c_void_p(rec.ctypes.data), len(rec), fp)
    assert n > 0, lib.attwarp_last_error()
    table = np.full(n, 0xEE, np.uint8)
    _lib.call("attwarp_jpegenc_plan_ex", ctypes.c_void_p(rec.ctypes.data), len(rec), fp, table.ctypes.data, n)
    return table, _lib.JpegEncHeader.from_buffer_copy(table[:ctypes.sizeof(_lib.JpegEncHeader)].tobytes())


def test_plan_ex_without_an_optimised_image_is_plan_byte_for_byte():
    from attwarp_amd import _lib
    lib = _lib.load()
    rec = records(SHAPES, **KW)
    n = lib.attwarp_jpegenc_table_bytes(ctypes.c_void_p(rec.ctypes.data), len(rec))
    plain = np.full(n, 0xEE, np.uint8)
    _lib.call("attwarp_jpegenc_plan", ctypes.c_void_p(rec.ctypes.data), len(rec), plain.ctypes.data, n)
    for optimize in (None, [0] * len(SHAPES)):
        table, h = plan_ex(rec, optimize)
        assert table.tobytes() == plain.tobytes() and h.off_optimize == 0 and h.reserved == 0


def test_optimised_plan_records_and_bound_ex():
    from attwarp_amd import _lib
    lib = _lib.load()
    rec = records(SHAPES, **KW)
    subs = ["4:4:4", "4:2:2", "4:2:0", "4:4:4", "4:2:2"]
    flags = [1, 0, 1, 1, 0]
    plain, hp = plan_ex(rec, None)
    table, h = plan_ex(rec, flags)
    total = 0
    for (H, W, Cn), q, sub, sid, rr, f in zip(SHAPES, KW["quality"], subs, KW["subsampling"], KW["restart_rows"], flags):
        want = O.bound(H, W, Cn, q, sub, rr, optimize=bool(f))
        assert lib.attwarp_jpegenc_bound_ex(H, W, Cn, q, sid, rr, f) == want
        assert lib.attwarp_jpegenc_bound_ex(H, W, Cn, q, sid, rr, 0) == lib.attwarp_jpegenc_bound(H, W, Cn, q, sid, rr) == R.bound(H, W, Cn, q, sub, rr)
        total += want
    assert (h.B, h.nunits, h.out_bytes) == (hp.B, hp.nunits, total) and h.out_bytes > hp.out_bytes
    # the record of the optimised images: JoPlan {nimages, nunits, off_hist, off_out}, JoImage {image, pre_len, suf_len, ntables} each,
    # then their units in order; it starts where the plain table ends
    assert h.off_optimize == hp.table_bytes and h.scratch_bytes > hp.scratch_bytes
    words = table[h.off_optimize:].view(np.int32)
    nimages, nunits = int(words[0]), int(words[1])
    off_hist, off_out = (int(v) for v in table[h.off_optimize + 8:h.off_optimize + 24].view(np.uint64))
    assert nimages == 3 and off_hist % 256 == 0 and off_out == off_hist + 3 * 4096 and h.scratch_bytes == off_out + 3 * 5928
    images = words[6:6 + 4 * nimages].reshape(nimages, 4)
    assert images[:, 0].tolist() == [0, 2, 3] and images[:, 3].tolist() == [2, 4, 4]
    for (b, pre, suf, _), rr in zip(images.tolist(), (0, 2, 0)):
        H, W, Cn = SHAPES[b]
        std = R.header(H, W, Cn, KW["quality"][b], subs[b], 7 if rr else 0)
        assert pre == std.index(b"\xff\xc4") and suf == len(std) - (pre + (432 if Cn == 3 else 216))
    unit_image = table[h.off_units:h.off_units + 32 * h.nunits].view(np.int32).reshape(-1, 8)[:, 0]
    assert words[6 + 4 * nimages:6 + 4 * nimages + nunits].tolist() == np.flatnonzero(np.isin(unit_image, [0, 2, 3])).tolist()
    assert len(table) == h.table_bytes == h.off_optimize + 24 + 16 * nimages + 4 * nunits


def test_refusals_and_declarations():
    from attwarp_amd import _lib
    lib = _lib.load()
    rec = records([(8, 8, 3), (8, 8, 1)])
    for flags, word in (([1, 2], b"optimize"), ([-1, 0], b"optimize")):
        f = np.asarray(flags, np.int32)
        assert lib.attwarp_jpegenc_table_bytes_ex(ctypes.c_void_p(rec.ctypes.data), 2, ctypes.c_void_p(f.ctypes.data)) == 0
        assert word in lib.attwarp_last_error()
        with pytest.raises(_lib.AttWarpError):
            _lib.call("attwarp_jpegenc_plan_ex", ctypes.c_void_p(rec.ctypes.data), 2, ctypes.c_void_p(f.ctypes.data), np.zeros(64, np.uint8).ctypes.data, 64)
    one = np.ones(1, np.int32)
    bad = records([(8, 8, 3)], quality=0)
    assert lib.attwarp_jpegenc_table_bytes_ex(ctypes.c_void_p(bad.ctypes.data), 1, ctypes.c_void_p(one.ctypes.data)) == 0 and b"quality" in lib.attwarp_last_error()
    assert lib.attwarp_jpegenc_bound_ex(8, 8, 3, 0, 2, 0, 1) == 0 and lib.attwarp_jpegenc_bound_ex(8, 65501, 1, 75, 2, 0, 1) == 0
    # the one more bit per block moves the 2 GiB limit: the tallest grey image of full width that fits plain does not fit optimised
    H, hi = 1, R.MAX_DIM + 1
    while hi - H > 1:
        mid = (H + hi) // 2
        H, hi = (mid, hi) if R.bound(mid, R.MAX_DIM, 1, 75) < 1 << 31 else (H, mid)
    assert lib.attwarp_jpegenc_bound(H, R.MAX_DIM, 1, 75, 2, 0) > 0 and lib.attwarp_jpegenc_bound_ex(H, R.MAX_DIM, 1, 75, 2, 0, 1) == 0
    big = records([(H, R.MAX_DIM, 1)])
    assert lib.attwarp_jpegenc_table_bytes_ex(ctypes.c_void_p(big.ctypes.data), 1, None) > 0
    assert lib.attwarp_jpegenc_table_bytes_ex(ctypes.c_void_p(big.ctypes.data), 1, ctypes.c_void_p(one.ctypes.data)) == 0 and b"2 GiB" in lib.attwarp_last_error()
    # too small a table
    f = np.ones(2, np.int32)
    with pytest.raises(_lib.AttWarpError):
        _lib.call("attwarp_jpegenc_plan_ex", ctypes.c_void_p(rec.ctypes.data), 2, ctypes.c_void_p(f.ctypes.data), np.zeros(64, np.uint8).ctypes.data, 64)
    # header, definitions and binding move together
    hdr = open(os.path.join(ROOT, "include", "attwarp.h")).read()
    source = open(os.path.join(CSRC, "jpegenc.hip")).read()
    want = {"attwarp_jpegenc_bound_ex": "ATTWARP_API size_t attwarp_jpegenc_bound_ex(int H, int W, int C, int quality, int subsampling, int restart_rows, int optimize);",
            "attwarp_jpegenc_table_bytes_ex": "ATTWARP_API size_t attwarp_jpegenc_table_bytes_ex(const attwarp_jpegenc_image* images, int B, const int32_t* optimize);",
            "attwarp_jpegenc_plan_ex": "ATTWARP_API int attwarp_jpegenc_plan_ex(const attwarp_jpegenc_image* images, int B, const int32_t* optimize, void* table, "
                                       "size_t table_bytes);"}
    for name, decl in want.items():
        assert decl in hdr, name
        assert 'extern "C" ' + decl[len("ATTWARP_API "):-1] + " {" in source, name
        assert name in _lib.SIGNATURES
    assert [len(_lib.SIGNATURES[n][1]) for n in want] == [7, 3, 5]
    assert re.search(r"uint64_t off_optimize;", hdr) and _lib.JpegEncHeader._fields_[-1][0] == "off_optimize" and ctypes.sizeof(_lib.JpegEncHeader) == 80
