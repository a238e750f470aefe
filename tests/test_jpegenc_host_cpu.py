"""The JPEG encoder's host side without a GPU.  (1) The host / device pieces of attwarp_amd/csrc/jpegenc_blocks.hpp (colour,
quantiser, islow DCT, the block fetch with the edge rule and the dummy blocks, the Huffman tables) on the CPU under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/jpegenc_host_main.cpp is compiled as a stand-alone program and run as
a child process; it must end clean, and the tables it prints must be those of a Pillow file.  (2) The planner's refusals
(attwarp_jpegenc_bound / _table_bytes / _plan, called with fake pointers: nothing is launched) and the largest shapes below."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpegenc_cases as K
import jpegenc_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def recorded_blocks():
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:8, 0:8]
    blocks = [np.zeros((8, 8)), np.full((8, 8), 255), ((x + y) & 1) * 255, (1 - ((x + y) & 1)) * 255, (x & 1) * 255, (y & 1) * 255,
              (x >= 4) * 255, x * 36, rng.integers(0, 256, (8, 8)), rng.integers(0, 2, (8, 8)) * 255]
    return np.stack(blocks).astype(np.int64) - 128


def recorded_images():
    """(image with its pitch padding, H, W, C, layout, swap, quality): every layout on sizes with dummy blocks."""
    out = []
    for n, ((h, w), layout) in enumerate([((17, 9), "4:2:0"), ((24, 40), "4:2:0"), ((40, 25), "4:2:0"), ((9, 40), "4:2:2"), ((7, 70), "4:2:2"),
                                         ((33, 47), "4:4:4"), ((17, 9), "grey"), ((1, 1), "4:2:0"), ((16, 16), "4:2:0"), ((1, 17), "grey")]):
        c = 1 if layout == "grey" else 3
        out.append((K.noise(h, w, c, 50 + n), layout, n % 2 == 1 and c == 3, (1, 30, 75, 95, 100)[n % 5], (0, 5)[n % 2]))
    return out


def write_input(path):
    words = []
    blocks = recorded_blocks()
    want = R.fdct(blocks)
    words.append(len(blocks))
    for b, w in zip(blocks, want):
        words += b.reshape(-1).tolist() + w.reshape(-1).tolist()
    images = recorded_images()
    words.append(len(images))
    for img, layout, swap, quality, extra in images:
        a = img[:, :, None] if img.ndim == 2 else img
        H, W, C = a.shape
        hmax, vmax = R.SUBSAMPLINGS[layout] if C == 3 else (1, 1)
        pitch = W * C + extra
        rows = np.full((H, pitch), 0xAB, np.int64)
        rows[:, :W * C] = a.reshape(H, W * C)
        info = {}
        R.encode(img, quality, layout if C == 3 else "4:4:4", order="bgr" if swap else "rgb", info=info)
        words += [H, W, C, hmax, vmax, int(swap), pitch, quality, len(info["blocks"])] + rows.reshape(-1).tolist()
        words += np.stack(info["blocks"]).reshape(-1).tolist()
    np.asarray(words, np.int32).tofile(path)


def test_host_pieces_under_sanitizers(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe, data = tmp_path / "jpegenc_host", tmp_path / "input.bin"
    write_input(data)
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "jpegenc_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    words = lines[-1].split()
    assert words[:2] == ["jpegenc_host", "ok"] and int(words[2]) > 256 ** 3 + 255 * (1 << 17)
    # the Huffman tables: the DHT payloads are those of a Pillow file, the codes those of Annex C
    f = io.BytesIO()
    Image.fromarray(K.photo(16, 16, 3, 1)).save(f, "JPEG")
    pil = f.getvalue()
    dht = [[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("dht ")]
    codes = [[int(v) for v in ln.split()[2:]] for ln in lines if ln.startswith("codes ")]
    assert len(dht) == 4 and len(codes) == 4
    for t, (payload, code) in enumerate(zip(dht, codes)):
        seg = b"\xff\xc4" + (2 + len(payload)).to_bytes(2, "big") + bytes(payload)
        assert seg in pil, t
        want = [0] * 256
        for sym, (c, ln) in R.CODES[t].items():
            want[sym] = ln << 16 | c
        assert code == want, t
    for ln in lines:
        if ln.startswith("quant "):
            w = ln.split()
            q = int(w[1])
            assert [int(v) for v in w[2:130]] == np.concatenate(R.quant_tables(q)).tolist()
            assert [int(w[131]), int(w[132])] == [R.block_bound_bits(q, 1), R.block_bound_bits(q, 3)]


# ---- the planner ----------------------------------------------------------------------------------------------------------------
def records(shapes, quality=75, subsampling=2, restart_rows=0, pitch=None):
    from attwarp_amd import _lib
    rec = np.zeros(len(shapes), dtype=np.dtype(_lib.JpegEncImage))
    s = np.asarray(shapes, np.int64).reshape(-1, 3)
    rec["src"] = 0x1000                                      # never dereferenced: nothing is launched
    rec["H"], rec["W"], rec["C"] = s[:, 0], s[:, 1], s[:, 2]
    rec["pitch"] = s[:, 1] * s[:, 2] if pitch is None else pitch
    rec["order"], rec["quality"], rec["subsampling"], rec["restart_rows"] = _lib.RGB, quality, subsampling, restart_rows
    return rec


def table_bytes(rec):
    from attwarp_amd import _lib
    return _lib.load().attwarp_jpegenc_table_bytes(ctypes.c_void_p(rec.ctypes.data), len(rec))


def plan(rec):
    from attwarp_amd import _lib
    n = table_bytes(rec)
    assert n > 0
    table = np.zeros(n, np.uint8)
    _lib.call("attwarp_jpegenc_plan", ctypes.c_void_p(rec.ctypes.data), len(rec), table.ctypes.data, n)
    h = _lib.JpegEncHeader.from_address(table.ctypes.data)
    return (h.B, h.nunits, h.out_bytes, h.table_bytes), table


def units(H, W, C, sub, restart_rows):
    hmax, vmax, mx, my = R.geometry(H, W, C, sub)
    step = restart_rows * mx or mx * my
    return sum(-(-min(step, mx * my - m0) // R.UNIT_MCUS) for m0 in range(0, mx * my, step))


def test_bound_equals_the_restatement_and_plans_add_up():
    from attwarp_amd import _lib
    lib = _lib.load()
    shapes = [(1, 1, 1), (33, 47, 3), (40, 25, 3), (500, 500, 3), (17, 9, 1)]
    total = nunits = 0
    for i, (H, W, C) in enumerate(shapes):
        for q in (1, 75, 100):
            for sub, sid in R.SUBSAMPLING_IDS.items():
                for rr in (0, 1, 3):
                    assert lib.attwarp_jpegenc_bound(H, W, C, q, sid, rr) == R.bound(H, W, C, q, sub, rr)
    rec = records(shapes, quality=[1, 30, 75, 95, 100], subsampling=[0, 1, 2, 0, 1], restart_rows=[0, 1, 2, 0, 1])
    subs = ["4:4:4", "4:2:2", "4:2:0", "4:4:4", "4:2:2"]
    for (H, W, C), q, sub, rr in zip(shapes, [1, 30, 75, 95, 100], subs, [0, 1, 2, 0, 1]):
        total += R.bound(H, W, C, q, sub, rr)
        nunits += units(H, W, C, sub, rr)
    (B, n, out_bytes, nbytes), _ = plan(rec)
    assert (B, n, out_bytes) == (5, nunits, total)


def test_refusals():
    from attwarp_amd import _lib
    lib = _lib.load()

    def refused(rec, word):
        assert table_bytes(rec) == 0 and word in lib.attwarp_last_error(), lib.attwarp_last_error()
        with pytest.raises(_lib.AttWarpError):
            _lib.call("attwarp_jpegenc_plan", ctypes.c_void_p(rec.ctypes.data), len(rec), np.zeros(64, np.uint8).ctypes.data, 64)
    refused(records([(8, 8, 3)], quality=0), b"quality")
    refused(records([(8, 8, 3)], quality=101), b"quality")
    refused(records([(8, 8, 3)], subsampling=3), b"subsampling")
    refused(records([(8, 8, 2)]), b"channels")
    refused(records([(0, 8, 3)]), b"size")
    refused(records([(8, 65501, 1)]), b"65500")
    refused(records([(65501, 8, 1)]), b"65500")
    refused(records([(8, 8, 3)], pitch=23), b"pitch")
    refused(records([(8, 8, 3), (8, 8, 3)], pitch=[24, 23]), b"pitch")
    refused(records([(8, 8, 3)], restart_rows=-1), b"restart_rows")
    # the restart interval: 65500 grey pixels are 8188 MCUs per row; 8 rows are 65504 MCUs, 9 rows 73692
    assert plan(records([(1, 65500, 1)], restart_rows=8))[0][1] == -(-8188 // 16)
    refused(records([(1, 65500, 1)], restart_rows=9), b"restart interval")
    assert plan(records([(8, 65500, 3)], restart_rows=16))[0][0] == 1     # 4094 MCUs per row x 16 = 65504
    refused(records([(8, 65500, 3)], restart_rows=17), b"restart interval")
    assert table_bytes(records([(1, 1, 1)])[:0]) == 0                                              # B = 0


def test_two_gib_bound_and_the_largest_shapes_below_it():
    from attwarp_amd import _lib
    lib = _lib.load()
    for C, q, sub in ((1, 75, "4:2:0"), (3, 75, "4:2:0"), (3, 100, "4:4:4")):
        W = R.MAX_DIM
        H, hi = 1, R.MAX_DIM + 1                              # bisect: bound(H) < 2^31 <= bound(hi), or all heights fit
        if R.bound(R.MAX_DIM, W, C, q, sub) < 1 << 31:
            H = R.MAX_DIM
        else:
            while hi - H > 1:
                mid = (H + hi) // 2
                H, hi = (mid, hi) if R.bound(mid, W, C, q, sub) < 1 << 31 else (H, mid)
            assert lib.attwarp_jpegenc_bound(hi, W, C, q, R.SUBSAMPLING_IDS[sub], 0) == 0
            assert table_bytes(records([(hi, W, C)], quality=q, subsampling=R.SUBSAMPLING_IDS[sub])) == 0 and b"2 GiB" in lib.attwarp_last_error()
        assert lib.attwarp_jpegenc_bound(H, W, C, q, R.SUBSAMPLING_IDS[sub], 0) == R.bound(H, W, C, q, sub)
        (B, n, out_bytes, nbytes), _ = plan(records([(H, W, C)], quality=q, subsampling=R.SUBSAMPLING_IDS[sub]))
        assert (B, n, out_bytes) == (1, units(H, W, C, sub, 0), R.bound(H, W, C, q, sub))


def test_batch_size_limit():
    from attwarp_amd import _lib
    lib = _lib.load()
    B = 1 << 20
    assert table_bytes(records([(1, 1, 1)] * (B + 1))) == 0 and b"2^20" in lib.attwarp_last_error()
    assert table_bytes(records([(1, 1, 1)] * B)) > 0         # (planning them would take a table of 1.5 GiB: the count alone)
    (b, n, out_bytes, nbytes), _ = plan(records([(1, 1, 1)] * 4096))
    assert (b, n, out_bytes) == (4096, 4096, 4096 * R.bound(1, 1, 1))


def test_unit_count_limit():
    """More than 2^24 units in one call are refused by attwarp_jpegenc_table_bytes, which only counts: a 20000 x 20000 grey
    image at quality 1 stays below 2 GiB and has 2500 x 2500 MCUs, 390625 units; 42 of them fit, 43 do not."""
    from attwarp_amd import _lib
    lib = _lib.load()
    assert units(20000, 20000, 1, "4:4:4", 0) == 390625 and R.bound(20000, 20000, 1, 1) < 1 << 31
    assert 42 * 390625 <= 1 << 24 < 43 * 390625
    assert table_bytes(records([(20000, 20000, 1)] * 42, quality=1)) > 0
    assert table_bytes(records([(20000, 20000, 1)] * 43, quality=1)) == 0 and b"units" in lib.attwarp_last_error()
