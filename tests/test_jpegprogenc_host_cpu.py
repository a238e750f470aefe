"""The progressive encoder's host side without a GPU.  (1) The block coders, the run resolution, the walk and the byte writer of
attwarp_amd/csrc/jpegprogenc_blocks.hpp (the text the jpegprogenc_* kernels run) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/jpegprogenc_host_main.cpp is compiled as a stand-alone program and run as a child process
over recorded coefficient blocks of the corpus and over random blocks; it must end clean and print the restatement's tokens
and bytes, for the one walk over an interval and for the interval coded block by block (summary, run resolution, a block
on its own), interleaved DC passes included.  (2) The planner: attwarp_jpegenc_plan_prog with no progressive image gives the
table attwarp_jpegenc_plan_ex gives (which forwards to it: that the bytes are the parent's rests on the older tests), the
progressive table's records, attwarp_jpegenc_bound_prog, the refusals and the declarations (fake pointers: nothing is
launched)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpegenc_ref as R
import jpegopt_ref as O
import jpegprogenc_cases as C
import jpegprogenc_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GREY_SCANS = [sc[1:] for sc in P.SCRIPT_GREY] + [(1, 63, 0, 1)]            # and the chroma first pass


def block_sets():
    """[(name, [(count, 64 coefficients)])]: luma blocks of corpus cases, random blocks, long runs of empty blocks."""
    out = []
    for name in ("be_flush", "refine_runs", "c63", "worst_grey", "restart_1", "dummy_h40_grey", "q100"):
        z = C.info(name)["comps"][0].reshape(-1, 64)[:300]
        out.append((name, [(1, b) for b in z]))
    rng = np.random.default_rng(5)
    for k, (density, hi) in enumerate(((0.05, 3), (0.3, 8), (1.0, 1023), (0.1, 40))):
        z = rng.integers(-hi, hi + 1, (120, 64)) * (rng.random((120, 64)) < density)
        out.append((f"random_{k}", [(1, b) for b in z]))
    e = np.zeros(64, np.int64)
    one = e.copy()
    one[3], one[40] = 5, -1
    out.append(("run_7fff", [(1, one), (0x7fff + 10, e), (1, one), (5, e)]))
    return out


def restated(blocks, slot, sc):
    """(tokens flattened as the program prints them, the stuffed bytes) of one interval over the blocks, from the restatement."""
    z = np.concatenate([np.repeat(np.asarray(b, np.int64)[None], n, 0) for n, b in blocks])
    tokens, _ = P.scan_tokens([z[None]], (1, 1, len(z), 1), (8, 8 * len(z)), ((0,),) + tuple(sc), slot, 0)
    flat, hist = [], np.zeros(256, np.int64)
    for t in tokens:
        if t[0] == "s":
            flat += [0, t[1], t[2]]
            hist[t[2]] += 1
        elif t[0] == "b":
            flat += [1, t[1], t[2]]
    codes = R.huffman_codes(*O.optimal_table(hist))
    bits = "".join(format(codes[t[2]][0], f"0{codes[t[2]][1]}b") if t[0] == "s" else format(t[1], f"0{t[2]}b") for t in tokens if t[0] != "r")
    bits += "1" * (-len(bits) % 8)
    data = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    return flat, data.replace(b"\xff", b"\xff\x00")


def walks():
    """(bpm, ny, hmax, vmax, mcus_x, comp, wc, n) and the restatement's answer: component and block index per step."""
    out = []
    for hmax, vmax, mx, my in ((2, 2, 3, 2), (2, 1, 4, 3), (1, 1, 5, 2)):
        ny, bpm = hmax * vmax, hmax * vmax + 2
        index = {}                                            # (component, row, column) -> block index in MCU order
        for m in range(mx * my):
            r, c = divmod(m, mx)
            for s in range(ny):
                index[0, r * vmax + s // hmax, c * hmax + s % hmax] = m * bpm + s
            index[1, r, c], index[2, r, c] = m * bpm + ny, m * bpm + ny + 1
        out.append(((bpm, ny, hmax, vmax, mx, -1, 0, mx * my * bpm), [(0 if j % bpm < ny else j % bpm - ny + 1, j) for j in range(mx * my * bpm)]))
        for comp, wc, hc in ((0, mx * hmax - 1, my * vmax - (vmax - 1)), (1, mx, my), (2, mx, my)):
            out.append(((bpm, ny, hmax, vmax, mx, comp, wc, wc * hc), [(comp, index[comp, j // wc, j % wc]) for j in range(wc * hc)]))
    return out


def test_coders_under_sanitizers(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "jpegprogenc_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "jpegprogenc_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    records, want = [], []
    for name, blocks in block_sets():
        for slot, sc in enumerate(GREY_SCANS):
            if name == "run_7fff" and sc[0] == 0:
                continue
            records.append(f"scan {slot} {sc[0]} {sc[1]} {sc[2]} {sc[3]} {len(blocks)}\n" +
                           "\n".join(f"{n} " + " ".join(str(int(v)) for v in b) for n, b in blocks))
            want.append((name, slot) + restated(blocks, slot, sc))
    dcs = []                                                  # interleaved DC first passes: whole MCUs of three components
    for name, ny in (("restart_1", 4), ("dummy_both_422", 2), ("q100", 1)):
        comps = C.info(name)["comps"]
        hm, vm = (2, 2) if ny == 4 else ((2, 1) if ny == 2 else (1, 1))
        blocks, order = [], []
        for r in range(comps[1].shape[0]):
            for c in range(comps[1].shape[1]):
                blocks += [comps[0][r * vm + by, c * hm + bx] for by in range(vm) for bx in range(hm)] + [comps[1][r, c], comps[2][r, c]]
                order += [0] * ny + [1, 2]
        records.append(f"dc {ny + 2} {ny} {len(blocks)}\n" + "\n".join("1 " + " ".join(str(int(v)) for v in b) for b in blocks))
        tokens = []
        P._dc_first([(ci, P.DC1_SLOT if ci else 0, b[0]) for ci, b in zip(order, blocks)], 1, tokens, None)
        dcs.append((name, [v for t in tokens for v in ((0, t[1], t[2]) if t[0] == "s" else (1, t[1], t[2]))]))
    ws = walks()
    for args, _ in ws:
        records.append("walk " + " ".join(str(v) for v in args))
    text = f"{len(records)}\n" + "\n".join(records) + "\n"
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"jpegprogenc_host ok {len(records)}" and len(lines) == 2 * len(want) + len(dcs) + len(ws) + 1
    forced = 0
    for i, (name, slot, tokens, data) in enumerate(want):
        got_t, got_b = lines[2 * i].split(), lines[2 * i + 1].split()
        assert got_t[0] == "tokens" and [int(v) for v in got_t[1:]] == tokens, (name, slot)
        assert got_b[0] == "bytes" and int(got_b[1]) == len(data) and bytes(int(v) for v in got_b[2:]) == data, (name, slot)
        forced += name in ("be_flush", "run_7fff") and slot in (3, 5)
    assert forced >= 3
    for (name, tokens), line in zip(dcs, lines[2 * len(want):]):
        assert [int(v) for v in line.split()[1:]] == tokens and {10, 0} <= set(tokens[1::3]), name
    for (args, answer), line in zip(ws, lines[2 * len(want) + len(dcs):]):
        v = [int(x) for x in line.split()[1:]]
        assert list(zip(v[0::2], v[1::2])) == answer, args


# ---- the planner ------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (33, 47, 3), (40, 56, 3), (500, 500, 3), (17, 9, 1)]
KW = dict(quality=[1, 30, 75, 95, 100], subsampling=[0, 1, 2, 0, 1], restart_rows=[0, 1, 1, 0, 2])
SUBS = ["4:4:4", "4:2:2", "4:2:0", "4:4:4", "4:2:2"]


def records_of(shapes, quality=75, subsampling=2, restart_rows=0):
    from attwarp_amd import _lib
    rec = np.zeros(len(shapes), dtype=np.dtype(_lib.JpegEncImage))
    s = np.asarray(shapes, np.int64).reshape(-1, 3)
    rec["src"] = 0x1000                                      # never dereferenced: nothing is launched
    rec["H"], rec["W"], rec["C"] = s[:, 0], s[:, 1], s[:, 2]
    rec["pitch"] = s[:, 1] * s[:, 2]
    rec["order"], rec["quality"], rec["subsampling"], rec["restart_rows"] = _lib.RGB, quality, subsampling, restart_rows
    return rec


def _ptr(flags):
    if flags is None:
        return None, None
    a = np.asarray(flags, np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


def plan_prog(rec, optimize, progressive):
    from attwarp_amd import _lib
    lib = _lib.load()
    (_o, op), (_p, pp) = _ptr(optimize), _ptr(progressive)
    n = lib.attwarp_jpegenc_table_bytes_prog(ctypes.c_void_p(rec.ctypes.data), len(rec), op, pp)
    assert n > 0, lib.attwarp_last_error()
    table = np.full(n, 0xEE, np.uint8)
    _lib.call("attwarp_jpegenc_plan_prog", ctypes.c_void_p(rec.ctypes.data), len(rec), op, pp, table.ctypes.data, n)
    return table, _lib.JpegEncHeader.from_buffer_copy(table[:ctypes.sizeof(_lib.JpegEncHeader)].tobytes())


def test_plan_prog_without_a_progressive_image_is_plan_ex_byte_for_byte():
    from attwarp_amd import _lib
    lib = _lib.load()
    rec = records_of(SHAPES, **KW)
    for optimize in (None, [1, 0, 1, 1, 0]):
        _o, op = _ptr(optimize)
        n = lib.attwarp_jpegenc_table_bytes_ex(ctypes.c_void_p(rec.ctypes.data), len(rec), op)
        want = np.full(n, 0xEE, np.uint8)
        _lib.call("attwarp_jpegenc_plan_ex", ctypes.c_void_p(rec.ctypes.data), len(rec), op, want.ctypes.data, n)
        for progressive in (None, [0] * len(SHAPES)):
            table, h = plan_prog(rec, optimize, progressive)
            assert table.tobytes() == want.tobytes() and h.reserved == 0


def test_progressive_plan_records_and_bound_prog():
    from attwarp_amd import _lib
    lib = _lib.load()
    rec = records_of(SHAPES, **KW)
    opt, prog = [1, 0, 1, 1, 0], [1, 0, 1, 0, 1]
    plain, hp = plan_prog(rec, opt, None)
    table, h = plan_prog(rec, opt, prog)
    total = 0
    for (H, W, Cn), q, sub, sid, rr, o, p in zip(SHAPES, KW["quality"], SUBS, KW["subsampling"], KW["restart_rows"], opt, prog):
        want = P.bound(H, W, Cn, q, sub, rr) if p else O.bound(H, W, Cn, q, sub, rr, optimize=bool(o))
        assert lib.attwarp_jpegenc_bound_prog(H, W, Cn, q, sid, rr, o, p) == want
        assert lib.attwarp_jpegenc_bound_prog(H, W, Cn, q, sid, rr, o, 0) == lib.attwarp_jpegenc_bound_ex(H, W, Cn, q, sid, rr, o)
        total += want
    assert h.out_bytes == total and h.B == 5
    # a progressive image owns no entropy unit: the header counts the others' only, its transform units follow them
    units = lambda H, W, Cn, sub, rr: len(R.unit_plan(np.zeros((H, W, Cn), np.uint8)[:, :, 0] if Cn == 1 else np.zeros((H, W, 3), np.uint8), 75, sub, rr)["units"])
    per_image = [units(H, W, Cn, sub, rr) for (H, W, Cn), sub, rr in zip(SHAPES, SUBS, KW["restart_rows"])]
    assert hp.nunits == sum(per_image) and h.nunits == sum(n for n, p in zip(per_image, prog) if not p)
    at = h.reserved * 16
    assert at >= h.off_units + 32 * hp.nunits and at % 16 == 0
    words = table[at:at + 56].view(np.int32)
    nimages, nsegs, ntunits = (int(v) for v in words[:3])
    off_images, off_segs, off_hist, off_tables, off_seg_out = (int(v) for v in table[at + 16:at + 56].view(np.uint64))
    assert nimages == 3 and ntunits == sum(n for n, p in zip(per_image, prog) if p)
    assert off_images == at + 64 and off_segs == off_images + 184 * nimages and len(table) == h.table_bytes == off_segs + 40 * nsegs
    assert off_tables == off_hist + nimages * 11 * 1024 and off_seg_out == off_tables + nimages * 11 * 1320 and h.scratch_bytes == off_seg_out + 16 * nsegs
    tunit_image = table[h.off_units + 32 * h.nunits:h.off_units + 32 * (h.nunits + ntunits)].view(np.int32).reshape(-1, 8)[:, 0]
    assert sorted(set(tunit_image.tolist())) == [0, 2, 4]
    images = table[off_images:off_images + 184 * nimages].view(np.int32).reshape(nimages, 46)
    segs = table[off_segs:off_segs + 40 * nsegs].view(np.int32).reshape(nsegs, 10)
    seg0 = 0
    for k, b in enumerate((0, 2, 4)):
        H, W, Cn = SHAPES[b]
        geo = P.scan_geometry(H, W, Cn, SUBS[b], KW["restart_rows"][b])
        image, nscans, s0, ns, header_len = images[k, :5].tolist()
        assert (image, nscans, s0, ns) == (b, len(geo), seg0, sum(g[2] for g in geo))
        assert header_len == len(P.frame_header(H, W, Cn, KW["quality"][b], SUBS[b]))
        info = {}
        P.encode(np.zeros((H, W, Cn), np.uint8)[:, :, 0] if Cn == 1 else np.zeros((H, W, 3), np.uint8), KW["quality"][b], SUBS[b], KW["restart_rows"][b], info=info)
        dri = [v for v in images[k, 6:6 + 4 * nscans].reshape(nscans, 4)[:, 3].tolist() if v]
        assert dri == info["dri"]
        mine = segs[s0:s0 + ns]
        assert (mine[:, 0] == k).all()
        for i, (nblk, step, nint, bpb, _, _) in enumerate(geo):
            rows = mine[mine[:, 1] == i]
            assert len(rows) == nint and rows[:, 2].tolist() == [j * step for j in range(nint)] and int(rows[:, 3].sum()) == nblk
            assert rows[:, 4].tolist() == list(range(nint))
            assert rows[:, 5].tolist() == [(int(n) * bpb + P.EOBRUN_BITS + 7) // 8 for n in rows[:, 3]]
            slot = rows[:, 6:8].copy().view(np.uint64)[:, 0].astype(np.int64)
            aux = rows[:, 8:10].copy().view(np.uint64)[:, 0].astype(np.int64)
            assert (slot % 16 == 0).all() and (aux - slot == (rows[:, 5] + 8 + 15) // 16 * 16).all()
        seg0 += ns
    if at:
        assert images[1, 6:46].reshape(10, 4)[:, 3].tolist() == [4, 7, 4, 0, 7, 0, 4, 0, 0, 7]


def test_refusals_and_declarations():
    from attwarp_amd import _lib
    lib = _lib.load()
    rec = records_of([(8, 8, 3), (8, 8, 1)])
    for flags in ([1, 2], [-1, 0]):
        f = np.asarray(flags, np.int32)
        assert lib.attwarp_jpegenc_table_bytes_prog(ctypes.c_void_p(rec.ctypes.data), 2, None, ctypes.c_void_p(f.ctypes.data)) == 0
        assert b"progressive" in lib.attwarp_last_error()
        with pytest.raises(_lib.AttWarpError):
            _lib.call("attwarp_jpegenc_plan_prog", ctypes.c_void_p(rec.ctypes.data), 2, None, ctypes.c_void_p(f.ctypes.data), np.zeros(64, np.uint8).ctypes.data, 64)
    one = np.ones(1, np.int32)
    # a luma scan walks twice the MCUs per row: 4:2:0, 4094 MCUs per row and 9 rows per interval pass plain (36846) and are refused
    # progressive (73692 luma blocks per interval; libjpeg would clamp the interval to 65535)
    wide = records_of([(256, 65500, 3)], restart_rows=9)
    assert lib.attwarp_jpegenc_table_bytes_ex(ctypes.c_void_p(wide.ctypes.data), 1, None) > 0
    assert lib.attwarp_jpegenc_table_bytes_prog(ctypes.c_void_p(wide.ctypes.data), 1, None, ctypes.c_void_p(one.ctypes.data)) == 0
    assert b"65535" in lib.attwarp_last_error() and b"clamps" in lib.attwarp_last_error()
    assert lib.attwarp_jpegenc_bound_prog(256, 65500, 3, 75, 2, 9, 0, 1) == 0 and lib.attwarp_jpegenc_bound_prog(256, 65500, 3, 75, 2, 9, 0, 0) > 0
    assert lib.attwarp_jpegenc_bound_prog(256, 65500, 3, 75, 2, 8, 0, 1) > 0          # (8188 x 8 = 65504 luma blocks: the largest that fits)
    assert lib.attwarp_jpegenc_bound_prog(8, 8, 3, 0, 2, 0, 0, 1) == 0 and lib.attwarp_jpegenc_bound_prog(8, 65501, 1, 75, 2, 0, 0, 1) == 0
    # the progressive bound moves the 2 GiB limit
    H, hi = 1, R.MAX_DIM + 1
    while hi - H > 1:
        mid = (H + hi) // 2
        H, hi = (mid, hi) if P.bound(mid, R.MAX_DIM, 1, 75) < 1 << 31 else (H, mid)
    assert lib.attwarp_jpegenc_bound_prog(H, R.MAX_DIM, 1, 75, 2, 0, 0, 1) > 0 and lib.attwarp_jpegenc_bound_prog(H + 1, R.MAX_DIM, 1, 75, 2, 0, 0, 1) == 0
    big = records_of([(H + 1, R.MAX_DIM, 1)])
    assert lib.attwarp_jpegenc_table_bytes_prog(ctypes.c_void_p(big.ctypes.data), 1, None, ctypes.c_void_p(one.ctypes.data)) == 0 and b"2 GiB" in lib.attwarp_last_error()
    # too small a table
    f = np.ones(2, np.int32)
    with pytest.raises(_lib.AttWarpError):
        _lib.call("attwarp_jpegenc_plan_prog", ctypes.c_void_p(rec.ctypes.data), 2, None, ctypes.c_void_p(f.ctypes.data), np.zeros(64, np.uint8).ctypes.data, 64)
    # header, definitions and binding move together
    hdr = open(os.path.join(ROOT, "include", "attwarp.h")).read()
    source = open(os.path.join(CSRC, "jpegenc.hip")).read()
    want = {"attwarp_jpegenc_bound_prog": "size_t attwarp_jpegenc_bound_prog(int H, int W, int C, int quality, int subsampling, int restart_rows, int optimize, int progressive)",
            "attwarp_jpegenc_table_bytes_prog": "size_t attwarp_jpegenc_table_bytes_prog(const attwarp_jpegenc_image* images, int B, const int32_t* optimize, const int32_t* progressive)",
            "attwarp_jpegenc_plan_prog": "int attwarp_jpegenc_plan_prog(const attwarp_jpegenc_image* images, int B, const int32_t* optimize, const int32_t* progressive,"}
    for name, decl in want.items():
        assert "ATTWARP_API " + decl in hdr, name
        assert 'extern "C" ' + decl in source, name
        assert name in _lib.SIGNATURES
    assert [len(_lib.SIGNATURES[n][1]) for n in want] == [8, 4, 6]
    assert ctypes.sizeof(_lib.JpegEncHeader) == 80
