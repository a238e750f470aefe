"""The PNG decoder's format blocks (attwarp_amd/csrc/pngfmt_blocks.hpp) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/pngfmt_host_main.cpp is compiled as a stand-alone program and run as a child process over
the whole corpus (tests/pngfmt_cases.py).  It must end clean and print, per file, the restatement's filtered size, pass
offsets and the CRC-32 of its pixels in every mode.  The host-only planner attwarp_pngdec_plan_formats is checked against the
restatement through ctypes, without a device."""
import ctypes
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import pngdec_cases as PC
import pngdec_ref as D
import pngfmt_cases as C
import pngfmt_ref as F

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
VARIANTS = (("RGB", "rgb"), ("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr"))


def record(data, filtered):
    p = F.parse(data)
    pal = p["palette"]
    return (struct.pack("<IIIIII", p["W"], p["H"], p["color_type"], p["depth"], p["interlace"], len(pal) // 3) + pal + bytes(768 - len(pal)) +
            struct.pack("<I", len(filtered)) + filtered)


def test_host_blocks_under_sanitizers_equal_the_restatement(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "pngfmt_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "pngfmt_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    files = [(k.name, k.file, zlib.decompress(F.parse(k.file)["stream"])) for k in C.good()]
    bad = [(n, f, zlib.decompress(F.parse(f)["stream"])) for n, f in C.malformed() if n.startswith("filter")]
    assert len(bad) == 4
    path = tmp_path / "corpus.bin"
    path.write_bytes(struct.pack("<I", len(files) + len(bad)) + b"".join(record(f, filt) for _, f, filt in files + bad))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(files) + len(bad)
    for (name, f, filt), line in zip(files, lines):
        p = F.parse(f)
        ch = F.CHANNELS[p["color_type"]]
        offs = F.pass_offsets(p["W"], p["H"], ch, p["depth"], p["interlace"])
        offs += [len(filt)] * (7 - len(offs))                               # (a non-interlaced image: slots 1 .. 6 are empty)
        st, samples = F.unfilter(filt, p["W"], p["H"], p["color_type"], p["depth"], p["interlace"])
        px = F.to8(samples, p["color_type"], p["depth"], p["palette"])
        crcs = [zlib.crc32(D.convert(px, m, o).tobytes()) for m, o in VARIANTS]
        assert [int(x) for x in line.split()] == [len(filt)] + offs + crcs, name
    for (name, _, _), line in zip(bad, lines[len(files):]):
        assert line.split()[-1] == "filter", name


# ---- the planner, without a device ----------------------------------------------------------------------------------------
def plan(files, mode="RGB", order="rgb", formats=True):
    """-> (table bytes, header) of attwarp_pngdec_plan_formats (formats=False: attwarp_pngdec_plan) for the files."""
    from attwarp_amd import _batch, _lib
    parsed = [F.parse(f) for f in files]
    B, nchunks = len(files), sum(len(p["chunks"]) for p in parsed)
    rec = np.zeros(B, dtype=np.dtype(_lib.PngDecImage))
    fmt = np.zeros(B, dtype=np.dtype(_lib.PngDecFormat))
    chunks = np.zeros(nchunks, dtype=np.dtype(_lib.PngDecChunk))
    at = c = 0
    for b, p in enumerate(parsed):
        rec[b] = (at, len(p["stream"]), p["H"], p["W"], p["color_type"], _lib.PNGDEC_MODE_IDS[mode], {"rgb": _lib.RGB, "bgr": _lib.BGR}[order], 0)
        fmt["depth"][b], fmt["interlace"][b], fmt["palette_entries"][b] = p["depth"], p["interlace"], len(p["palette"]) // 3
        fmt["palette"][b, :len(p["palette"])] = np.frombuffer(p["palette"], np.uint8)
        for payload, crc in p["chunks"]:
            chunks[c] = (at, len(payload), crc, b, 0)
            at += len(payload)
            c += 1
    rp, fp, cp = (ctypes.c_void_p(a.ctypes.data) for a in (rec, fmt, chunks))
    if formats:
        size, pl = ("attwarp_pngdec_table_bytes_formats", rp, fp, B, cp, nchunks), ("attwarp_pngdec_plan_formats", rp, fp, B, cp, nchunks, 1, _batch.TABLE)
    else:
        size, pl = ("attwarp_pngdec_table_bytes", rp, B, nchunks), ("attwarp_pngdec_plan", rp, B, cp, nchunks, 1, _batch.TABLE)
    table, header = _batch.planned_table(size, pl, _lib.PngDecHeader, ValueError, "test: ", wrap_plan=True)
    return table, header, parsed


IMAGE = np.dtype([("stream_off", "<u8"), ("filt_off", "<u8"), ("out_off", "<u8"), ("stream_len", "<u4"), ("filt_bytes", "<u4"), ("H", "<i4"),
                  ("W", "<i4"), ("ch", "<i4"), ("oc", "<i4"), ("swap", "<i4"), ("row_bytes", "<i4")])
FORMAT = np.dtype([("depth", "<i4"), ("ctype", "<i4"), ("interlace", "<i4"), ("pal_off", "<u4")])


@pytest.mark.parametrize("mode,order", VARIANTS)
def test_planner_equals_the_restatement(mode, order):
    files = [k.file for k in C.small_good()] + [f for _, f in PC.good()[:5]]
    table, h, parsed = plan(files, mode, order)
    B = len(files)
    assert h.formats == 1 and h.B == B and h.table_bytes == table.size
    im = table[h.off_images:h.off_images + B * IMAGE.itemsize].view(IMAGE)
    foff = -(-(h.off_chunks + h.nchunks * 24) // 16) * 16
    fm = table[foff:foff + B * FORMAT.itemsize].view(FORMAT)
    out = scr = 0
    rows = []
    for b, p in enumerate(parsed):
        ch = F.CHANNELS[p["color_type"]]
        oc = 1 if mode == "L" else 3 if mode == "RGB" else (1 if p["color_type"] in (0, 4) else 3)
        r = im[b]
        assert (r["H"], r["W"], r["ch"], r["oc"]) == (p["H"], p["W"], ch, oc)
        assert r["filt_bytes"] == F.filt_bytes(p["W"], p["H"], ch, p["depth"], p["interlace"])
        assert r["row_bytes"] == F.row_bytes(p["W"], ch, p["depth"])
        assert r["swap"] == int(order == "bgr" and oc == 3 and p["color_type"] in (2, 3, 6))
        assert r["out_off"] == out and (b == 0 or r["filt_off"] == scr) and r["filt_off"] % 16 == 0
        out += p["H"] * p["W"] * oc
        scr = int(r["filt_off"]) + -(-int(r["filt_bytes"]) // 16) * 16
        rows.append(int(r["row_bytes"]))
        assert (fm[b]["depth"], fm[b]["ctype"], fm[b]["interlace"]) == (p["depth"], p["color_type"], p["interlace"])
        if p["color_type"] == 3:
            po = int(fm[b]["pal_off"])
            assert po >= foff + B * 16 and po + 768 <= table.size
            assert table[po:po + 768].tobytes() == p["palette"] + bytes(768 - len(p["palette"]))
        else:
            assert fm[b]["pal_off"] == 0
    assert h.out_bytes == out and h.scratch_bytes == scr
    assert h.lds_bytes == 1024 + max(16, -(-(max(rows) - 1) // 16) * 16)


def test_plain_files_plan_the_parents_table_byte_for_byte():
    files = [f for _, f in PC.good()]
    a, ha, _ = plan(files, formats=True)
    b, hb, _ = plan(files, formats=False)
    assert ha.formats == 0 and a.tobytes() == b.tobytes()
    c, hc, _ = plan(files + [C.pillow_written()[0].file])
    assert hc.formats == 1 and c.size > a.size


def test_row_limit_files_plan_and_the_planner_refuses_what_the_walk_refuses():
    from attwarp_amd import _lib
    _, h, _ = plan([k.file for k in C.row_limits()])
    assert h.lds_bytes == 1024 + D.MAX_ROW_BYTES                       # the palette, then a carry of 49151 bytes in 16s
    lib = _lib.load()
    rec = np.zeros(1, dtype=np.dtype(_lib.PngDecImage))
    fmt = np.zeros(1, dtype=np.dtype(_lib.PngDecFormat))
    table = np.zeros(1 << 16, np.uint8)

    def rc(W, H, ctype, depth, lace=0, entries=0):
        rec[0] = (0, 16, H, W, ctype, 0, _lib.RGB, 0)
        fmt["depth"], fmt["interlace"], fmt["palette_entries"] = depth, lace, entries
        code = lib.attwarp_pngdec_plan_formats(rec.ctypes.data, fmt.ctypes.data, 1, None, 0, 1, table.ctypes.data, table.size)
        return code, lib.attwarp_last_error().decode()

    assert rc(5, 5, 0, 1)[0] == 0 and rc(5, 5, 3, 4, 1, 16)[0] == 0
    for args, word in (((5, 5, 2, 4), "bit depth"), ((5, 5, 3, 16, 0, 4), "bit depth"), ((5, 5, 5, 8), "bit depth"), ((5, 5, 2, 8, 2), "interlace"),
                       ((5, 5, 3, 8, 0, 0), "PLTE"), ((5, 5, 3, 8, 0, 257), "PLTE"), ((393209, 2, 0, 1), "row of 49153"),
                       ((6144, 2, 6, 16), "row of 49153"), ((6000, 44740, 6, 16, 1), "2 GiB")):
        code, msg = rc(*args)
        assert code != 0 and word in msg, (args, code, msg)
