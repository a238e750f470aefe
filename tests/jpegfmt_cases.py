"""Files of the JPEG layouts the baseline records refuse (tests of attwarp_amd.jpeg with ``all_layouts=True``: test_jpegfmt_
ref_cpu.py, test_jpegfmt_host_cpu.py, test_jpegfmt_gpu.py), built at run time three ways: Pillow's writer (CMYK, RGB-coded),
header edits of Pillow's files (4:4:0, 4:1:1, 1x4, YCCK, RGB-coded with sub-sampled G and B), and a small coefficient-domain
writer for the layouts no edit reaches (4:1:0, a factor of 3, luma coarser than chroma, a sub-sampled K ...).  Pillow opens
every file of good(); malformed() files carry the restatement's status; refused() files are turned away by the marker walk
even with the keyword."""
from __future__ import annotations

import functools
import io
import struct

import numpy as np
from PIL import Image

import jpegdec_cases as C

ADOBE = lambda transform: (0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([transform]))
JFIF = (0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")


def write_cmyk(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img, "CMYK").save(b, "JPEG", **kw)
    return b.getvalue()


def strip_jfif(segs):
    return [(m, pl) for m, pl in segs if m != 0xE0]


def resized(w, h, luma):
    """An SOF edit: the size set to w x h and the first component's factors to `luma`."""
    def go(b):
        b[1:5] = struct.pack(">HH", h, w)
        b[7] = luma
        return bytes(b)
    return C.sof_edit(go)


# ---- the coefficient-domain writer ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _standard_tables():
    """The Annex K Huffman tables and two quantisation tables, as Pillow writes them: {(class, id): (counts, symbols)}, [DQT payloads]."""
    segs, _ = C.split(C.write(C.noise(8, 8, 3, 0), quality=90))
    huff, dqt = {}, []
    for m, pl in C.split_tables(segs):
        if m == 0xC4:
            huff[(pl[0] >> 4, pl[0] & 15)] = (list(pl[1:17]), list(pl[17:]))
        elif m == 0xDB:
            dqt.append(pl)
    return huff, dqt


def _codes(counts, symbols):
    """symbol -> (code, length) of a canonical code."""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[symbols[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def _put_value(w, v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def _put_block(w, blk, pred, dc, ac):
    """One block of 64 zigzag-ordered coefficients."""
    s, bits = _put_value(w, blk[0] - pred)
    w.put(*dc[s])
    if s:
        w.put(bits, s)
    run = 0
    last = max([k for k in range(1, 64) if blk[k]], default=0)
    for k in range(1, last + 1):
        if blk[k] == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac[0xF0])
            run -= 16
        s, bits = _put_value(w, blk[k])
        w.put(*ac[run << 4 | s])
        w.put(bits, s)
        run = 0
    if last < 63:
        w.put(*ac[0x00])


def coef_file(W, H, samp, color, seed, ri=0):
    """A sequential file of W x H with the sampling factors samp [(h, v)] per component and random small coefficients in every
    block (no forward DCT: Pillow judges the pixels).  color: "ycc" (JFIF), "rgb" (Adobe transform 0), "cmyk" (Adobe 0),
    "ycck" (Adobe 2).  Component 0 takes the first tables, every other the second."""
    huff, dqt = _standard_tables()
    nf = len(samp)
    ids = {"ycc": [1, 2, 3], "rgb": list(b"RGB"), "cmyk": list(b"CMYK"), "ycck": list(b"CMYK")}[color]
    sof = struct.pack(">BHHB", 8, H, W, nf) + b"".join(bytes([ids[c], h << 4 | v, min(c, 1)]) for c, (h, v) in enumerate(samp))
    sos = bytes([nf]) + b"".join(bytes([ids[c], 0x11 * min(c, 1)]) for c in range(nf)) + bytes([0, 63, 0])
    segs = [JFIF if color == "ycc" else ADOBE(2 if color == "ycck" else 0)] + [(0xDB, pl) for pl in dqt]
    segs += [(0xC0, sof)] + [(0xC4, bytes([tc << 4 | th]) + bytes(t[0]) + bytes(t[1])) for (tc, th), t in sorted(huff.items())]
    if ri:
        segs.append((0xDD, struct.pack(">H", ri)))
    segs.append((0xDA, sos))
    enc = [(_codes(*huff[(0, min(c, 1))]), _codes(*huff[(1, min(c, 1))])) for c in range(nf)]
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    nmcu = -(-W // (8 * hmax)) * -(-H // (8 * vmax))
    r = np.random.RandomState(seed)
    out, w, pred = bytearray(), C.BitWriter(), [0] * nf
    for m in range(nmcu):
        if ri and m and m % ri == 0:
            out += w.bytes() + bytes([0xFF, 0xD0 + (m // ri - 1) % 8])
            w, pred = C.BitWriter(), [0] * nf
        for c, (h, v) in enumerate(samp):
            for _ in range(h * v):
                blk = [0] * 64
                blk[0] = int(np.clip(pred[c] + r.randint(-12, 13), -60, 60))
                for k in r.randint(1, 10, r.randint(0, 5)):
                    blk[k] = int(r.randint(-9, 10))
                if r.randint(8) == 0:                        # a far coefficient: a long zero run (ZRL), or the block's last place
                    blk[int(r.choice([40, 63]))] = int(r.choice([-2, 1, 3]))
                _put_block(w, blk, pred[c], *enc[c])
                pred[c] = blk[0]
    return C.join(segs, bytes(out) + w.bytes() + b"\xff\xd9")


# (name, factors, colour): the layouts of the writer
LAYOUTS = [
    ("440", [(1, 2), (1, 1), (1, 1)], "ycc"),
    ("411", [(4, 1), (1, 1), (1, 1)], "ycc"),
    ("1x4", [(1, 4), (1, 1), (1, 1)], "ycc"),
    ("410", [(4, 2), (1, 1), (1, 1)], "ycc"),                # 10 blocks per MCU, MCUs of 32 x 16
    ("y3x1", [(3, 1), (1, 1), (1, 1)], "ycc"),
    ("y1_c2x2", [(1, 1), (2, 2), (2, 2)], "ycc"),            # luma coarser than chroma
    ("y4x1_c2x1", [(4, 1), (2, 1), (2, 1)], "ycc"),
    ("y1x4_c1x2", [(1, 4), (1, 2), (1, 1)], "ycc"),          # 1 x 2 between rows two to a group; box 1 x 4, MCUs of 8 x 32
    ("rgb_g2x1", [(2, 2), (2, 1), (1, 2)], "rgb"),
    ("cmyk_k2x2", [(1, 1), (1, 1), (1, 1), (2, 2)], "cmyk"),
    ("ycck_y2x2", [(2, 2), (1, 1), (1, 1), (2, 2)], "ycck"),
    ("cmyk_c1x2", [(1, 2), (1, 1), (2, 1), (2, 2)], "cmyk"),
]


def sizes(samp):
    """The smallest sizes at which each rule can go wrong: true widths 1, 2, 3 of a component 2 or 4 times coarser, true
    heights 1 and 2, 1 x 1 and 1 x N, one under / at / one over the MCU, and three MCU rows."""
    mw, mh = 8 * max(h for h, _ in samp), 8 * max(v for _, v in samp)
    return [(1, 1), (2, 1), (1, 3), (2, 3), (3, 2), (4, 3), (5, 5), (6, 2), (7, 1), (9, 3), (1, mh + 3), (mw - 1, mh - 1), (mw, mh), (mw + 1, mh + 1),
            (2 * mw + 3, 2 * mh + 5)]


@functools.lru_cache(maxsize=None)
def good():
    """(name, file): every file decodes with Pillow."""
    out = []
    # 1. Pillow writes
    for sub in (0, 1, 2):                                    # (Pillow sub-samples the first component only)
        for W, H in ((1, 1), (5, 3), (17, 15), (33, 20)):
            out.append((f"cmyk_s{sub}_{W}x{H}", write_cmyk(C.noise(W, H, 4, 10 * sub + W), quality=85, subsampling=sub)))
        out.append((f"cmyk_s{sub}_ri_row", write_cmyk(C.blocky(40, 31, 4, sub), quality=85, subsampling=sub, restart_marker_rows=1)))
        out.append((f"cmyk_s{sub}_ri_1", write_cmyk(C.noise(24, 17, 4, 50 + sub), quality=75, subsampling=sub, restart_marker_blocks=1)))
    for W, H in ((1, 1), (16, 16), (23, 19)):
        out.append((f"keep_rgb_{W}x{H}", C.write(C.noise(W, H, 3, W), quality=85, keep_rgb=True)))
    out.append(("keep_rgb_ri_row", C.write(C.blocky(40, 31, 3, 3), quality=85, keep_rgb=True, restart_marker_rows=1)))
    # 2. header edits of Pillow's files
    for W, H in ((16, 8), (32, 24), (48, 40), (15, 7)):       # 4:2:2 of W x H -> 4:4:0 of H x W: the same blocks per MCU and MCUs
        out.append((f"edit_440_{H}x{W}", C.edit(C.write(C.noise(W, H, 3, W + H), quality=80, subsampling=1), resized(H, W, 0x12))))
    f420 = C.write(C.noise(64, 32, 3, 7), quality=80, subsampling=2)
    out.append(("edit_411_128x16", C.edit(f420, resized(128, 16, 0x41))))
    out.append(("edit_1x4_16x128", C.edit(f420, resized(16, 128, 0x14))))
    out.append(("edit_411_97x9", C.edit(f420, resized(97, 9, 0x41))))
    out.append(("edit_440_ri_row", C.edit(C.write(C.noise(48, 40, 3, 8), quality=80, subsampling=1, restart_marker_rows=1), resized(40, 48, 0x12))))
    cmyk = write_cmyk(C.noise(33, 20, 4, 9), quality=85, subsampling=2)
    ycck = lambda s: C.replace(s, 0xEE, lambda pl: pl[:11] + b"\x02")
    out.append(("edit_ycck_s2", C.edit(cmyk, ycck)))
    out.append(("edit_ycck_s0_ri", C.edit(write_cmyk(C.noise(24, 17, 4, 11), quality=85, subsampling=0, restart_marker_blocks=2), ycck)))
    out.append(("edit_cmyk_no_adobe", C.edit(cmyk, lambda s: [(m, pl) for m, pl in s if m != 0xEE])))
    for sub in (1, 2):                                       # RGB-coded with sub-sampled G and B (no JFIF marker: Adobe decides)
        f = C.write(C.noise(33, 20, 3, 12 + sub), quality=85, subsampling=sub)
        out.append((f"edit_adobe_rgb_s{sub}", C.edit(f, lambda s: C.insert_before_sos(strip_jfif(s), [ADOBE(0)]))))
    plain = C.write(C.noise(23, 19, 3, 16), quality=75, subsampling=2)
    out.append(("edit_ids_rgb_s2", C.edit(plain, lambda s: C.component_ids(strip_jfif(s), list(b"RGB")))))
    out.append(("jfif_adobe0_is_ycc", C.edit(plain, lambda s: C.insert_before_sos(s, [ADOBE(0)]))))     # JFIF wins: a plain file
    out.append(("adobe1_is_ycc_440", C.edit(C.write(C.noise(16, 8, 3, 5), quality=80, subsampling=1),
                                            lambda s: C.insert_before_sos(strip_jfif(resized(8, 16, 0x12)(s)), [ADOBE(1)]))))
    # 3. the coefficient-domain writer
    for k, (name, samp, color) in enumerate(LAYOUTS):
        for j, (W, H) in enumerate(sizes(samp)):
            out.append((f"coef_{name}_{W}x{H}", coef_file(W, H, samp, color, 100 * k + j)))
        mw, mh = 8 * max(h for h, _ in samp), 8 * max(v for _, v in samp)
        out.append((f"coef_{name}_ri_1", coef_file(2 * mw + 1, 2 * mh, samp, color, 100 * k + 50, ri=1)))
        out.append((f"coef_{name}_ri_row", coef_file(3 * mw, 2 * mh + 1, samp, color, 100 * k + 51, ri=3)))
    out += long_plain()
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def long_plain():
    """Marker-less files of several 256-byte segments, segment ends inside a 10-block MCU included: what the sub-streams take."""
    return [("long_cmyk_s2", write_cmyk(C.noise(96, 80, 4, 30), quality=90, subsampling=2)),
            ("long_cmyk_s0", write_cmyk(C.smooth_detail(64, 48, 31)[:, :, [0, 1, 2, 0]].copy(), quality=95, subsampling=0)),
            ("long_440", C.edit(C.write(C.noise(80, 96, 3, 32), quality=85, subsampling=1), resized(96, 80, 0x12))),
            ("long_411", C.edit(C.write(C.noise(128, 64, 3, 33), quality=85, subsampling=2), resized(256, 32, 0x41))),
            ("long_410", coef_file(320, 128, [(4, 2), (1, 1), (1, 1)], "ycc", 34)),
            ("long_ycck_k2x2", coef_file(200, 150, [(1, 1), (1, 1), (1, 1), (2, 2)], "ycck", 35)),
            ("long_keep_rgb", C.write(C.noise(64, 48, 3, 36), quality=90, keep_rgb=True))]


def good_file(name):
    return dict(good())[name]


@functools.lru_cache(maxsize=None)
def malformed():
    """(name, file): broken files of the new layouts; the status is the restatement's."""
    out = []
    for name in ("long_cmyk_s2", "long_440", "long_410"):
        f = good_file(name)
        segs, tail = C.split(f)
        out += [(f"{name}_cut_{int(fr * 100)}", C._data_cut(f, fr)) for fr in (0.0, 0.5, 0.9)]
        out.append((f"{name}_bad_code", C.join(segs, tail[:C._safe(tail, len(tail) // 2)] + b"\xff\x00" * 4 + tail[C._safe(tail, len(tail) // 2):])))
        out.append((f"{name}_no_eoi", f[:-2]))
        out.append((f"{name}_rst_in_plain_file", C.join(segs, tail[:C._safe(tail, 300)] + b"\xff\xd0" + tail[C._safe(tail, 300):])))
    for name in ("cmyk_s2_ri_1", "edit_440_ri_row", "coef_410_ri_1", "coef_cmyk_k2x2_ri_row"):
        f = good_file(name)
        out.append((f"{name}_rst_missing", C._drop_rst(f, 1, "missing")))
        out.append((f"{name}_rst_wrong_index", C._drop_rst(f, 0, "index")))
        out.append((f"{name}_unit_1_bad_code", C._unit_edit(f, {1: b"\xff\x00" * 6})))
        out.append((f"{name}_unit_0_cut_short", C._unit_edit(f, {0: b"\x12"})))
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def refused():
    """(name, file, keywords of parse_jpeg, a word of the ValueError's message): refused even with ``all_layouts=True``."""
    plain = C.write(C.noise(16, 16, 3, 20), quality=75, subsampling=0)
    R = {n: f for n, f, _, _ in C.refused()}
    sof = lambda fn: C.edit(plain, C.sof_edit(fn))
    ncomp5 = C.edit(plain, lambda s: [(m, pl[:5] + b"\x05" + (pl[6:] * 2)[:15] if m == 0xC0 else bytes([5]) + (pl[1:7] * 2)[:10] + pl[-3:] if m == 0xDA else pl)
                                      for m, pl in s])
    prog_440 = C.edit(C.write(C.noise(16, 8, 3, 1), quality=80, subsampling=1, progressive=True),
                      lambda s: [(m, resized(8, 16, 0x12)([(0xC0, pl)])[0][1] if m == 0xC2 else pl) for m, pl in s])
    prog_cmyk = write_cmyk(C.noise(16, 16, 4, 2), quality=80, progressive=True)
    both = dict(all_layouts=True, progressive=True)
    return [
        ("two_components", R["two_components"], dict(all_layouts=True), "2 components (1, 3 or 4)"),
        ("five_components", ncomp5, dict(all_layouts=True), "5 components (1, 3 or 4)"),
        ("factor_0", sof(lambda b: C._set(b, 7, 0x01)), dict(all_layouts=True), "outside 1..4"),
        ("factor_5", sof(lambda b: C._set(b, 10, 0x15)), dict(all_layouts=True), "outside 1..4"),
        ("eleven_blocks", sof(lambda b: C._set(b, 7, 0x33)), dict(all_layouts=True), "blocks per MCU"),
        ("fractional_3_over_2", sof(lambda b: C._set(C._set(b, 7, 0x31) and b, 10, 0x21)), dict(all_layouts=True), "fractional"),
        ("fractional_vertical", sof(lambda b: C._set(C._set(b, 7, 0x13) and b, 13, 0x12)), dict(all_layouts=True), "fractional"),
        ("progressive_440", prog_440, both, "all_layouts covers sequential files only"),
        ("progressive_cmyk", prog_cmyk, both, "all_layouts covers sequential files only"),
        ("progressive_440_without_progressive", prog_440, dict(all_layouts=True), "progressive"),
        ("scan_of_one_component", R["scan_of_one_component"], dict(all_layouts=True), "more than one scan"),
        ("dqt_16_bit", R["dqt_16_bit"], dict(all_layouts=True), "16-bit"),
        ("precision_12", R["precision_12"], dict(all_layouts=True), "precision 12"),
        ("arithmetic", R["arithmetic"], dict(all_layouts=True), "arithmetic"),
        ("lossless", R["lossless"], dict(all_layouts=True), "lossless"),
        ("hierarchical", R["hierarchical"], dict(all_layouts=True), "hierarchical"),
    ]
