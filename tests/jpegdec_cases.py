"""Files shared by the JPEG decoder's tests (test_jpegdec_ref_cpu.py, test_jpegdec_host_cpu.py, test_jpegdec_gpu.py), built
at run time with Pillow's writer plus byte edits.  good() files decode with Pillow; malformed() files carry the status the
decoder must report (OK for the hostile-value files, whose pixels are the restatement's alone); refused() files are turned
away by the marker walk."""
from __future__ import annotations

import functools
import io
import struct

import numpy as np
from PIL import Image

import jpegdec_ref as D


# ---- pictures -----------------------------------------------------------------------------------------------------------------
def noise(W, H, ch=3, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (H, W, ch) if ch > 1 else (H, W)).astype(np.uint8)


def blocky(W, H, ch=3, seed=0):
    r = np.random.RandomState(seed)
    small = r.randint(0, 256, (-(-H // 5), -(-W // 5), ch)).astype(np.uint8)
    img = np.kron(small, np.ones((5, 5, 1), np.uint8))[:H, :W]
    return img if ch > 1 else img[:, :, 0]


def checker(W, H):
    """A slow ramp under a one-pixel checkerboard: the energy sits in the DC and in the last coefficients, with long zero
    runs in between (ZRL)."""
    y, x = np.mgrid[0:H, 0:W]
    img = 100 + x // 2 + y // 3 + 40 * ((x + y) % 2)
    return np.stack([img, img + 10, 255 - img], 2).astype(np.uint8)


def smooth_detail(W, H, seed=0):
    """A smooth gradient with sparse single-pixel detail."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(W + H - 2, 1)], 2).astype(np.int32)
    r = np.random.RandomState(seed)
    for _ in range(max(W * H // 40, 1)):
        img[r.randint(H), r.randint(W)] += r.randint(-90, 90)
    return np.clip(img, 0, 255).astype(np.uint8)


def write(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


def pillow(f, mode="RGB"):
    im = Image.open(io.BytesIO(f))
    if mode == "keep":
        mode = "L" if im.mode == "L" else "RGB"
    a = np.asarray(im.convert(mode))
    return a[:, :, None] if a.ndim == 2 else a


# ---- segments -----------------------------------------------------------------------------------------------------------------
def split(f):
    """A file -> ([(marker, payload)] up to and including SOS, everything behind the SOS header)."""
    segs, pos = [], 2
    while True:
        assert f[pos] == 0xFF
        m = f[pos + 1]
        L = struct.unpack(">H", f[pos + 2:pos + 4])[0]
        segs.append((m, bytes(f[pos + 4:pos + 2 + L])))
        pos += 2 + L
        if m == 0xDA:
            return segs, bytes(f[pos:])


def join(segs, tail, fill=0):
    out = bytearray(b"\xff\xd8")
    for m, pl in segs:
        out += b"\xff" * fill + bytes([0xFF, m]) + struct.pack(">H", len(pl) + 2) + pl
    return bytes(out) + tail


def edit(f, fn, **kw):
    segs, tail = split(f)
    return join(fn(segs), tail, **kw)


def replace(segs, marker, fn):
    return [(m, fn(pl) if m == marker else pl) for m, pl in segs]


def table_ids(segs, add):
    """Every quantisation and Huffman table moved to id + add, with the references of SOF and SOS."""
    out = []
    for m, pl in segs:
        b = bytearray(pl)
        if m == 0xDB:
            for q in range(0, len(b), 65):
                b[q] += add
        elif m == 0xC4:
            q = 0
            while q < len(b):
                b[q] += add
                q += 17 + sum(b[q + 1:q + 17])
        elif m in (0xC0, 0xC1):
            for i in range(b[5]):
                b[8 + 3 * i] += add
        elif m == 0xDA:
            for i in range(b[0]):
                b[2 + 2 * i] += add | add << 4
        out.append((m, bytes(b)))
    return out


def merge(segs, marker):
    """All segments of one kind merged into the first."""
    payload = b"".join(pl for m, pl in segs if m == marker)
    out, done = [], False
    for m, pl in segs:
        if m != marker:
            out.append((m, pl))
        elif not done:
            out.append((m, payload))
            done = True
    return out


def split_tables(segs):
    """One table per DQT / DHT segment."""
    out = []
    for m, pl in segs:
        if m == 0xDB:
            out += [(m, pl[q:q + 65]) for q in range(0, len(pl), 65)]
        elif m == 0xC4:
            q = 0
            while q < len(pl):
                ln = 17 + sum(pl[q + 1:q + 17])
                out.append((m, pl[q:q + ln]))
                q += ln
        else:
            out.append((m, pl))
    return out


def component_ids(segs, ids):
    out = []
    for m, pl in segs:
        b = bytearray(pl)
        if m in (0xC0, 0xC1):
            for i in range(b[5]):
                b[6 + 3 * i] = ids[i]
        elif m == 0xDA:
            for i in range(b[0]):
                b[1 + 2 * i] = ids[i]
        out.append((m, bytes(b)))
    return out


def insert_before_sos(segs, new):
    return segs[:-1] + list(new) + segs[-1:]


def sof_edit(fn):
    def go(segs):
        return [(m, fn(bytearray(pl)) if m in (0xC0, 0xC1) else pl) for m, pl in segs]
    return go


def _set(b, i, v):
    b[i] = v
    return bytes(b)


# ---- hand-written files: tiny tables of our own, so that any symbol sequence can be written ---------------------------------------
DC_TINY = ([1, 1] + [0] * 14, [0, 15])                       # '0' -> category 0, '10' -> category 15
AC_TINY = ([1, 1, 1, 1] + [0] * 12, [0x00, 0xF1, 0xF0, 0xE1])  # '0' EOB, '10' run 15 + 1 bit, '110' ZRL, '1110' run 14 + 1 bit


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]

    def bytes(self):
        b = self.bits + [1] * (-len(self.bits) % 8)
        out = bytearray()
        for i in range(0, len(b), 8):
            v = int("".join(map(str, b[i:i + 8])), 2)
            out.append(v)
            if v == 0xFF:
                out.append(0)
        return bytes(out)


def hand_file(W, H, data, dc=DC_TINY, ac=AC_TINY, q=1, ri=0, eoi=b"\xff\xd9"):
    """A grey file with the (counts, symbols) tables dc / ac, a constant quantisation table, a DRI segment if ri, the given
    entropy data and whatever is to stand where the EOI does."""
    segs = [(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"), (0xDB, bytes([0]) + bytes([q]) * 64),
            (0xC0, struct.pack(">BHHB", 8, H, W, 1) + bytes([1, 0x11, 0])),
            (0xC4, bytes([0x00]) + bytes(dc[0]) + bytes(dc[1]) + bytes([0x10]) + bytes(ac[0]) + bytes(ac[1]))]
    if ri:
        segs.append((0xDD, struct.pack(">H", ri)))
    segs.append((0xDA, bytes([1, 1, 0x00, 0, 63, 0])))
    return join(segs, data + eoi)


def tiny_file(W, H, data, q=1):
    """A grey file with DC_TINY / AC_TINY, a constant quantisation table and the given entropy data."""
    return hand_file(W, H, data, q=q)


def _dc15(w, v):
    w.put(0b10, 2)
    w.put(v if v >= 0 else v + 32767, 15)


def _tiny_dc_overflow():
    w = BitWriter()
    for v in (32767, 32767, 32767, -32767, -20000, 16384):      # the predictor passes 2^15 and comes back
        _dc15(w, v)
        w.put(0, 1)
    return tiny_file(48, 8, w.bytes())


def _tiny_run_past_63():
    w = BitWriter()
    w.put(0, 1)                                              # DC category 0
    for _ in range(4):                                       # k = 16, 32, 48, then 64
        w.put(0b10, 2)
        w.put(1, 1)
    w.put(0, 1)
    return tiny_file(8, 8, w.bytes())


def _tiny_zrl_past_63():
    w = BitWriter()
    w.put(0, 1)
    for _ in range(4):                                       # k = 17, 33, 49, then 65 > 64
        w.put(0b110, 3)
    w.put(0, 1)
    return tiny_file(8, 8, w.bytes())


def _tiny_zrl_to_the_end():
    """Three ZRL and a run of 14 reach coefficient 63 exactly: decodable, and the block ends without an EOB."""
    w = BitWriter()
    w.put(0, 1)
    for _ in range(3):
        w.put(0b110, 3)
    w.put(0b1110, 4)                                         # k = 49, run 14: coefficient 63
    w.put(1, 1)
    return tiny_file(8, 8, w.bytes())


# ---- the corpus ------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 2), (2, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 15), (17, 33), (40, 31), (64, 48)]


@functools.lru_cache(maxsize=None)
def good():
    out = []
    for k, (W, H) in enumerate(SIZES):
        sub = k % 3
        out.append((f"noise_{W}x{H}_s{sub}", write(noise(W, H, 3, k), quality=75, subsampling=sub)))
        out.append((f"blocky_{W}x{H}_s{(sub + 1) % 3}", write(blocky(W, H, 3, k), quality=90, subsampling=(sub + 1) % 3)))
    for sub in (0, 1, 2):                                    # every sampling at the sizes where the edge rules meet
        for W, H in ((1, 1), (2, 1), (1, 2), (17, 33), (40, 31)):
            out.append((f"edge_{W}x{H}_s{sub}", write(noise(W, H, 3, 100 + sub), quality=95, subsampling=sub)))
    out.append(("grey_17x15", write(noise(17, 15, 1, 3), quality=75)))
    out.append(("grey_64x48_q100", write(blocky(64, 48, 1, 4), quality=100)))
    out.append(("grey_2x2_factors", edit(write(noise(20, 13, 1, 5), quality=80), sof_edit(lambda b: _set(b, 7, 0x22)))))
    out.append(("sof1", edit(write(noise(24, 17, 3, 6), quality=75), lambda s: [(0xC1 if m == 0xC0 else m, pl) for m, pl in s])))
    for sub in (0, 2):
        out.append((f"q1_s{sub}", write(noise(33, 20, 3, 7), quality=1, subsampling=sub)))
        out.append((f"q100_s{sub}", write(noise(33, 20, 3, 8), quality=100, subsampling=sub)))
    out.append(("q100_optimize", write(noise(48, 40, 3, 9), quality=100, subsampling=0, optimize=True)))
    out.append(("q20_optimize", write(blocky(40, 31, 3, 10), quality=20, optimize=True)))
    out.append(("zrl", write(checker(40, 24), quality=60, subsampling=0)))
    base = noise(40, 24, 3, 12)                              # 4:2:0: 3 x 2 MCUs; 4:4:4: 5 x 3
    out.append(("ri_1", write(base, quality=85, subsampling=2, restart_marker_blocks=1)))
    out.append(("ri_row", write(base, quality=85, subsampling=0, restart_marker_rows=1)))
    out.append(("ri_not_dividing", write(base, quality=85, subsampling=0, restart_marker_blocks=4)))
    out.append(("ri_larger", write(base, quality=85, subsampling=2, restart_marker_blocks=50)))
    out.append(("ri_wrap", write(noise(64, 48, 3, 13), quality=100, subsampling=0, restart_marker_blocks=2)))   # 24 units
    out.append(("ri_wrap_grey", write(noise(56, 40, 1, 14), quality=100, restart_marker_blocks=1)))             # 35 units
    out.append(("ri_stuffed_end", stuffed_end()))
    out.append(("big_200x136", write(smooth_detail(200, 136, 15), quality=75, subsampling=2, restart_marker_rows=1)))
    plain = write(noise(23, 19, 3, 16), quality=75, subsampling=2)
    out.append(("ids_2_3", edit(plain, lambda s: table_ids(s, 2))))
    out.append(("merged", edit(plain, lambda s: merge(merge(s, 0xDB), 0xC4))))
    out.append(("split", edit(write(noise(23, 19, 3, 16), quality=75, subsampling=1), lambda s: split_tables(merge(merge(s, 0xDB), 0xC4)))))
    out.append(("redefined", edit(plain, lambda s: [(0xDB, bytes([0]) + bytes([9]) * 64), (0xC4, bytes([0x00, 0, 1] + [0] * 14 + [3]))] + s)))
    out.append(("comp_ids_012", edit(plain, lambda s: component_ids(s, [0, 1, 2]))))
    trap = b"\xff\xd0\xff\xda\x00\x03\xff\xd9\xff\xc4"
    out.append(("app_com_traps", edit(plain, lambda s: insert_before_sos(s, [(0xE1, b"Exif\0\0" + trap), (0xFE, trap), (0xED, trap)]))))
    out.append(("fill_bytes", edit(plain, lambda s: s, fill=3)))
    out.append(("behind_eoi", plain + b"\xff\xd0junk\xff\xda\x00"))
    out.append(("exif_orientation", write(noise(12, 20, 3, 17), quality=75, exif=_exif_rotated())))
    out.append(("tiny_zrl_to_the_end", _tiny_zrl_to_the_end()))
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    return out


def _exif_rotated():
    ex = Image.Exif()
    ex[0x0112] = 6
    return ex.tobytes()


@functools.lru_cache(maxsize=None)
def stuffed_end():
    """A restart file one of whose units ends in a stuffed FF 00 right in front of its restart marker."""
    for seed in range(STUFFED_SEEDS[0], STUFFED_SEEDS[1]):
        f = write(noise(32, 24, 1, seed), quality=100, restart_marker_blocks=1)
        s = split(f)[1]
        if any(s[i:i + 2] == b"\xff\x00" and s[i + 2] == 0xFF and 0xD0 <= s[i + 3] <= 0xD7 for i in range(len(s) - 3)):
            return f
    raise AssertionError("no unit ending in FF 00 found")


STUFFED_SEEDS = (0, 400)


def good_file(name):
    return dict(good())[name]


def _data_cut(f, frac):
    segs, tail = split(f)
    return join(segs, tail[:int(len(tail) * frac)])


def _drop_rst(f, which, mode):
    """The which-th restart marker removed / doubled / given the next index."""
    segs, tail = split(f)
    pos = [i for i in range(len(tail) - 1) if tail[i] == 0xFF and 0xD0 <= tail[i + 1] <= 0xD7]
    i = pos[which]
    if mode == "missing":
        tail = tail[:i] + tail[i + 2:]
    elif mode == "extra":
        tail = tail[:i] + tail[i:i + 2] + tail[i:]
    else:
        tail = tail[:i + 1] + bytes([0xD0 + ((tail[i + 1] + 1) & 7)]) + tail[i + 2:]
    return join(segs, tail)


def _unit_edit(f, edits):
    """{unit: new bytes} in a restart file: the bytes between the restart markers around those units replaced."""
    segs, tail = split(f)
    pos = [i for i in range(len(tail) - 1) if tail[i] == 0xFF and 0xD0 <= tail[i + 1] <= 0xD7]
    bounds = list(zip([0] + [p + 2 for p in pos], pos + [len(tail) - 2]))
    out = bytearray()
    for k, (a, b) in enumerate(bounds):
        out += edits.get(k, tail[a:b]) + tail[b:b + 2]
    return join(segs, bytes(out))


@functools.lru_cache(maxsize=None)
def malformed():
    """(name, file, status)."""
    base = good_file("noise_64x48_s1")
    rst = good_file("ri_wrap")
    segs, tail = split(base)
    out = [(f"cut_{int(fr * 100)}", _data_cut(base, fr), D.E_TRUNCATED) for fr in (0.0, 0.1, 0.5, 0.9)]
    out.append(("cut_in_restart_file", _data_cut(rst, 0.5), D.E_RESTART))
    out.append(("no_eoi", base[:-2], D.E_NO_EOI))
    out.append(("eoi_replaced", base[:-1] + b"\xe0", D.E_NO_EOI))
    out.append(("ff_last_byte", base[:-1], D.E_NO_EOI))
    out.append(("all_ones_code", join(segs, b"\xff\x00" * 4 + tail), D.E_HUFFMAN))
    out.append(("run_past_63", _tiny_run_past_63(), D.E_COEFF))
    out.append(("zrl_past_63", _tiny_zrl_past_63(), D.E_COEFF))
    out.append(("rst_missing", _drop_rst(rst, 5, "missing"), D.E_RESTART))
    out.append(("rst_extra", _drop_rst(rst, 9, "extra"), D.E_RESTART))
    out.append(("rst_wrong_index", _drop_rst(rst, 13, "index"), D.E_RESTART))
    out.append(("rst_in_plain_file", join(segs, tail[:_safe(tail, 40)] + b"\xff\xd0" + tail[_safe(tail, 40):]), D.E_RESTART))
    out.append(("dht_inside_data", join(segs, tail[:_safe(tail, len(tail) // 2)] + b"\xff\xc4\x00\x02" + tail[_safe(tail, len(tail) // 2):]), D.E_TRUNCATED))
    out.append(("dht_inside_restart_data", _marker_in(rst), D.E_RESTART))
    # errors inside single units of a 24-unit file: the lowest failing unit decides
    out.append(("units_7_and_15_all_ones", _unit_edit(rst, {15: b"", 7: b"\xff\x00" * 6}), D.E_HUFFMAN))
    out.append(("units_20_all_ones_3_empty", _unit_edit(rst, {20: b"\xff\x00" * 6, 3: b""}), D.E_TRUNCATED))
    out.append(("unit_5_cut_short", _unit_edit(rst, {5: b"\x12"}), D.E_TRUNCATED))
    # hostile but decodable
    out.append(("dc_predictor_overflow", _tiny_dc_overflow(), D.OK))
    q100 = good_file("q100_s0")
    for k in (16, 255):
        out.append((f"quant_{k}", edit(q100, lambda s: replace(s, 0xDB, lambda pl: b"".join(pl[q:q + 1] + bytes([k]) * 64 for q in range(0, len(pl), 65)))), D.OK))
    names = [n for n, _, _ in out]
    assert len(set(names)) == len(names)
    return out


def _safe(tail, h):
    while tail[h - 1] == 0xFF or tail[h] == 0:               # (not between an FF and its 00)
        h += 1
    return h


def _marker_in(f):
    segs, tail = split(f)
    h = _safe(tail, len(tail) // 2)
    return join(segs, tail[:h] + b"\xff\xc4\x00\x02" + tail[h:])


@functools.lru_cache(maxsize=None)
def refused():
    """(name, file, exception, a word of its message)."""
    rgb = noise(16, 16, 3, 20)
    plain = write(rgb, quality=75, subsampling=0)
    grey = write(noise(16, 16, 1, 21), quality=75)

    def sof(fn):
        return edit(plain, sof_edit(fn))

    def ncomp(n):
        def go(segs):
            out = []
            for m, pl in segs:
                if m == 0xC0:
                    pl = pl[:5] + bytes([n]) + (pl[6:] + pl[6:])[:3 * n]
                elif m == 0xDA:
                    pl = bytes([n]) + (pl[1:7] + pl[1:7])[:2 * n] + pl[-3:]
                out.append((m, pl))
            return out
        return go

    def dht(fn):
        first = [True]

        def go(pl):
            if first[0]:
                first[0] = False
                return fn(bytearray(pl))
            return pl
        return edit(plain, lambda s: replace(s, 0xC4, go))

    strip = lambda s: [(m, pl) for m, pl in s if m != 0xE0]
    out = [
        ("progressive", write(rgb, quality=75, progressive=True), ValueError, "progressive"),
        ("lossless", edit(plain, lambda s: [(0xC3 if m == 0xC0 else m, pl) for m, pl in s]), ValueError, "lossless"),
        ("arithmetic", edit(plain, lambda s: [(0xC9 if m == 0xC0 else m, pl) for m, pl in s]), ValueError, "arithmetic"),
        ("hierarchical", edit(plain, lambda s: [(0xC5 if m == 0xC0 else m, pl) for m, pl in s]), ValueError, "hierarchical"),
        ("precision_12", sof(lambda b: _set(b, 0, 12)), ValueError, "precision"),
        ("two_components", edit(plain, ncomp(2)), ValueError, "components"),
        ("four_components", edit(plain, ncomp(4)), ValueError, "components"),
        ("sampling_1x2", sof(lambda b: _set(b, 7, 0x12)), ValueError, "sampling"),
        ("sampling_chroma_2x1", sof(lambda b: _set(b, 10, 0x21)), ValueError, "sampling"),
        ("sampling_4x1", sof(lambda b: _set(b, 7, 0x41)), ValueError, "sampling"),
        ("dqt_16_bit", edit(plain, lambda s: replace(s, 0xDB, lambda pl: bytes([pl[0] | 0x10]) + b"".join(b"\0" + pl[k:k + 1] for k in range(1, 65)))), ValueError, "16-bit"),
        ("adobe_rgb", edit(plain, lambda s: insert_before_sos(s, [(0xEE, b"Adobe\0\x64\0\0\0\0\0")])), ValueError, "RGB"),
        ("ids_rgb", edit(plain, lambda s: component_ids(strip(s), list(b"RGB"))), ValueError, "RGB"),
        ("scan_of_one_component", edit(plain, lambda s: replace(s, 0xDA, lambda pl: bytes([1]) + pl[1:3] + pl[-3:])), ValueError, "scan"),
        ("scan_out_of_order", edit(plain, lambda s: replace(s, 0xDA, lambda pl: pl[:1] + pl[3:5] + pl[1:3] + pl[5:])), ValueError, "scan"),
        ("spectral_selection", edit(plain, lambda s: replace(s, 0xDA, lambda pl: pl[:-3] + bytes([0, 5, 0]))), ValueError, "spectral"),
        ("table_never_defined", edit(plain, lambda s: replace(s, 0xDA, lambda pl: pl[:2] + bytes([0x22]) + pl[3:])), ValueError, "never defined"),
        ("quant_never_defined", sof(lambda b: _set(b, 8, 3)), ValueError, "never defined"),
        ("dht_over_subscribed", dht(lambda b: _set(b, 1, 3)), ValueError, "over-subscribed"),
        ("dht_past_segment", dht(lambda b: _set(b, 16, 100)), ValueError, "past the segment"),
        ("dht_300_symbols", edit(plain, lambda s: insert_before_sos(s, [(0xC4, bytes([0x13] + [0] * 7 + [100, 100, 100] + [0] * 6) + bytes(300))])),
         ValueError, "exceed 256"),
        ("zero_height", sof(lambda b: _set(_set(b, 1, 0) and b, 2, 0)), ValueError, "size"),
        ("zero_width", sof(lambda b: _set(_set(b, 3, 0) and b, 4, 0)), ValueError, "size"),
        ("too_many_units", edit(write(np.zeros((2056, 2056), np.uint8), quality=10), lambda s: insert_before_sos(s, [(0xDD, b"\0\x01")])), ValueError, "limit"),
        ("ends_in_headers", plain[:60], OSError, "headers"),
        ("ends_in_sos", plain[:plain.index(b"\xff\xda") + 5], OSError, "headers"),
        ("not_a_jpeg", b"\x89PNG\r\n\x1a\n" + plain, ValueError, "signature"),
        ("grey_scan_wrong_id", edit(grey, lambda s: replace(s, 0xDA, lambda pl: pl[:1] + b"\x07" + pl[2:])), ValueError, "scan"),
    ]
    return out
