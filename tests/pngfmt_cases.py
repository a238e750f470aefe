"""Files shared by the tests of the PNG decoder's formats path (test_pngfmt_ref_cpu.py, test_pngfmt_host_cpu.py,
test_pngfmt_gpu.py): palette, 1 / 2 / 4 / 16 bits, Adam7.  Pillow writes what it can (P with bits=, 1, I;16); a hand writer
(zlib + struct, the filters of png_ref) writes the rest with a chosen filter type per pass and row and with the unused low
bits of a row's last byte set to ones.  good() files decode with Pillow; malformed() carry a status; refused() a word."""
from __future__ import annotations

import functools
import io
import itertools
import struct
import zlib

import numpy as np
from PIL import Image

import png_ref as R
import pngdec_ref as D
import pngfmt_ref as F

GREY16 = (0, 1, 254, 255, 256, 257, 0x7FFF, 0x8000, 0xFF00, 0xFFFF)


class Case:
    def __init__(self, name, file, W, H, ctype, depth, lace, filtered=None, samples=None, types=None):
        self.name, self.file, self.W, self.H, self.ctype, self.depth, self.lace = name, file, W, H, ctype, depth, lace
        self.filtered, self.samples, self.types = filtered, samples, types      # types: {(pass, row): filter type}

    @property
    def ch(self):
        return F.CHANNELS[self.ctype]


def _rng(seed):
    return np.random.default_rng(7100 + seed)


def noise(H, W, ctype, depth, seed=0):
    return _rng(seed).integers(0, 1 << depth, (H, W, F.CHANNELS[ctype]), dtype=np.uint16)


def pack(samples, depth):
    """[h, w, ch] samples -> [h, ceil(w ch depth / 8)] bytes; the unused low bits of the last byte are ONES."""
    h, w, ch = samples.shape
    if depth == 8:
        return samples.astype(np.uint8).reshape(h, w * ch)
    if depth == 16:
        return np.stack([samples >> 8, samples & 255], -1).astype(np.uint8).reshape(h, w * ch * 2)
    per = 8 // depth
    nb = (w + per - 1) // per
    s = np.full((h, nb * per), (1 << depth) - 1, np.uint16)
    s[:, :w] = samples[:, :, 0]
    shifts = np.array([8 - depth * (j + 1) for j in range(per)], np.uint16)
    return (s.reshape(h, nb, per) << shifts).sum(-1).astype(np.uint8)


def cycle(start=0):
    return lambda p, r: (start + p + r) % 5


def filtered_of(samples, ctype, depth, lace, ft):
    """-> (filtered bytes of all passes, {(pass, row): filter type})."""
    H, W, ch = samples.shape
    unit = F.unit_bytes(ch, depth)
    out, types = bytearray(), {}
    for p, (x0, y0, dx, dy, w, h) in enumerate(F.passes(W, H, lace)):
        if not (w and h):
            continue
        rows = pack(samples[y0::dy, x0::dx], depth)
        assert rows.shape == (h, F.row_bytes(w, ch, depth) - 1)
        zero = np.zeros(rows.shape[1], np.uint8)
        for r in range(h):
            t = ft(p, r)
            types[(p, r)] = t
            out.append(t)
            out += R.filter_row(rows[r], rows[r - 1] if r else zero, unit, t).tobytes()
    return bytes(out), types


def ihdr(W, H, depth, ctype, lace=0):
    return R.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, lace))


def make_file(W, H, depth, ctype, lace, stream, before=b"", idat=None):
    parts = [stream] if idat is None else [stream[i:i + idat] for i in range(0, len(stream), idat)]
    return D.SIGNATURE + ihdr(W, H, depth, ctype, lace) + before + b"".join(R.chunk(b"IDAT", p) for p in parts) + R.chunk(b"IEND", b"")


def hand(name, samples, ctype, depth, lace=0, ft=cycle(), palette=None, before=b"", level=6, idat=None):
    H, W, _ = samples.shape
    filtered, types = filtered_of(samples, ctype, depth, lace, ft)
    if palette is not None:
        before = R.chunk(b"PLTE", bytes(palette)) + before
    f = make_file(W, H, depth, ctype, lace, zlib.compress(filtered, level), before, idat)
    return Case(name, f, W, H, ctype, depth, lace, filtered, samples, types)


def _pil(name, im, **kw):
    buf = io.BytesIO()
    im.save(buf, "PNG", **kw)
    p = F.parse(buf.getvalue())
    return Case(name, buf.getvalue(), p["W"], p["H"], p["color_type"], p["depth"], p["interlace"])


def boundary_palette():
    """256 colours of test_luma_is_pillows_at_every_rounding_boundary's set: one channel sweeps, the others on an edge."""
    edge = [0, 1, 127, 128, 254, 255]
    rng = _rng(3)
    pal = np.zeros((256, 3), np.uint8)
    combos = list(itertools.product(edge, edge, range(3)))
    for i in range(256):
        a, b, k = combos[int(rng.integers(len(combos)))]
        pal[i, k], pal[i, (k + 1) % 3], pal[i, (k + 2) % 3] = int(rng.integers(256)), a, b
    return pal


def random_palette(n, seed):
    return _rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def adam7_sizes():
    """Every W x H in 1 .. 9 x 1 .. 9, interlaced, at RGB-8, grey-1 and RGBA-16."""
    c = []
    for (ctype, depth), tag in (((2, 8), "rgb8"), ((0, 1), "grey1"), ((6, 16), "rgba16")):
        for H in range(1, 10):
            for W in range(1, 10):
                c.append(hand(f"adam7_{tag}_{W}x{H}", noise(H, W, ctype, depth, 10 * H + W), ctype, depth, 1, cycle(W)))
    return c


@functools.lru_cache(maxsize=None)
def subbyte_tails():
    c = []
    for depth, wmax in ((1, 17), (2, 9), (4, 5)):
        for W in range(1, wmax + 1):
            for ctype in (0, 3):
                pal = random_palette(1 << depth, depth) if ctype == 3 else None
                c.append(hand(f"tail_d{depth}_c{ctype}_w{W}", noise(5, W, ctype, depth, W), ctype, depth, 0, lambda p, r: r, pal))
    return c


@functools.lru_cache(maxsize=None)
def filter_units():
    """Units of 2, 3, 4, 6 and 8 bytes with Sub / Average / Paeth on noise, W = 1, 2, 3."""
    c = []
    for ctype, depth in ((4, 8), (2, 8), (6, 8), (4, 16), (2, 16), (6, 16)):
        for W in (1, 2, 3):
            c.append(hand(f"unit{F.unit_bytes(F.CHANNELS[ctype], depth)}_c{ctype}_d{depth}_w{W}", noise(6, W, ctype, depth, W + depth),
                          ctype, depth, 0, lambda p, r: (1, 3, 4, 4, 3, 1)[r]))
    return c


@functools.lru_cache(maxsize=None)
def carries():
    c = []
    for k, H in enumerate((63, 64, 65, 129)):
        c.append(hand(f"carry_grey1_h{H}", noise(H, 11, 0, 1, H), 0, 1, 0, cycle(k)))
        c.append(hand(f"carry_rgba16_h{H}", noise(H, 3, 6, 16, H), 6, 16, 0, cycle(k + 2)))
    # (pass 3 has exactly 65 rows, so row 65 exists in six passes: their filter types still cover all five)
    c.append(hand("carry_adam7_9x521", noise(521, 9, 2, 8, 521), 2, 8, 1, lambda p, r: ((0, 1, 2, 2, 3, 4, 0)[p] + r) % 5))
    return c


@functools.lru_cache(maxsize=None)
def values():
    g = np.array(GREY16, np.uint16).reshape(2, 5, 1)
    ga = np.concatenate([g, noise(2, 5, 0, 16, 1)], 2)
    c = [hand("grey16_values", g, 0, 16), hand("grey_alpha16_values", ga, 4, 16),
         hand("grey16_values_adam7", g, 0, 16, 1), hand("grey2_ramp", np.arange(12, dtype=np.uint16).reshape(2, 6, 1) % 4, 0, 2),
         hand("grey4_ramp", np.arange(32, dtype=np.uint16).reshape(2, 16, 1) % 16, 0, 4)]
    pal = boundary_palette()
    idx = np.arange(256, dtype=np.uint16).reshape(16, 16, 1)
    c.append(hand("palette_boundary", idx, 3, 8, 0, cycle(), pal.tobytes()))
    c.append(hand("palette_boundary_adam7", idx, 3, 8, 1, cycle(), pal.tobytes()))
    short = np.array([[0, 1, 2, 3], [255, 2, 3, 255]], np.uint16)[:, :, None]
    c.append(hand("palette_short", short, 3, 8, 0, cycle(), random_palette(3, 1).tobytes()))
    c.append(hand("palette_trns", noise(4, 6, 3, 2, 5), 3, 2, 0, cycle(), random_palette(4, 2).tobytes(),
                  before=R.chunk(b"tRNS", b"\x00\x80\xff")))
    c.append(hand("rgb_suggested_plte", noise(3, 4, 2, 8, 6), 2, 8, 1, cycle(), random_palette(5, 3).tobytes()))
    c.append(hand("rgb16_photo_idat7", noise(7, 9, 2, 16, 8), 2, 16, 1, cycle(), idat=7))
    return c


@functools.lru_cache(maxsize=None)
def pillow_written():
    rng = _rng(9)
    c = []
    for bits in (1, 2, 4, 8):
        im = Image.frombytes("P", (21, 13), rng.integers(0, 1 << bits, (13, 21), dtype=np.uint8).tobytes())
        im.putpalette(random_palette(1 << bits, 20 + bits).tobytes())
        c.append(_pil(f"pil_P_bits{bits}", im, bits=bits))
    c.append(_pil("pil_1", Image.fromarray(rng.integers(0, 2, (9, 19), dtype=np.uint8) * 255).convert("1")))
    c.append(_pil("pil_I16", Image.fromarray(rng.integers(0, 65536, (6, 7), dtype=np.uint16))))
    assert [(k.ctype, k.depth) for k in c] == [(3, 1), (3, 2), (3, 4), (3, 8), (0, 1), (0, 16)]
    return c


@functools.lru_cache(maxsize=None)
def row_limits():
    """Rows of exactly ATTWARP_PNGDEC_MAX_ROW_BYTES = 49152 bytes, two of them; stored, so that the restatement is quick."""
    g = _rng(4).integers(0, 2, (2, 393208, 1), dtype=np.uint16)
    return [hand("rowmax_grey1", g, 0, 1, 0, cycle(1), level=0), hand("rowmax_grey1_adam7", g, 0, 1, 1, cycle(1), level=0),
            hand("rowmax_rgba16", noise(2, 6143, 6, 16, 5), 6, 16, 0, cycle(3), level=0)]


def good():
    """[Case]: every one decodes with Pillow."""
    return adam7_sizes() + subbyte_tails() + filter_units() + carries() + values() + pillow_written() + row_limits()


def small_good():
    """good() without the row-limit files."""
    return adam7_sizes() + subbyte_tails() + filter_units() + carries() + values() + pillow_written()


# ---- malformed ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def malformed():
    """[(name, file bytes)]: the device reports the restatement's status for each (none is 0)."""
    s = noise(9, 9, 2, 8, 77)
    W = H = 9
    filt, _ = filtered_of(s, 2, 8, 1, cycle())
    offs = F.pass_offsets(W, H, 3, 8, 1)
    c = []
    for p in (0, 3, 6):                                     # a filter byte 5 in pass 1, pass 4 and pass 7 (their last rows)
        rb = F.row_bytes(F.passes(W, H, 1)[p][4], 3, 8)
        end = offs[p + 1] if p < 6 else len(filt)
        bad = bytearray(filt)
        bad[end - rb] = 5
        c.append((f"filter5_pass{p + 1}", make_file(W, H, 8, 2, 1, zlib.compress(bytes(bad)))))
    plain, _ = filtered_of(s, 2, 8, 0, cycle())
    assert len(plain) != len(filt)
    c.append(("plain_stream_in_adam7_header", make_file(W, H, 8, 2, 1, zlib.compress(plain))))
    c.append(("adam7_stream_in_plain_header", make_file(W, H, 8, 2, 0, zlib.compress(filt))))
    stored = zlib.compress(filt, 0)                         # one stored block: 2 + 5 bytes in front of the filtered bytes
    assert stored[7:7 + len(filt)] == filt
    c.append(("cut_in_pass6", make_file(W, H, 8, 2, 1, stored[:7 + offs[5] + 9])))
    bad = bytearray(filtered_of(noise(5, 9, 0, 1, 3), 0, 1, 0, cycle())[0])
    bad[2 * 3] = 7
    c.append(("filter7_grey1", make_file(9, 5, 1, 0, 0, zlib.compress(bytes(bad)))))
    return c


def refused():
    """[(name, file bytes, word of the ValueError)]: what parse_png(all_formats=True) refuses before any launch."""
    s = R.chunk(b"IDAT", zlib.compress(b"\x00" * 8))
    end = R.chunk(b"IEND", b"")
    sig = D.SIGNATURE
    pl = lambda n: R.chunk(b"PLTE", bytes(n))
    badcrc = pl(6)[:-1] + bytes([pl(6)[-1] ^ 1])
    c = [(f"depth{d}_ctype{t}", sig + ihdr(1, 1, d, t) + pl(3) + s + end, "bit depth")
         for d, t in ((3, 0), (1, 2), (2, 2), (4, 2), (16, 3), (4, 4), (1, 6), (32, 0), (0, 0))]
    c += [("interlace2", sig + ihdr(1, 1, 8, 2, 2) + s + end, "interlace"),
          ("plte_missing", sig + ihdr(1, 1, 8, 3) + s + end, "PLTE"),
          ("plte_behind_idat", sig + ihdr(1, 1, 8, 3) + s + pl(3) + end, "PLTE"),
          ("plte_length_4", sig + ihdr(1, 1, 8, 3) + pl(4) + s + end, "PLTE"),
          ("plte_length_771", sig + ihdr(1, 1, 8, 3) + pl(771) + s + end, "PLTE"),
          ("plte_twice", sig + ihdr(1, 1, 8, 3) + pl(3) + pl(3) + s + end, "PLTE"),
          ("plte_crc", sig + ihdr(1, 1, 8, 3) + badcrc + s + end, "PLTE"),
          ("row_grey1_393209", sig + ihdr(393209, 2, 1, 0) + s + end, "size limit"),
          ("row_rgba16_6144", sig + ihdr(6144, 2, 16, 6) + s + end, "size limit"),
          ("row_grey1_393209_adam7", sig + ihdr(393209, 2, 1, 0, 1) + s + end, "size limit"),
          ("two_gib", sig + ihdr(6000, 44740, 16, 6, 1) + s + end, "size limit"),
          ("colour_type_5", sig + ihdr(1, 1, 8, 5) + s + end, "colour type"),
          ("signature", b"\x89PNX" + sig[4:] + ihdr(1, 1, 8, 2) + s + end, "signature"),
          ("idat_before_ihdr", sig + s + ihdr(1, 1, 8, 2) + end, "IHDR"), ("no_idat", sig + ihdr(1, 1, 8, 2) + end, "IDAT"),
          ("no_iend", sig + ihdr(1, 1, 8, 2) + s, "IEND"), ("zero_width", sig + ihdr(0, 1, 8, 2) + s + end, "size")]
    return c


def pillow(data, mode):
    """What Image.open(...).convert(...) gives, [H,W,C]; mode "keep": the file's channels without alpha at 8 bits, a
    palette file its palette's three."""
    im = Image.open(io.BytesIO(data))
    if mode == "keep":
        mode = "L" if data[25] in (0, 4) else "RGB"             # (IHDR's colour type: grey, grey + alpha)
    a = np.asarray(im.convert(mode))
    return a[:, :, None] if a.ndim == 2 else a
