"""Files shared by the PNG decoder's tests (test_pngdec_ref_cpu.py, test_pngdec_host_cpu.py, test_pngdec_gpu.py), built on
the host with zlib, Pillow and the encoder's restatement.  good() files decode with Pillow; malformed() files are each
derived from a good one and carry the status the decoder must report."""
from __future__ import annotations

import functools
import io
import struct
import zlib

import numpy as np
from PIL import Image

import png_cases as PC
import png_ref as R
import pngdec_ref as D

CTYPE = {1: 0, 2: 4, 3: 2, 4: 6}
MARKER = b"\x00\x00\xff\xff"


def filtered_cycle(img, start=0):
    """[H,W,C] -> filtered bytes with the filter type cycling 0 .. 4 over the rows."""
    H, W, C = img.shape
    rows = img.reshape(H, W * C)
    zero = np.zeros(W * C, np.uint8)
    out = bytearray()
    for r in range(H):
        ft = (start + r) % 5
        out.append(ft)
        out += R.filter_row(rows[r], rows[r - 1] if r else zero, C, ft).tobytes()
    return bytes(out)


def filtered_plain(img, ft=0):
    H, W, C = img.shape
    rows = img.reshape(H, W * C)
    zero = np.zeros(W * C, np.uint8)
    return b"".join(bytes([ft]) + R.filter_row(rows[r], rows[r - 1] if r else zero, C, ft).tobytes() for r in range(H))


def split(stream, size):
    if size is None:
        return [stream]
    return [stream[i:i + size] for i in range(0, len(stream), size)]


def make_png(W, H, ch, stream, idat=None, bad_crc=False):
    """A file around a zlib stream; idat: bytes per IDAT chunk (None: one chunk)."""
    out = D.SIGNATURE + R.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, CTYPE[ch], 0, 0, 0))
    parts = [R.chunk(b"IDAT", p) for p in split(stream, idat)]
    if bad_crc:
        parts[-1] = parts[-1][:-1] + bytes([parts[-1][-1] ^ 1])
    return out + b"".join(parts) + R.chunk(b"IEND", b"")


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, flush=None):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    if flush_at is None:
        return co.compress(data) + co.flush()
    return co.compress(data[:flush_at]) + co.flush(flush) + co.compress(data[flush_at:]) + co.flush()


def _fixed_code(w, sym):
    """One literal / length symbol of the fixed code into the LSB-first writer (codes are sent MSB first)."""
    if sym < 144:
        c, l = 0x30 + sym, 8
    elif sym < 256:
        c, l = 0x190 + sym - 144, 9
    elif sym < 280:
        c, l = sym - 256, 7
    else:
        c, l = 0xC0 + sym - 280, 8
    w.put(int(format(c, "0%db" % l)[::-1], 2), l)


def _fixed_match(w, length, dist):
    s, eb, ev = R.length_symbol(length)
    _fixed_code(w, s)
    w.put(ev, eb)
    d = max(k for k in range(30) if D.DIST_BASE[k] <= dist)
    w.put(int(format(d, "05b")[::-1], 2), 5)
    w.put(dist - D.DIST_BASE[d], D.DIST_EXTRA[d])


def far_match_stream(row):
    """Two identical rows of 32768 filtered bytes: the first stored, the second as matches at distance 32768, the first of
    them 258 long (zlib itself never reaches back further than 32506, so the block is written here)."""
    assert len(row) == 32768
    w = R.BitWriter()
    w.put(1, 1)
    w.put(1, 2)                        # final, fixed
    for _ in range(126):
        _fixed_match(w, 258, 32768)
    _fixed_match(w, 257, 32768)
    _fixed_match(w, 3, 32768)
    _fixed_code(w, 256)
    data = row + row
    return b"\x78\x01\x00" + struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + row + w.to_bytes() + struct.pack(">I", zlib.adler32(data))


def _photo():
    return PC.photo(37, 53, 3)


@functools.lru_cache(maxsize=None)
def photo_streams():
    """{name: zlib stream} of the 37 x 53 x 3 photo, filter type cycling."""
    f = filtered_cycle(_photo())
    half = len(f) // 2
    s = {"level0": zlib.compress(f, 0), "level1": zlib.compress(f, 1), "level9": zlib.compress(f, 9),
         "fixed": deflate(f, 6, zlib.Z_FIXED), "huffman_only": deflate(f, 6, zlib.Z_HUFFMAN_ONLY), "rle1": deflate(f, 1, zlib.Z_RLE),
         "sync_flush": deflate(f, 6, flush_at=half, flush=zlib.Z_SYNC_FLUSH),
         "full_flush": deflate(f, 6, flush_at=half, flush=zlib.Z_FULL_FLUSH)}
    assert s["sync_flush"].count(MARKER) == 1 and s["full_flush"].count(MARKER) == 1
    return s


def false_sync_image():
    img = np.full((4, 16, 3), 7, np.uint8)
    img[1, 5] = (9, 0, 0)
    img[1, 6] = (255, 255, 9)
    return img


def _pil_file(img, mode, **kw):
    buf = io.BytesIO()
    Image.fromarray(img if img.shape[2] > 1 else img[:, :, 0]).save(buf, "PNG", **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def good():
    """[(name, file bytes)]: every one decodes with Pillow."""
    c = []
    for name, s in photo_streams().items():
        for tag, size in (("one", None), ("idat7", 7), ("idat1", 1)):
            c.append((f"photo_{name}_{tag}", make_png(53, 37, 3, s, size)))
    fs = zlib.compress(filtered_plain(false_sync_image()), 0)
    assert fs.count(MARKER) == 1
    c.append(("false_sync", make_png(16, 4, 3, fs)))
    for name, img, filt, order in PC.cases():
        c.append((f"own_{name}", PC.reference(name, filt, order)))
    c.append(("own_500_sub", R.encode(PC.photo(500, 500, 3), "sub")))
    for mode, ch in (("L", 1), ("LA", 2), ("RGB", 3), ("RGBA", 4)):
        img = PC.photo(23, 31, ch, 20 + ch)
        for tag, kw in (("l0", dict(compress_level=0)), ("l1", dict(compress_level=1)), ("l6", dict(compress_level=6)),
                        ("l9", dict(compress_level=9)), ("opt", dict(optimize=True))):
            c.append((f"pil_{mode}_{tag}", _pil_file(img, mode, **kw)))
    for name, (h, w, ch) in (("1x1", (1, 1, 3)), ("1x300", (1, 300, 3)), ("300x1", (300, 1, 3)), ("row32768", (2, 32767, 1)),
                            ("row32769", (2, 32768, 1)), ("rgba", (9, 11, 4)), ("grey_alpha", (9, 11, 2))):
        img = PC.photo(h, w, ch, h + w)
        c.append((f"geo_{name}", make_png(w, h, ch, zlib.compress(filtered_cycle(img, 1), 6))))
    row = b"\x00" + PC.noise(1, 32767, 1, 9).tobytes()
    c.append(("far_match", make_png(32767, 2, 1, far_match_stream(row))))
    c.append(("distance1", make_png(40, 30, 3, zlib.compress(filtered_plain(np.full((30, 40, 3), 200, np.uint8)), 9))))
    # more sync points than ATTWARP_PNGDEC_MAX_UNITS are kept.  many_false: 480 patterns inside ONE stored block, none a block
    # boundary (256 kept, a chain of one unit).  many_flush: a full flush every 19 filtered bytes, 311 true boundaries, so the
    # 256th unit is the last kept one and decodes on through 56 more boundaries to the end (a chain of 256).
    spell = np.tile(np.frombuffer(b"\x00\x00\xff\xff\x55", np.uint8), 480)[:2400].reshape(2, 1200, 1)
    fs = zlib.compress(filtered_plain(spell), 0)
    assert fs.count(MARKER) == 480
    c.append(("many_false", make_png(1200, 2, 1, fs)))
    f = filtered_cycle(_photo())
    co = zlib.compressobj(6)
    fl = b"".join(co.compress(f[i:i + 19]) + co.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(f), 19)) + co.flush()
    assert fl.count(MARKER) > 300
    c.append(("many_flush", make_png(53, 37, 3, fl)))
    return c


@functools.lru_cache(maxsize=None)
def routes():
    """[(route, units on the chain, kept positions)] of good(), as PngFiles.routes() reports them: route 0 unit, 1 serial."""
    out = []
    for _, f in good():
        st, _, info = D.decode(f)
        assert st == D.OK
        out.append(({"unit": 0, "serial": 1}[info["route"]], info["chain"], info["nunits"]))
    return out


def good_file(name):
    return next(f for n, f in good() if n == name)


# ---- malformed ---------------------------------------------------------------------------------------------------------------
def _bits_stream(puts, tail=b"\x00\x00\x00\x01"):
    w = R.BitWriter()
    for v, n in puts:
        w.put(v, n)
    return b"\x78\x01" + w.to_bytes() + tail


@functools.lru_cache(maxsize=None)
def malformed():
    """[(name, file bytes, status)]; every file has a valid IHDR / IEND and, except wrong_crc, valid IDAT CRCs."""
    img = _photo()
    f = filtered_cycle(img)
    good_s = zlib.compress(f, 6)
    mk = lambda s, **kw: make_png(53, 37, 3, s, **kw)
    c = [("trunc_middle", mk(good_s[:len(good_s) // 2]), None), ("trunc_last", mk(good_s[:-1]), D.E_TRUNCATED)]
    for pos in (2, 40, len(good_s) // 3, len(good_s) // 2, 2 * len(good_s) // 3, len(good_s) - 9):
        s = bytearray(good_s)
        s[pos] ^= 0x10
        try:                                # keep the flip only when zlib itself rejects the stream (Adler included)
            zlib.decompress(bytes(s))
        except zlib.error:
            c.append((f"flip_{pos}", mk(bytes(s)), None))
    c.append(("wrong_adler", mk(good_s[:-1] + bytes([good_s[-1] ^ 1])), D.E_ADLER))
    c.append(("wrong_crc", mk(good_s, idat=100, bad_crc=True), D.E_CRC))
    st = bytearray(zlib.compress(f, 0))
    st[5] ^= 0x40                           # NLEN of the first stored block
    c.append(("stored_len", mk(bytes(st)), D.E_STORED_LEN))
    w = R.BitWriter()
    w.put(1, 1); w.put(1, 2)
    _fixed_match(w, 3, 1)
    _fixed_code(w, 256)
    c.append(("distance_before_start", mk(b"\x78\x01" + w.to_bytes() + b"\x00\x00\x00\x01"), D.E_DISTANCE))
    c.append(("oversubscribed", mk(_bits_stream([(1, 1), (2, 2), (0, 5), (0, 5), (15, 4)] + [(1, 3)] * 19)), D.E_CODE_LENGTHS))
    c.append(("one_too_many", mk(zlib.compress(f + b"\x00", 6)), D.E_OVERFLOW))
    c.append(("one_too_few", mk(zlib.compress(f[:-1], 6)), D.E_UNDERFLOW))
    bad = bytearray(f)
    bad[3 * (1 + 53 * 3)] = 5
    c.append(("filter5", mk(zlib.compress(bytes(bad), 6)), D.E_FILTER))
    c.append(("block_type3", mk(_bits_stream([(1, 1), (3, 2)])), D.E_BLOCK_TYPE))
    c.append(("zlib_header", mk(b"\x79" + good_s[1:]), D.E_ZLIB_HEADER))
    w = R.BitWriter()
    w.put(1, 1); w.put(1, 2)
    _fixed_code(w, 65)
    _fixed_code(w, 286)                     # a code of the fixed table that is no length symbol
    c.append(("length_symbol_286", mk(b"\x78\x01" + w.to_bytes() + b"\x00\x00\x00\x01"), D.E_SYMBOL))
    return c


def refused():
    """[(name, file bytes, word of the ValueError)]: what the host refuses before any launch."""
    s = zlib.compress(b"\x00" * 4)

    def hdr(depth=8, ctype=2, lace=0, W=1, H=1):
        return R.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, lace))

    idat, iend = R.chunk(b"IDAT", s), R.chunk(b"IEND", b"")
    sig = D.SIGNATURE
    return [("depth16", sig + hdr(depth=16) + idat + iend, "depth"), ("depth1", sig + hdr(depth=1, ctype=0) + idat + iend, "depth"),
            ("palette", sig + hdr(ctype=3) + R.chunk(b"PLTE", b"\0\0\0") + idat + iend, "colour type"),
            ("interlaced", sig + hdr(lace=1) + idat + iend, "interlace"), ("signature", b"\x89PNX" + sig[4:] + hdr() + idat + iend, "signature"),
            ("idat_before_ihdr", sig + idat + hdr() + iend, "IHDR"), ("no_idat", sig + hdr() + iend, "IDAT"),
            ("no_iend", sig + hdr() + idat, "IEND"), ("zero_width", sig + hdr(W=0) + idat + iend, "size"),
            ("too_wide", sig + hdr(W=20000) + idat + iend, "size limit")]


def pillow(data, mode):
    """What Image.open(...).convert(...) gives, [H,W,C]; mode "keep": the file's channels without alpha."""
    im = Image.open(io.BytesIO(data))
    if mode == "keep":
        mode = "L" if im.mode in ("L", "LA") else "RGB"
    a = np.asarray(im.convert(mode))
    return a[:, :, None] if a.ndim == 2 else a
