"""Plain Python / numpy restatement of what the PNG decoder does behind inflate for every format of the specification
(attwarp_amd/csrc/pngfmt_blocks.hpp, pngdec_unfilter_formats_kernel, png.parse_png(all_formats=True)): the
extended chunk walk and its refusals, the Adam7 pass geometry, the per-pass filters on byte units, bit unpacking, the
palette and Pillow's conversion rules.  The inflate part and the status order are pngdec_ref's.  No product code."""
from __future__ import annotations

import struct
import zlib

import numpy as np

import pngdec_ref as D

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


# ---- the host's part: chunks ----------------------------------------------------------------------------------------------
def parse(data):
    """File bytes -> dict(W, H, color_type, depth, interlace, palette, chunks=[(payload, stated crc)], stream).  ValueError
    carries the word of the refusal."""
    data = bytes(data)
    if data[:8] != D.SIGNATURE:
        raise ValueError("signature")
    pos, ihdr, chunks, seen_iend, idat_done, plte = 8, None, [], False, False, None
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError("chunk: truncated")
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if pos + 12 + n > len(data):
            raise ValueError("chunk: truncated")
        payload, crc = data[pos + 8:pos + 8 + n], struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        if ihdr is None and kind != b"IHDR":
            raise ValueError("IHDR: not the first chunk")
        if kind == b"IHDR":
            if ihdr is not None or n != 13:
                raise ValueError("IHDR: misplaced")
            if zlib.crc32(kind + payload) != crc:
                raise ValueError("IHDR: CRC")
            ihdr = struct.unpack(">IIBBBBB", payload)
        elif kind == b"IDAT":
            if idat_done:
                raise ValueError("IDAT: not consecutive")
            chunks.append((payload, crc))
        elif kind == b"IEND":
            if not chunks:
                raise ValueError("IDAT: missing")
            seen_iend = True
            break
        else:
            if chunks:
                idat_done = True
            if not (kind[0] & 32) and kind != b"PLTE":
                raise ValueError("chunk: unknown critical chunk")
            if kind == b"PLTE" and ihdr[3] == 3:          # (in a colour file it is a suggestion and skipped)
                if plte is not None:
                    raise ValueError("PLTE: a second one")
                if chunks:
                    raise ValueError("PLTE: behind the first IDAT")
                if n == 0 or n % 3 or n > 768:
                    raise ValueError("PLTE: length")
                if zlib.crc32(kind + payload) != crc:
                    raise ValueError("PLTE: CRC")
                plte = payload
        pos += 12 + n
    if ihdr is None:
        raise ValueError("IHDR: missing")
    if not seen_iend:
        raise ValueError("IEND: missing")
    W, H, depth, ctype, comp, filt, lace = ihdr
    if ctype not in DEPTHS:
        raise ValueError("colour type")
    if depth not in DEPTHS[ctype]:
        raise ValueError("bit depth")
    if comp != 0 or filt != 0:
        raise ValueError("compression / filter method")
    if lace > 1:
        raise ValueError("interlace")
    if W == 0 or H == 0:
        raise ValueError("size")
    if ctype == 3 and plte is None:
        raise ValueError("PLTE: missing")
    ch = CHANNELS[ctype]
    if row_bytes(W, ch, depth) > D.MAX_ROW_BYTES or filt_bytes(W, H, ch, depth, lace) >= 1 << 31:
        raise ValueError("size limit")
    return dict(W=W, H=H, color_type=ctype, depth=depth, interlace=lace, palette=plte or b"", chunks=chunks,
                stream=b"".join(c[0] for c in chunks))


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def row_bytes(w, ch, depth):
    return 1 + (w * ch * depth + 7) // 8


def unit_bytes(ch, depth):
    return max(1, ch * depth // 8)


def passes(W, H, interlace):
    """[(x0, y0, dx, dy, w, h)]: seven for Adam7 (empty ones included), one otherwise."""
    if not interlace:
        return [(0, 0, 1, 1, W, H)]
    out = []
    for x0, y0, dx, dy in ADAM7:
        w = -(-(W - x0) // dx) if W > x0 else 0
        h = -(-(H - y0) // dy) if H > y0 else 0
        out.append((x0, y0, dx, dy, w, h))
    return out


def pass_sizes(W, H, ch, depth, interlace):
    """Filtered bytes of each pass; an empty pass has none."""
    return [h * row_bytes(w, ch, depth) if w and h else 0 for _, _, _, _, w, h in passes(W, H, interlace)]


def pass_offsets(W, H, ch, depth, interlace):
    sizes = pass_sizes(W, H, ch, depth, interlace)
    return [sum(sizes[:k]) for k in range(len(sizes))]


def filt_bytes(W, H, ch, depth, interlace):
    return sum(pass_sizes(W, H, ch, depth, interlace))


# ---- behind the filters ---------------------------------------------------------------------------------------------------------
def unpack(rows, w, ch, depth):
    """[h, ceil(w ch depth / 8)] reconstructed bytes -> [h, w, ch] samples (uint16): below 8 bits MSB first in the byte, the
    tail bits of the last byte dropped; 16 bits big-endian."""
    h = rows.shape[0]
    if depth == 8:
        return rows.reshape(h, w, ch).astype(np.uint16)
    if depth == 16:
        r = rows.reshape(h, w, ch, 2).astype(np.uint16)
        return r[..., 0] << 8 | r[..., 1]
    per = 8 // depth
    shifts = np.array([8 - depth * (j + 1) for j in range(per)], np.uint16)
    s = (rows[:, :, None].astype(np.uint16) >> shifts) & ((1 << depth) - 1)
    return s.reshape(h, -1)[:, :w].reshape(h, w, 1)


def to8(samples, ctype, depth, palette):
    """[H, W, ch] samples -> the file's channels at 8 bits without alpha, [H, W, 1 or 3], by Pillow's rules:
    grey below 8 bits x 255 / 85 / 17; 16-bit GREY saturates, min(v, 255); every other 16-bit sample its high byte;
    a palette index its PLTE entry, black at or past the entries."""
    s = samples.astype(np.uint32)
    if ctype == 3:
        pal = np.zeros((256, 3), np.uint8)
        e = np.frombuffer(palette, np.uint8).reshape(-1, 3)
        pal[:len(e)] = e
        return pal[s[:, :, 0]]
    if ctype == 0:
        if depth == 16:
            s = np.minimum(s, 255)
        elif depth < 8:
            s = s * (255 // ((1 << depth) - 1))
        return s.astype(np.uint8)
    if depth == 16:
        s = s >> 8
    keep = 1 if ctype == 4 else 3
    return np.ascontiguousarray(s[:, :, :keep]).astype(np.uint8)


def unfilter(filtered, W, H, ctype, depth, interlace):
    """Filtered bytes of all passes -> (status, [H, W, ch] samples): every pass on its own, the row above its first row
    zero, the filters' pixel `unit_bytes` wide.  A filter byte above 4 in any pass is E_FILTER."""
    ch = CHANNELS[ctype]
    unit = unit_bytes(ch, depth)
    out = np.zeros((H, W, ch), np.uint16)
    off, bad = 0, False
    for x0, y0, dx, dy, w, h in passes(W, H, interlace):
        if not (w and h):
            continue
        rb = row_bytes(w, ch, depth)
        st, rows = D.unfilter(filtered[off:off + h * rb], h, (rb - 1) // unit, unit)
        off += h * rb
        if st:
            bad = True
            continue
        out[y0::dy, x0::dx] = unpack(rows.reshape(h, rb - 1), w, ch, depth)
    assert off == len(filtered)
    return (D.E_FILTER, None) if bad else (D.OK, out)


def decode(data, mode="RGB", order="rgb", check_crc=True):
    """File bytes -> (status, image [H, W, C] or None, info); ValueError for what the host refuses."""
    p = parse(data)
    ch = CHANNELS[p["color_type"]]
    W, H, depth, lace = p["W"], p["H"], p["depth"], p["interlace"]
    st, filtered, info = D.decode_stream(p["stream"], filt_bytes(W, H, ch, depth, lace))
    info["filtered"] = filtered
    if check_crc and any(zlib.crc32(b"IDAT" + c) != crc for c, crc in p["chunks"]):
        return D.E_CRC, None, info
    if st:
        return st, None, info
    st, samples = unfilter(filtered, W, H, p["color_type"], depth, lace)
    if st:
        return st, None, info
    return D.OK, D.convert(to8(samples, p["color_type"], depth, p["palette"]), mode, order), info
