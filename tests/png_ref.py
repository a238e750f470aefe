"""Plain numpy / Python restatement of the PNG encoder of attwarp_amd/csrc/png.hip.  Integer arithmetic
only; the kernels must produce the same bytes.

A file: signature, IHDR, ONE IDAT, IEND.  The zlib stream: 78 01, then per segment (whole rows, at most SEG_BYTES filtered
bytes and SEG_MAX_ROWS rows) either a dynamic-Huffman block followed by an empty stored block (which ends the segment on a
byte boundary) or one stored block, then 01 00 00 FF FF and the Adler-32 of the filtered bytes.  Matches have distance 1
only and never reach back over a segment's first byte."""
from __future__ import annotations

import struct

import numpy as np

SEG_BYTES = 24576
MAX_ROW_BYTES = 24576
SEG_MAX_ROWS = 1024
FILE_OVERHEAD = 68                    # everything of a file but its segments
FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
ADLER = 65521
POLY = 0xEDB88320
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 287 * 4

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


# ---- CRC-32 and Adler-32 with their combine steps ---------------------------------------------------------------------
def _crc_table():
    t = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ POLY if c & 1 else c >> 1
        t.append(c)
    return t


CRC_TABLE = _crc_table()


def crc32(data, crc=0):
    c = crc ^ 0xFFFFFFFF
    for b in bytes(data):
        c = CRC_TABLE[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def mulmod(a, b):
    """a * b mod the CRC polynomial, both in the reflected representation (bit 31 = x^0)."""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


def _pow_table():
    """x^(8 * 2^k) for k = 0 .. 31."""
    p = 0x40000000                    # x^1
    for _ in range(3):
        p = mulmod(p, p)              # x^8
    t = []
    for _ in range(32):
        t.append(p)
        p = mulmod(p, p)
    return t


CRC_POW8 = _pow_table()


def xpow8(nbytes):
    """x^(8 * nbytes)."""
    p = 0x80000000
    for k in range(32):
        if (nbytes >> k) & 1:
            p = mulmod(p, CRC_POW8[k])
    return p


def crc32_combine(crc1, crc2, len2):
    """crc32(A + B) from crc32(A), crc32(B) and len(B)."""
    return mulmod(crc1, xpow8(len2)) ^ crc2


def crc32_sliced(data, lanes=256):
    """What a workgroup computes: one table CRC per lane over equal slices, each shifted to the end, all XORed."""
    data = bytes(data)
    n = len(data)
    L = (n + lanes - 1) // lanes
    c = 0
    for t in range(lanes):
        lo, hi = min(n, t * L), min(n, (t + 1) * L)
        c ^= mulmod(crc32(data[lo:hi]), xpow8(n - hi))
    return c


def adler_partial(data):
    """(S1, S2, n) of a segment: S1 = sum d_i, S2 = sum (n - i) d_i, both mod 65521."""
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    n = d.size
    return int(d.sum() % ADLER), int((d * (n - np.arange(n))).sum() % ADLER), n


def adler_combine(parts):
    """Adler-32 of the concatenation: a = 1 + sum S1, b = N + sum S2 + sum S1 * (bytes after the segment)."""
    total = sum(p[2] for p in parts)
    a, b, before = 1, total % ADLER, 0
    for s1, s2, n in parts:
        after = total - before - n
        a = (a + s1) % ADLER
        b = (b + s2 + s1 * (after % ADLER)) % ADLER
        before += n
    return (b << 16) | a


# ---- filters ----------------------------------------------------------------------------------------------------------
def _as_hwc(image, order="rgb"):
    a = np.asarray(image)
    if a.ndim == 2:
        a = a[:, :, None]
    if order == "bgr" and a.shape[2] == 3:
        a = a[:, :, ::-1]
    return np.ascontiguousarray(a)


def filter_row(cur, prev, bpp, ftype):
    """One scanline (uint8 arrays) under filter 0 .. 4 -> filtered bytes."""
    cur = cur.astype(np.int32)
    up = prev.astype(np.int32)
    left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if cur.size > bpp else np.zeros_like(cur)
    ul = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]]) if cur.size > bpp else np.zeros_like(cur)
    if ftype == 0:
        pred = 0
    elif ftype == 1:
        pred = left
    elif ftype == 2:
        pred = up
    elif ftype == 3:
        pred = (left + up) >> 1
    else:
        p = left + up - ul
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    return ((cur - pred) & 255).astype(np.uint8)


def filtered_stream(image, filt="sub", order="rgb"):
    """The filtered scanline stream of an image as [H, 1 + W C] uint8."""
    a = _as_hwc(image, order)
    H, W, C = a.shape
    rows = a.reshape(H, W * C)
    out = np.zeros((H, 1 + W * C), np.uint8)
    zero = np.zeros(W * C, np.uint8)
    for r in range(H):
        prev = rows[r - 1] if r else zero
        if filt == "adaptive":
            best, bt = None, 0
            for t in range(5):
                f = filter_row(rows[r], prev, C, t)
                s = int(np.abs(f.view(np.int8).astype(np.int32)).sum())
                if best is None or s < best:
                    best, bt, bf = s, t, f
            out[r, 0], out[r, 1:] = bt, bf
        else:
            t = FILTERS[filt]
            out[r, 0], out[r, 1:] = t, filter_row(rows[r], prev, C, t)
    return out


# ---- segments, tokens, codes --------------------------------------------------------------------------------------------
def rows_per_segment(row_bytes):
    return max(1, min(SEG_MAX_ROWS, SEG_BYTES // row_bytes))


def segments(H, row_bytes):
    rps = rows_per_segment(row_bytes)
    return [(r0, min(rps, H - r0)) for r0 in range(0, H, rps)]


def bound(H, W, C):
    """Upper bound of a file's size: every segment stored."""
    rb = 1 + W * C
    return FILE_OVERHEAD + sum(n * rb + 5 for _, n in segments(H, rb))


def runs(data):
    """Maximal runs of equal bytes -> [(value, length)]."""
    d = np.frombuffer(bytes(data), np.uint8)
    starts = np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1]]))
    ends = np.concatenate([starts[1:], [d.size]])
    return [(int(d[s]), int(e - s)) for s, e in zip(starts, ends)]


def tokens(data):
    """[('lit', v) | ('len', n)]: the first byte of a run as a literal, then distance-1 matches of 258, then the rest as
    one match (3 .. 257) or as one or two literals."""
    out = []
    for v, n in runs(data):
        out.append(("lit", v))
        r = n - 1
        out += [("len", 258)] * (r // 258)
        rem = r % 258
        out += [("len", rem)] if rem >= 3 else [("lit", v)] * rem
    return out


def length_symbol(n):
    """match length 3 .. 258 -> (symbol, extra bits, extra value)."""
    for k in range(28, -1, -1):
        if n >= LEN_BASE[k]:
            return 257 + k, LEN_EXTRA[k], n - LEN_BASE[k]
    raise ValueError(n)


def histogram(toks):
    h = [0] * 286
    for kind, v in toks:
        h[v if kind == "lit" else length_symbol(v)[0]] += 1
    h[256] += 1
    return h


def huffman_depths(freq):
    """Depths of an (unlimited) Huffman tree over the symbols with freq > 0: leaves ordered by (frequency, symbol), two
    queues, a leaf before an internal node of the same weight.  At least two used symbols."""
    used = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    n = len(used)
    assert n >= 2
    parent = [0] * (2 * n - 1)
    node = []
    li = nj = 0

    def pick():
        nonlocal li, nj
        if li < n and (nj >= len(node) or used[li][0] <= node[nj]):
            li += 1
            return li - 1, used[li - 1][0]
        nj += 1
        return n + nj - 1, node[nj - 1]

    for k in range(n - 1):
        a, fa = pick()
        b, fb = pick()
        node.append(fa + fb)
        parent[a] = parent[b] = n + k
    depth = [0] * (2 * n - 1)
    for i in range(2 * n - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    lens = [0] * len(freq)
    for i, (_, s) in enumerate(used):
        lens[s] = depth[i]
    return lens


def code_lengths(hist, limit=15):
    """Code lengths of at most `limit` bits: while the tree is deeper, halve the frequencies (rounding up) and rebuild."""
    freq = list(hist)
    for _ in range(17):
        lens = huffman_depths(freq)
        if max(lens) <= limit:
            return lens
        freq = [(f + 1) >> 1 if f else 0 for f in freq]
    raise AssertionError("length limiter did not terminate")


def canonical_codes(lens):
    """RFC 1951 3.2.2 -> codes, already bit-reversed for the LSB-first bit writer."""
    codes = [0] * len(lens)
    nxt, code = {}, 0
    for bits in range(1, 16):
        code = (code + sum(1 for l in lens if l == bits - 1 and l)) << 1
        nxt[bits] = code
    for s, l in enumerate(lens):
        if l:
            c = nxt[l]
            nxt[l] += 1
            codes[s] = int(format(c, "0%db" % l)[::-1], 2)
    return codes


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits

    def to_bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _rev4(v):
    return ((v & 1) << 3) | ((v & 2) << 1) | ((v & 4) >> 1) | ((v & 8) >> 3)


def encode_segment(data):
    """One segment's filtered bytes -> its deflate bytes (byte aligned)."""
    data = bytes(data)
    n = len(data)
    toks = tokens(data)
    hist = histogram(toks)
    lens = code_lengths(hist)
    extra_bits = sum(hist[257 + k] * (LEN_EXTRA[k] + 1) for k in range(29))        # extra bits + the 1-bit distance
    dyn_bits = HEADER_BITS + sum(h * l for h, l in zip(hist, lens)) + extra_bits
    dyn_bytes = (dyn_bits + 3 + 7) // 8 + 4
    if dyn_bytes > n + 5:
        return b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + data
    codes = canonical_codes(lens)
    w = BitWriter()
    w.put(4, 3)                       # BFINAL = 0, BTYPE = 10
    w.put(29, 5)                      # HLIT = 286
    w.put(0, 5)                       # HDIST = 1
    w.put(15, 4)                      # HCLEN = 19
    for s in CL_ORDER:
        w.put(4 if s < 16 else 0, 3)  # a flat 4-bit code for 0 .. 15
    for l in lens + [1]:              # 286 literal / length lengths and one distance code of length 1
        w.put(_rev4(l), 4)
    assert w.n == HEADER_BITS
    for kind, v in toks:
        if kind == "lit":
            w.put(codes[v], lens[v])
        else:
            s, eb, ev = length_symbol(v)
            w.put(codes[s], lens[s])
            w.put(ev, eb)
            w.put(0, 1)               # the distance code
    w.put(codes[256], lens[256])
    assert w.n == dyn_bits
    w.put(0, 3)                       # empty stored block: BFINAL = 0, BTYPE = 00
    out = w.to_bytes() + b"\x00\x00\xff\xff"
    assert len(out) == dyn_bytes
    return out


# ---- the file ---------------------------------------------------------------------------------------------------------
def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", crc32(kind + payload))


def zlib_stream(filtered):
    """[H, row_bytes] filtered bytes -> (zlib stream, number of segments)."""
    H, rb = filtered.shape
    segs = segments(H, rb)
    parts, body = [], []
    for r0, nr in segs:
        d = filtered[r0:r0 + nr].tobytes()
        parts.append(adler_partial(d))
        body.append(encode_segment(d))
    z = b"\x78\x01" + b"".join(body) + b"\x01\x00\x00\xff\xff" + struct.pack(">I", adler_combine(parts))
    return z, len(segs)


def encode(image, filt="sub", order="rgb"):
    """uint8 [H,W] / [H,W,1] / [H,W,3] -> the PNG file's bytes."""
    a = _as_hwc(image, order)
    H, W, C = a.shape
    if C not in (1, 3) or H < 1 or W < 1:
        raise ValueError("png_ref: [H,W], [H,W,1] or [H,W,3] with H, W >= 1")
    if 1 + W * C > MAX_ROW_BYTES:
        raise ValueError("png_ref: row too long")
    z, _ = zlib_stream(filtered_stream(a, filt))
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 0 if C == 1 else 2, 0, 0, 0)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", z) + chunk(b"IEND", b"")
    assert len(out) <= bound(H, W, C)
    return out


def idat_payload(png):
    """The single IDAT chunk's payload of a file written by this encoder."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[12:16] == b"IHDR" and png[37:41] == b"IDAT"
    n = struct.unpack(">I", png[33:37])[0]
    assert len(png) == 41 + n + 4 + 12
    assert struct.unpack(">I", png[41 + n:45 + n])[0] == crc32(png[37:41 + n])
    return png[41:41 + n]
