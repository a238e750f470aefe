"""numpy restatement of the JPEG decoder (attwarp_amd/csrc/jpegdec.hip, jpegdec_blocks.hpp): the marker
walk, the restart-marker scan, the entropy decode with its statuses, dequantisation, the integer IDCT, "fancy" chroma
up-sampling and YCbCr -> RGB.  Pinned to Pillow by tests/test_jpegdec_ref_cpu.py; the kernels and the host program of the
shared core are compared with it.  All pixel arithmetic is int32 with wrap-around, as the kernels define it."""
from __future__ import annotations

import struct
import zlib

import numpy as np

OK, E_TRUNCATED, E_HUFFMAN, E_COEFF, E_RESTART, E_NO_EOI = range(6)
STATUS_NAMES = ["OK", "E_TRUNCATED", "E_HUFFMAN", "E_COEFF", "E_RESTART", "E_NO_EOI"]
MAX_UNITS = 65536
MAX_BLOCKS = 1 << 24

# zigzag position -> natural (row-major) position
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

_FRAMES = {0xC2: "progressive", 0xC3: "lossless", 0xC5: "hierarchical", 0xC6: "hierarchical", 0xC7: "hierarchical",
           0xC9: "arithmetic", 0xCA: "arithmetic", 0xCB: "arithmetic", 0xCD: "arithmetic", 0xCE: "arithmetic", 0xCF: "arithmetic"}


def parse(data):
    """The marker walk: bytes -> dict(W, H, ncomp, hs, vs, ri, qt [ncomp][64] natural order, dc / ac [(counts, symbols)] per
    component, stream = everything behind the SOS header).  ValueError for what is not decoded, OSError for a file that ends
    inside its headers."""
    d = bytes(data)
    n = len(d)

    def need(a, b):
        if b > n:
            raise OSError("jpeg: the file ends inside its headers")
        return d[a:b]

    if need(0, 2) != b"\xff\xd8":
        raise ValueError("jpeg: bad signature")
    pos = 2
    qts, dcs, acs = {}, {}, {}
    frame, ri, jfif, adobe = None, 0, False, None
    while True:
        if need(pos, pos + 1) != b"\xff":
            raise ValueError("jpeg: a marker was expected")
        while need(pos, pos + 1) == b"\xff":
            pos += 1
        m = d[pos]
        pos += 1
        if m in _FRAMES:
            raise ValueError(f"jpeg: {_FRAMES[m]} frame")
        if m == 0xCC:
            raise ValueError("jpeg: arithmetic conditioning")
        if m == 0xD9 or m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01 or m == 0x00:
            raise ValueError(f"jpeg: marker {m:02x} in the headers")
        L = struct.unpack(">H", need(pos, pos + 2))[0]
        if L < 2:
            raise ValueError("jpeg: segment length below 2")
        seg = need(pos + 2, pos + L)
        pos += L
        if m in (0xC0, 0xC1):
            if frame is not None:
                raise ValueError("jpeg: a second frame (hierarchical)")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise ValueError("jpeg: bad frame header")
            prec, H, W, nf = struct.unpack(">BHHB", seg[:6])
            if prec != 8:
                raise ValueError(f"jpeg: precision {prec} (8 only)")
            if H == 0 or W == 0:
                raise ValueError(f"jpeg: size {W} x {H}")
            if nf not in (1, 3):
                raise ValueError(f"jpeg: {nf} components (1 or 3)")
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)]
            frame = (W, H, comps)
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise ValueError("jpeg: DHT runs past its segment")
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                ns = sum(counts)
                if tc > 1 or th > 3:
                    raise ValueError("jpeg: DHT class / id")
                left = 1
                for c in counts:
                    left = 2 * left - c
                    if left < 0:
                        raise ValueError("jpeg: DHT over-subscribed")
                if ns > 256 or q + 17 + ns > len(seg):
                    raise ValueError("jpeg: DHT symbols exceed 256 or run past the segment")
                syms = list(seg[q + 17:q + 17 + ns])
                if tc == 0 and any(s > 15 for s in syms):
                    raise ValueError("jpeg: DHT with a DC category above 15")
                (acs if tc else dcs)[th] = (counts, syms)
                q += 17 + ns
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq == 1:
                    raise ValueError("jpeg: 16-bit quantisation table")
                if pq > 1 or tq > 3 or q + 65 > len(seg):
                    raise ValueError("jpeg: bad DQT")
                t = [0] * 64
                for k in range(64):
                    t[ZIGZAG[k]] = seg[q + 1 + k]
                qts[tq] = t
                q += 65
        elif m == 0xDD:
            if len(seg) != 2:
                raise ValueError("jpeg: bad DRI")
            ri = struct.unpack(">H", seg)[0]
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\0"
        elif m == 0xEE:
            if seg[:5] == b"Adobe" and len(seg) >= 12:
                adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise ValueError("jpeg: SOS before the frame header")
            W, H, comps = frame
            nf = len(comps)
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise ValueError("jpeg: bad scan header")
            if seg[0] != nf or [seg[1 + 2 * i] for i in range(nf)] != [c[0] for c in comps]:
                raise ValueError("jpeg: the scan does not hold all components in frame order (more than one scan)")
            if tuple(seg[1 + 2 * nf:]) != (0, 63, 0):
                raise ValueError("jpeg: spectral selection / successive approximation")
            if nf == 3:
                if (adobe == 0) or (adobe is None and not jfif and bytes(c[0] for c in comps) == b"RGB"):
                    raise ValueError("jpeg: RGB-coded file")
                samp = [(c[1], c[2]) for c in comps]
                if samp[1] != (1, 1) or samp[2] != (1, 1) or samp[0] not in ((1, 1), (2, 1), (2, 2)):
                    raise ValueError(f"jpeg: sampling layout {samp}")
                hs, vs = samp[0]
            else:
                hs = vs = 1
            qt, dc, ac = [], [], []
            for i, c in enumerate(comps):
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if c[3] not in qts or td not in dcs or ta not in acs:
                    raise ValueError("jpeg: the scan names a table never defined")
                qt.append(qts[c[3]]); dc.append(dcs[td]); ac.append(acs[ta])
            stream = d[pos:]
            break
        elif m in (0xDC, 0xDE, 0xDF):
            raise ValueError("jpeg: DNL / hierarchical marker")
    p = dict(W=W, H=H, ncomp=nf, hs=hs, vs=vs, ri=ri, qt=qt, dc=dc, ac=ac, stream=stream)
    g = geometry(p)
    if g["nunits"] > MAX_UNITS or g["nblocks"] >= MAX_BLOCKS or len(stream) >= 1 << 31:
        raise ValueError("jpeg: size limit")
    return p


def geometry(p):
    hs, vs = p["hs"], p["vs"]
    mcux, mcuy = -(-p["W"] // (8 * hs)), -(-p["H"] // (8 * vs))
    nmcu = mcux * mcuy
    samp = [(hs, vs)] + [(1, 1)] * (p["ncomp"] - 1)
    bw = [mcux * h for h, _ in samp]
    bh = [mcuy * v for _, v in samp]
    nunits = -(-nmcu // p["ri"]) if p["ri"] else 1
    return dict(mcux=mcux, mcuy=mcuy, nmcu=nmcu, samp=samp, bw=bw, bh=bh, nunits=nunits, nblocks=sum(a * b for a, b in zip(bw, bh)))


def scan(s, nunits):
    """The restart-marker scan -> (status, [(start, end)] per unit, EOI seen).  The data ends at the first FF that is followed
    by neither 00 nor D0..D7 (or by nothing); restart markers behind that are not looked at."""
    n = len(s)
    rst, term = [], n
    i = 0
    while i < n:
        if s[i] == 0xFF:
            nx = s[i + 1] if i + 1 < n else None
            if nx == 0:
                i += 2
                continue
            if nx is not None and 0xD0 <= nx <= 0xD7:
                rst.append((i, nx & 7))
                i += 2
                continue
            term = i
            break
        i += 1
    q = term
    while q < n and s[q] == 0xFF:
        q += 1
    eoi = q > term and q < n and s[q] == 0xD9
    if len(rst) != nunits - 1 or any(ix != (k & 7) for k, (_, ix) in enumerate(rst)):
        return E_RESTART, [], eoi
    starts = [0] + [p + 2 for p, _ in rst]
    ends = [p for p, _ in rst] + [term]
    return OK, list(zip(starts, ends)), eoi


def code_table(counts, symbols):
    """{(length, code): symbol} of a canonical code."""
    t, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            t[(l, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return t


class _Bits:
    def __init__(self, unit):
        out = bytearray()
        i, n = 0, len(unit)
        while i < n:
            out.append(unit[i])
            i += 2 if unit[i] == 0xFF else 1          # (inside a unit every FF is followed by 00)
        self.bits = np.unpackbits(np.frombuffer(bytes(out), np.uint8)).tolist()
        self.n = len(self.bits)
        self.pos = 0

    def symbol(self, table):
        code = 0
        for l in range(1, 17):
            at = self.pos + l - 1
            code = code << 1 | (self.bits[at] if at < self.n else 0)
            if (l, code) in table:
                if self.pos + l > self.n:
                    return E_TRUNCATED, 0
                self.pos += l
                SEEN["long"] += l > 8
                return OK, table[(l, code)]
        return (E_TRUNCATED if self.pos + 16 > self.n else E_HUFFMAN), 0

    def value(self, s):
        if self.pos + s > self.n:
            return E_TRUNCATED, 0
        v = 0
        for b in self.bits[self.pos:self.pos + s]:
            v = v << 1 | b
        self.pos += s
        return OK, v


def extend(v, s):
    return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1


def _wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


SEEN = {"zrl": 0, "long": 0}                       # ZRL symbols and codes above 8 bits decoded so far (for the corpus tests)


def decode_block(bits, dc, ac, pred, blk):
    """One block into blk (64 int16, natural order, zero on entry) -> (status, new predictor).  The predictor is a 32-bit
    two's-complement sum; the DC coefficient stored is its low 16 bits."""
    st, s = bits.symbol(dc)
    if st:
        return st, pred
    st, v = bits.value(s)
    if st:
        return st, pred
    pred = _wrap32(pred + extend(v, s))
    blk[0] = _wrap16(pred)
    k = 1
    while k < 64:
        st, rs = bits.symbol(ac)
        if st:
            return st, pred
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            if k + 16 > 64:
                return E_COEFF, pred
            SEEN["zrl"] += 1
            k += 16
            continue
        k += r
        if k > 63:
            return E_COEFF, pred
        st, v = bits.value(s)
        if st:
            return st, pred
        blk[ZIGZAG[k]] = extend(v, s)
        k += 1
    return OK, pred


def entropy(p, want_rs=None):
    """-> (status, [coefficient planes int16 [bh, bw, 64]] per component, info)."""
    g = geometry(p)
    s = p["stream"]
    st, units, eoi = scan(s, g["nunits"])
    planes = [np.zeros((g["bh"][c], g["bw"][c], 64), np.int16) for c in range(p["ncomp"])]
    info = dict(nunits=g["nunits"], eoi=eoi, units=units)
    if st:
        return st, planes, info
    dct = [code_table(*t) for t in p["dc"]]
    act = [code_table(*t) for t in p["ac"]]
    ri = p["ri"] or g["nmcu"]
    first = OK
    for k, (a, b) in enumerate(units):
        bits = _Bits(s[a:b])
        pred = [0] * p["ncomp"]
        ust = OK
        for m in range(k * ri, min((k + 1) * ri, g["nmcu"])):
            mx, my = m % g["mcux"], m // g["mcux"]
            for c, (h, v) in enumerate(g["samp"]):
                for yy in range(v):
                    for xx in range(h):
                        blk = planes[c][my * v + yy, mx * h + xx]
                        ust, pred[c] = decode_block(bits, dct[c], act[c], pred[c], blk)
                        if ust:
                            break
                    if ust:
                        break
                if ust:
                    break
            if ust:
                break
        if ust and not first:
            first = ust                               # the lowest failing unit's status
    if first:
        return first, planes, info
    return (OK if eoi else E_NO_EOI), planes, info


def coef_crc(planes):
    """CRC-32 of the coefficients as the device lays them out: component after component, blocks row-major, int16 LE."""
    c = 0
    for pl in planes:
        c = zlib.crc32(pl.astype("<i2").tobytes(), c)
    return c


def _pass(i, shift):
    """One IDCT pass along axis 0 of i [8, ...] int32 (wrapping), Appendix A."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (i[k] for k in range(8))
    I = np.int32
    z1 = (i2 + i6) * I(4433)
    t2 = z1 - i6 * I(15137)
    t3 = z1 + i2 * I(6270)
    t0 = (i0 + i4) * I(8192)
    t1 = (i0 - i4) * I(8192)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = i7, i5, i3, i1
    z5 = (a + c + b + d) * I(9633)
    z1 = (a + d) * I(-7373)
    z2 = (b + c) * I(-20995)
    z3 = (a + c) * I(-16069) + z5
    z4 = (b + d) * I(-3196) + z5
    a = a * I(2446) + z1 + z3
    b = b * I(16819) + z2 + z4
    c = c * I(25172) + z2 + z3
    d = d * I(12299) + z1 + z4
    rnd = I(1 << (shift - 1))
    o = [t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d]
    return np.stack([(x + rnd) >> I(shift) for x in o])


def idct_planes(p, planes):
    """Coefficient planes -> uint8 component planes padded to whole blocks."""
    out = []
    with np.errstate(over="ignore"):
        for c, pl in enumerate(planes):
            bh, bw, _ = pl.shape
            q = np.asarray(p["qt"][c], np.int32)
            x = (pl.astype(np.int32) * q).reshape(bh, bw, 8, 8)          # [.., row, col]
            x = _pass(np.moveaxis(x, 2, 0), 11)                          # columns: along the row index
            x = np.moveaxis(x, 0, 2)
            x = _pass(np.moveaxis(x, 3, 0), 18)                          # rows: along the column index
            x = np.moveaxis(x, 0, 3)
            x = np.clip(x + np.int32(128), 0, 255).astype(np.uint8)
            out.append(x.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def upsample(pl, hs, vs, W, H):
    """"Fancy" up-sampling of a chroma plane (already cropped to its true size) by hs x vs, cropped to W x H.  A plane of
    one or two columns is replicated instead: jdsample.c takes the triangle filter only when downsampled_width > 2."""
    p = pl.astype(np.int32)
    dh, dw = p.shape
    if hs == 1 and vs == 1:
        return p[:H, :W]
    if dw <= 2:
        return np.repeat(np.repeat(p, vs, 0), hs, 1)[:H, :W]
    if vs == 2:
        up = np.concatenate([p[:1], p[:-1]])
        dn = np.concatenate([p[1:], p[-1:]])
        s = np.empty((2 * dh, dw), np.int32)
        s[0::2] = 3 * p + up
        s[1::2] = 3 * p + dn
        lf = np.concatenate([s[:, :1], s[:, :-1]], 1)
        rt = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        o = np.empty((2 * dh, 2 * dw), np.int32)
        o[:, 0::2] = (3 * s + lf + 8) >> 4
        o[:, 1::2] = (3 * s + rt + 7) >> 4
        return o[:H, :W]
    lf = np.concatenate([p[:, :1], p[:, :-1]], 1)
    rt = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    o = np.empty((dh, 2 * dw), np.int32)
    o[:, 0::2] = (3 * p + lf + 1) >> 2
    o[:, 1::2] = (3 * p + rt + 2) >> 2
    o[:, 0] = p[:, 0]
    o[:, -1] = p[:, -1]
    return o[:H, :W]


def luma(rgb):
    r, g, b = (rgb[..., k].astype(np.uint32) for k in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).astype(np.uint8)


def pixels(p, comp, mode="RGB", order="rgb"):
    W, H, hs, vs = p["W"], p["H"], p["hs"], p["vs"]
    y = comp[0][:H, :W]
    if p["ncomp"] == 1:
        return np.repeat(y[:, :, None], 3, 2) if mode == "RGB" else y[:, :, None].copy()
    dw, dh = -(-W // hs), -(-H // vs)
    cb = upsample(comp[1][:dh, :dw], hs, vs, W, H) - 128
    cr = upsample(comp[2][:dh, :dw], hs, vs, W, H) - 128
    yy = y.astype(np.int32)
    r = yy + ((91881 * cr + 32768) >> 16)
    g = yy + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = yy + ((116130 * cb + 32768) >> 16)
    rgb = np.clip(np.stack([r, g, b], 2), 0, 255).astype(np.uint8)
    if mode == "L":
        return luma(rgb)[:, :, None]
    return rgb[:, :, ::-1].copy() if order == "bgr" else rgb


_CACHE = {}


def decode(f, mode="RGB", order="rgb"):
    """A file -> (status, pixels [H, W, C] or None, info).  info: nunits, crc (of the coefficients; 0 unless OK), eoi."""
    key = bytes(f)
    if key not in _CACHE:
        p = parse(key)
        st, planes, info = entropy(p)
        info = dict(info, crc=coef_crc(planes) if st == OK else 0)
        _CACHE[key] = (p, st, idct_planes(p, planes) if st == OK else None, info)
    p, st, comp, info = _CACHE[key]
    if st:
        return st, None, info
    return st, pixels(p, comp, mode, order), info
