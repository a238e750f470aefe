"""Plain Python / numpy restatement of the PNG decoder of attwarp_amd/csrc/pngdec.hip and pngdec_blocks.hpp (DESIGN.md
3.15): the chunk walk, the marker scan, the units, their chain and the dependent-unit rule, the status codes, the filters
and the three modes.  Integer arithmetic only; the kernels must give the same status and the same bytes."""
from __future__ import annotations

import struct
import zlib

import numpy as np

import png_ref as R

MAX_UNITS = 256
MAX_ROW_BYTES = 49152
(OK, E_CRC, E_ZLIB_HEADER, E_TRUNCATED, E_BLOCK_TYPE, E_STORED_LEN, E_CODE_LENGTHS, E_SYMBOL, E_DISTANCE, E_OVERFLOW,
 E_UNDERFLOW, E_ADLER, E_FILTER) = range(13)
STATUS_NAMES = ["OK", "E_CRC", "E_ZLIB_HEADER", "E_TRUNCATED", "E_BLOCK_TYPE", "E_STORED_LEN", "E_CODE_LENGTHS", "E_SYMBOL",
                "E_DISTANCE", "E_OVERFLOW", "E_UNDERFLOW", "E_ADLER", "E_FILTER"]
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
MARKER = b"\x00\x00\xff\xff"


# ---- the host's part: chunks ----------------------------------------------------------------------------------------------
def parse(data):
    """File bytes -> dict(W, H, color_type, chunks=[(payload, stated crc)], stream).  ValueError names the field."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise ValueError("signature")
    pos, ihdr, chunks, seen_iend, idat_done = 8, None, [], False, False
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
        pos += 12 + n
    if ihdr is None:
        raise ValueError("IHDR: missing")
    if not seen_iend:
        raise ValueError("IEND: missing")
    W, H, depth, ctype, comp, filt, lace = ihdr
    if depth != 8:
        raise ValueError("bit depth")
    if ctype not in CHANNELS:
        raise ValueError("colour type")
    if comp != 0 or filt != 0:
        raise ValueError("compression / filter method")
    if lace != 0:
        raise ValueError("interlace")
    if W == 0 or H == 0:
        raise ValueError("size")
    if 1 + W * CHANNELS[ctype] > MAX_ROW_BYTES or H * (1 + W * CHANNELS[ctype]) >= 1 << 31:
        raise ValueError("size limit")
    return dict(W=W, H=H, color_type=ctype, chunks=chunks, stream=b"".join(c[0] for c in chunks))


# ---- inflate ------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, s, at):
        self.s, self.n, self.pos, self.cnt, self.acc = s, len(s), min(at, len(s)), 0, 0

    def refill(self):
        if self.cnt > 32:
            return
        take = min(8, self.n - self.pos)
        if take > 0:
            self.acc |= int.from_bytes(self.s[self.pos:self.pos + take], "little") << self.cnt
            self.pos += take
            self.cnt += 8 * take

    def bits(self, nb):
        self.refill()
        if nb > self.cnt:
            return None
        v = self.acc & ((1 << nb) - 1)
        self.acc >>= nb
        self.cnt -= nb
        return v

    def byte_pos(self):
        return self.pos - self.cnt // 8

    def to_byte(self, at):
        self.pos, self.cnt, self.acc = at, 0, 0


def _rev(c, l):
    return int(format(c, "0%db" % l)[::-1], 2)


def build(lens, allow_single):
    """Code lengths -> table over the next 15 bits (LSB first): (symbol, length) or None; None for a refused set."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    left, maxl = 1, 0
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            return None
        if count[l]:
            maxl = l
    if left > 0 and not (allow_single and maxl <= 1):
        return None
    tab = [None] * (1 << 15)
    code = 0
    for l in range(1, 16):
        for sym, sl in enumerate(lens):
            if sl == l:
                r = _rev(code, l)
                tab[r::1 << l] = [(sym, l)] * (1 << (15 - l))
                code += 1
        code <<= 1
    return tab


def _decode(br, tab, used=None):
    br.refill()
    e = tab[br.acc & 0x7FFF]
    if e is None:
        return E_SYMBOL, 0
    sym, l = e
    if l > br.cnt:
        return E_TRUNCATED, 0
    br.acc >>= l
    br.cnt -= l
    if used is not None:
        used.add(l)
    return OK, sym


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False), build([5] * 32, False))
    return _FIXED


class Result:
    def __init__(self, start):
        self.status, self.start, self.end, self.out, self.final, self.dependent = OK, start, start, bytearray(), 0, 0
        self.seen = set()             # (length, distance) of every match: the tests' token walk
        self.lit_lens, self.dist_lens = set(), set()   # code lengths of the literals and length symbols / distances decoded

    @property
    def out_len(self):
        return len(self.out)


def inflate(s, start, cap, kept=None, write=True):
    """pd_inflate: whole blocks from byte `start` until the final block or, with `kept`, until behind an empty stored block
    on a kept position.  write=False counts: a match reaching back before the first byte sets `dependent` (zeros stand in
    for its bytes); write=True makes it E_DISTANCE."""
    R_ = Result(start)
    br = _Bits(s, start)
    out = R_.out
    n = len(s)

    def fail(code):
        R_.status, R_.end = code, br.byte_pos()
        return R_

    while True:
        hdr = br.bits(3)
        if hdr is None:
            return fail(E_TRUNCATED)
        bfinal, btype = hdr & 1, hdr >> 1
        if btype == 3:
            return fail(E_BLOCK_TYPE)
        if btype == 0:
            at = br.byte_pos()
            if at + 4 > n:
                br.to_byte(n)
                return fail(E_TRUNCATED)
            ln, nln = struct.unpack("<HH", s[at:at + 4])
            at += 4
            br.to_byte(at)
            if ln ^ nln != 0xFFFF:
                return fail(E_STORED_LEN)
            if ln > n - at:
                br.to_byte(n)
                return fail(E_TRUNCATED)
            if ln > cap - len(out):
                return fail(E_OVERFLOW)
            out += s[at:at + ln]
            at += ln
            br.to_byte(at)
            if not bfinal and ln == 0 and kept is not None and at in kept and at > start:
                R_.end = at
                return R_
        else:
            if btype == 1:
                lit, dist = _fixed()
            else:
                v = br.bits(14)
                if v is None:
                    return fail(E_TRUNCATED)
                nlen, ndist, ncode = 257 + (v & 31), 1 + ((v >> 5) & 31), 4 + (v >> 10)
                if nlen > 286 or ndist > 30:
                    return fail(E_CODE_LENGTHS)
                cl = [0] * 19
                for i in range(ncode):
                    v = br.bits(3)
                    if v is None:
                        return fail(E_TRUNCATED)
                    cl[R.CL_ORDER[i]] = v
                ctab = build(cl, False)
                if ctab is None:
                    return fail(E_CODE_LENGTHS)
                lens = []
                total = nlen + ndist
                while len(lens) < total:
                    rc, sym = _decode(br, ctab)
                    if rc:
                        return fail(E_CODE_LENGTHS if rc == E_SYMBOL else rc)
                    if sym < 16:
                        lens.append(sym)
                        continue
                    val = 0
                    if sym == 16:
                        if not lens:
                            return fail(E_CODE_LENGTHS)
                        val, nb, base = lens[-1], 2, 3
                    elif sym == 17:
                        nb, base = 3, 3
                    else:
                        nb, base = 7, 11
                    v = br.bits(nb)
                    if v is None:
                        return fail(E_TRUNCATED)
                    if len(lens) + base + v > total:
                        return fail(E_CODE_LENGTHS)
                    lens += [val] * (base + v)
                if lens[256] == 0:
                    return fail(E_CODE_LENGTHS)
                dist = build(lens[nlen:], True)
                if dist is None:
                    return fail(E_CODE_LENGTHS)
                lit = build(lens[:nlen], True)
                if lit is None:
                    return fail(E_CODE_LENGTHS)
            while True:
                eob = set()
                rc, sym = _decode(br, lit, eob)
                if rc:
                    return fail(rc)
                if sym != 256:
                    R_.lit_lens |= eob
                if sym < 256:
                    if len(out) >= cap:
                        return fail(E_OVERFLOW)
                    out.append(sym)
                    continue
                if sym == 256:
                    break
                sym -= 257
                if sym >= 29:
                    return fail(E_SYMBOL)
                v = br.bits(R.LEN_EXTRA[sym])
                if v is None:
                    return fail(E_TRUNCATED)
                ln = R.LEN_BASE[sym] + v
                rc, sym = _decode(br, dist, R_.dist_lens)
                if rc:
                    return fail(rc)
                if sym >= 30:
                    return fail(E_SYMBOL)
                v = br.bits(DIST_EXTRA[sym])
                if v is None:
                    return fail(E_TRUNCATED)
                d = DIST_BASE[sym] + v
                R_.seen.add((ln, d))
                if d > len(out):
                    if write:
                        return fail(E_DISTANCE)
                    R_.dependent = 1
                    if ln > cap - len(out):
                        return fail(E_OVERFLOW)
                    out += bytes(ln)
                    continue
                if ln > cap - len(out):
                    return fail(E_OVERFLOW)
                if d >= ln:
                    out += out[len(out) - d:len(out) - d + ln]
                else:
                    seg = bytes(out[len(out) - d:])
                    out += (seg * (ln // d + 1))[:ln]
        if bfinal:
            R_.final, R_.end = 1, br.byte_pos()
            return R_


def zlib_header(s):
    if len(s) < 2:
        return E_TRUNCATED
    cmf, flg = s[0], s[1]
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or (cmf * 256 + flg) % 31 or (flg & 32):
        return E_ZLIB_HEADER
    return OK


def find_markers(s):
    """The kept unit starts: 2, then the first MAX_UNITS - 1 positions p < len(s) with s[p - 4:p] == 00 00 FF FF, p >= 6."""
    kept, i = [2], s.find(MARKER, 2)
    while i >= 0 and len(kept) < MAX_UNITS:
        if i + 4 < len(s):
            kept.append(i + 4)
        i = s.find(MARKER, i + 1)
    return kept


def adler32(data):
    return R.adler_combine([R.adler_partial(data)]) if len(data) else 1


def decode_stream(s, filt_bytes, force_serial=False):
    """zlib stream -> (status, filtered bytes or None, info).  info: route "unit" / "serial" / None, nunits (kept
    positions), chain (units on the chain, unit route only)."""
    s = bytes(s)
    info = dict(route=None, nunits=0, chain=0, adler=1)
    st = zlib_header(s)
    if st:
        return st, None, info
    kept = find_markers(s)
    info["nunits"] = len(kept)
    filtered, adler_pos = None, 0
    if len(kept) > 1 and not force_serial:
        keptset = set(kept)
        units = [inflate(s, p, filt_bytes, keptset, write=False) for p in kept]
        u, total, parts, ok = 0, 0, [], False
        for _ in range(len(units)):
            U = units[u]
            if U.status or U.dependent or U.out_len > filt_bytes - total:
                break
            parts.append(U.out)
            total += U.out_len
            if U.final:
                adler_pos = U.end
                ok = total == filt_bytes and len(s) - U.end >= 4
                break
            nxt = [v for v in range(u + 1, len(units)) if kept[v] == U.end]
            if not nxt:
                break
            u = nxt[0]
        if ok:
            info["route"], info["chain"] = "unit", len(parts)
            filtered = b"".join(bytes(p) for p in parts)
    if filtered is None:
        info["route"] = "serial"
        r = inflate(s, 2, filt_bytes, None, write=True)
        info["adler"] = adler32(bytes(r.out))
        if r.status:
            return r.status, None, info
        if r.out_len < filt_bytes:
            return E_UNDERFLOW, None, info
        if len(s) - r.end < 4:
            return E_TRUNCATED, None, info
        filtered, adler_pos = bytes(r.out), r.end
    info["adler"] = adler32(filtered)
    if struct.unpack(">I", s[adler_pos:adler_pos + 4])[0] != info["adler"]:
        return E_ADLER, None, info
    return OK, filtered, info


# ---- filters and pixels -------------------------------------------------------------------------------------------------------
def unfilter(filtered, H, W, ch):
    """Filtered bytes -> (status, [H, W, ch] uint8).  The device stops before the 64-row batch that holds a bad filter byte;
    only the status is defined then."""
    f = np.frombuffer(filtered, np.uint8).reshape(H, 1 + W * ch)
    if (f[:, 0] > 4).any():
        return E_FILTER, None
    out = np.zeros((H, W * ch), np.uint8)
    prev = np.zeros(W * ch, np.int32)
    for r in range(H):
        ft, row = int(f[r, 0]), f[r, 1:].astype(np.int32)
        if ft == 0:
            cur = row
        elif ft == 2:
            cur = (row + prev) & 255
        elif ft == 1:
            cur = (np.cumsum(row.reshape(W, ch), 0) & 255).reshape(-1)
        else:
            cur = np.zeros(W * ch, np.int32)
            rl, pl = row.tolist(), prev.tolist()
            cl = [0] * (W * ch)
            for i in range(W * ch):
                a = cl[i - ch] if i >= ch else 0
                b = pl[i]
                c = pl[i - ch] if i >= ch else 0
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cl[i] = (rl[i] + pred) & 255
            cur = np.array(cl, np.int32)
        out[r] = cur
        prev = cur
    return OK, out.reshape(H, W, ch)


def luma(rgb):
    a = rgb.astype(np.uint32)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 32768) >> 16).astype(np.uint8)


def out_channels(ch, mode):
    return 1 if mode == "L" else 3 if mode == "RGB" else (1 if ch <= 2 else 3)


def convert(px, mode="RGB", order="rgb"):
    """[H, W, ch] of the file -> [H, W, C] of the mode: grey replicated, alpha dropped, Pillow's integer luma."""
    ch = px.shape[2]
    oc = out_channels(ch, mode)
    if ch <= 2:
        g = px[:, :, :1]
        return np.ascontiguousarray(np.repeat(g, oc, 2))
    rgb = px[:, :, :3]
    if oc == 1:
        return luma(rgb)[:, :, None]
    return np.ascontiguousarray(rgb[:, :, ::-1] if order == "bgr" else rgb)


def decode(data, mode="RGB", order="rgb", check_crc=True, force_serial=False):
    """File bytes -> (status, image or None, info); ValueError for what the host refuses."""
    p = parse(data)
    ch = CHANNELS[p["color_type"]]
    H, W = p["H"], p["W"]
    st, filtered, info = decode_stream(p["stream"], H * (1 + W * ch), force_serial)
    if check_crc and any(zlib.crc32(b"IDAT" + c) != crc for c, crc in p["chunks"]):
        return E_CRC, None, info
    if st:
        return st, None, info
    st, px = unfilter(filtered, H, W, ch)
    if st:
        return st, None, info
    return OK, convert(px, mode, order), info
