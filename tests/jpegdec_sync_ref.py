"""Restatement of the JPEG decoder's self-synchronising sub-streams (attwarp_amd/csrc/jpegdec_blocks.hpp: jd_decode_segment,
jd_segment_check, jd_write_segment; jpegdec_substream_kernel) in the raw-byte domain, Jacobi rounds.

A marker-less unit is cut into segments of ``segment_bytes`` raw bytes.  A decoder's state between two symbols is
``(byte, bit, slot, k)``: the raw offset of the byte that holds the next bit (never a stuffed 00; the unit's end when no bit
is left), the bit's index in it, the block's slot within the MCU and the zigzag index of the next coefficient (0: a DC symbol
is next).  Segment 0 enters at (0, 0, 0, 0); every other segment first guesses that a block starts at its first byte.  A
round decodes every segment whose entry changed, then hands every exit to the next segment as its entry; the rounds end when
no entry changes.  After round r the entries of segments 0..r are the sequential decoder's, so a fixed point is the
sequential decode."""
from __future__ import annotations

import functools

import numpy as np

import jpegdec_ref as D

NO_ERROR = 0xFFFFFFFF
MAX_SEGMENTS = 1 << 14                                     # longer images are decoded sequentially
DEFAULT_SEGMENT_BYTES, DEFAULT_MAX_ROUNDS = 256, 64


def planned_segments(p, segment_bytes):
    """Segments planned for a parsed file from its headers and length alone; 0: decoded sequentially."""
    n = len(p["stream"])
    nseg = -(-n // segment_bytes)
    if D.geometry(p)["nunits"] != 1 or n < 2 * segment_bytes or nseg > MAX_SEGMENTS:
        return 0
    return nseg


def _lookup(counts, symbols):
    """By the next 16 bits: (length, symbol) lists; length 0: no code."""
    ln, sy = [0] * 65536, [0] * 65536
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            a, b = code << (16 - l), (code + 1) << (16 - l)
            ln[a:b] = [l] * (b - a)
            sy[a:b] = [symbols[k]] * (b - a)
            code += 1
            k += 1
        code <<= 1
    return ln, sy


class Unit:
    """The unit's bits with the raw offset of every data byte."""

    def __init__(self, s, uend):
        data, raw = bytearray(), []
        i = 0
        while i < uend:
            data.append(s[i])
            raw.append(i)
            i += 2 if s[i] == 0xFF else 1                  # (inside a unit every FF is followed by 00)
        self.raw, self.uend, self.n = raw, uend, 8 * len(data)
        self.index = {r: i for i, r in enumerate(raw)}
        self.index[uend] = len(data)
        self.data = bytes(data) + b"\0\0\0\0"

    def to_bit(self, byte, bit):
        return 8 * self.index[min(byte, self.uend)] + bit

    def to_pos(self, u):
        return (self.raw[u >> 3], u & 7) if u < self.n else (self.uend, 0)

    def window(self, u):
        """The 24 bits from u on, zeros behind the end."""
        i = u >> 3
        return (int.from_bytes(self.data[i:i + 4], "big") >> (8 - (u & 7))) & 0xFFFFFF

    def symbol(self, tab, u):
        ln, sy = tab
        c = self.window(u) >> 8
        l = ln[c]
        if l == 0:
            return (D.E_TRUNCATED if self.n - u < 16 else D.E_HUFFMAN), 0, u
        if l > self.n - u:
            return D.E_TRUNCATED, 0, u
        return D.OK, sy[c], u + l

    def value(self, s, u):
        if s > self.n - u:
            return D.E_TRUNCATED, 0, u
        return D.OK, (self.window(u) >> (24 - s)) if s else 0, u + s


def guess(s, seg, segment_bytes, uend):
    b = seg * segment_bytes
    if b >= uend:
        b = uend
    elif b > 0 and s[b] == 0 and s[b - 1] == 0xFF:
        b += 1
    return (b, 0, 0, 0)


def decode_segment(un, entry, seg_end, dct, act, nb0, nblk):
    """-> dict(exit, owned, nend, eclean, dc)."""
    byte, bit, slot, k = entry
    u = un.to_bit(byte, bit)
    owned = nend = 0
    eclean = NO_ERROR
    dc = [0, 0, 0]
    at_end = False
    while un.to_pos(u)[0] < seg_end:
        c = 0 if slot < nb0 else slot - nb0 + 1
        endblk = False
        if k == 0:
            st, s, u = un.symbol(dct[c], u)
            s &= 15
            if not st:
                st, v, u = un.value(s, u)
            if not st:
                owned += 1
                dc[c] = (dc[c] + D.extend(v, s)) & 0xFFFFFFFF
                k = 1
        else:
            st, rs, u = un.symbol(act[c], u)
            if not st:
                run, s = rs >> 4, rs & 15
                if s == 0:
                    if run != 15:
                        endblk = True
                    elif k + 16 > 64:
                        st = D.E_COEFF
                    else:
                        k += 16
                elif k + run > 63:
                    st = D.E_COEFF
                else:
                    st, v, u = un.value(s, u)
                    if not st:
                        k += run + 1
            if not st and k >= 64:
                endblk = True
        if st:
            if eclean == NO_ERROR:
                eclean = nend
            if st == D.E_TRUNCATED or u >= un.n:
                at_end = True
                break
            u += 1
            slot, k = (slot + 1) % nblk, 0
        elif endblk:
            nend += 1
            slot, k = (slot + 1) % nblk, 0
    pos = (un.uend, 0) if at_end else un.to_pos(u)
    return dict(exit=(pos[0], pos[1], slot, k), owned=owned, nend=nend, eclean=eclean, dc=dc)


def check(entry, r, before, expected, nblk):
    inprog = int(entry[3] != 0)
    if before < inprog:
        return 1
    done = before - inprog
    if done >= expected:
        return 0
    if entry[2] != done % nblk:
        return 1
    last = expected - 1 - done
    if last < r["nend"]:
        return 2 if r["eclean"] > last else 1
    return 0 if r["eclean"] == NO_ERROR else 1


def _skip_rest(un, u, k, ac):
    while k < 64:
        st, rs, u = un.symbol(ac, u)
        assert not st
        run, s = rs >> 4, rs & 15
        if s == 0:
            if run != 15:
                break
            assert k + 16 <= 64
            k += 16
            continue
        assert k + run <= 63
        st, _, u = un.value(s, u)
        assert not st
        k += run + 1
    return u


class _At:
    """jpegdec_ref's reader interface on a Unit at a bit position."""

    def __init__(self, un, u):
        self.un, self.u = un, u

    def symbol(self, table):
        st, sym, self.u = self.un.symbol(table, self.u)
        return st, sym

    def value(self, s):
        st, v, self.u = self.un.value(s, self.u)
        return st, v


def _decode_block(at, dc, ac, pred, blk):
    """jpegdec_ref.decode_block over 16-bit lookup tables."""
    st, s = at.symbol(dc)
    assert not st
    st, v = at.value(s & 15)
    assert not st
    pred = D._wrap32(pred + D.extend(v, s & 15))
    blk[0] = D._wrap16(pred)
    k = 1
    while k < 64:
        st, rs = at.symbol(ac)
        assert not st
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            continue
        k += r
        st, v = at.value(s)
        assert not st and k <= 63
        blk[D.ZIGZAG[k]] = D.extend(v, s)
        k += 1
    return pred


def substream_decode(p, segment_bytes=DEFAULT_SEGMENT_BYTES, max_rounds=DEFAULT_MAX_ROUNDS):
    """A parsed file (jpegdec_ref.parse) -> (accepted, rounds, coefficient planes or None, segments)."""
    nseg = planned_segments(p, segment_bytes)
    if nseg == 0:
        return 0, 0, None, 0
    g = D.geometry(p)
    s = p["stream"]
    st, units, _ = D.scan(s, 1)
    if st:
        return 0, 0, None, nseg
    uend = units[0][1]
    un = Unit(s, uend)
    dct = [_lookup(*t) for t in p["dc"]]
    act = [_lookup(*t) for t in p["ac"]]
    nb0 = p["hs"] * p["vs"]
    nblk = nb0 + p["ncomp"] - 1
    expected = g["nmcu"] * nblk
    ends = [min((i + 1) * segment_bytes, uend) for i in range(nseg)]
    entry = [guess(s, i, segment_bytes, uend) for i in range(nseg)]
    dirty = [True] * nseg
    res = [None] * nseg
    rounds, converged = 0, False
    while rounds < max_rounds:
        rounds += 1
        for i in range(nseg):
            if dirty[i]:
                res[i] = decode_segment(un, entry[i], ends[i], dct, act, nb0, nblk)
        changed = False
        dirty[0] = False
        for i in range(1, nseg):
            dirty[i] = res[i - 1]["exit"] != entry[i]
            if dirty[i]:
                entry[i] = res[i - 1]["exit"]
                changed = True
        if not changed:
            converged = True
            break
    if not converged:
        return 0, rounds, None, nseg
    before, pred, flags = [], [], 0
    b, dc = 0, [0, 0, 0]
    for i in range(nseg):
        before.append(b)
        pred.append(list(dc))
        flags |= check(entry[i], res[i], b, expected, nblk)
        b += res[i]["owned"]
        dc = [(x + y) & 0xFFFFFFFF for x, y in zip(dc, res[i]["dc"])]
    if flags != 2:
        return 0, rounds, None, nseg
    planes = [np.zeros((g["bh"][c], g["bw"][c], 64), np.int16) for c in range(p["ncomp"])]
    for i in range(nseg):
        if before[i] >= expected or res[i]["owned"] == 0:
            continue
        byte, bit, slot, k = entry[i]
        u = un.to_bit(byte, bit)
        if k:
            u = _skip_rest(un, u, k, act[0 if slot < nb0 else slot - nb0 + 1])
        at = _At(un, u)
        pr = [D._wrap32(x) for x in pred[i]]
        for o in range(before[i], min(before[i] + res[i]["owned"], expected)):
            m, j = divmod(o, nblk)
            c = 0 if j < nb0 else j - nb0 + 1
            h, v = g["samp"][c]
            yy, xx = (j // h, j % h) if c == 0 else (0, 0)
            mx, my = m % g["mcux"], m // g["mcux"]
            pr[c] = _decode_block(at, dct[c], act[c], pr[c], planes[c][my * v + yy, mx * h + xx])
    return 1, rounds, planes, nseg


@functools.lru_cache(maxsize=None)
def decode_file(f, segment_bytes=DEFAULT_SEGMENT_BYTES, max_rounds=DEFAULT_MAX_ROUNDS):
    """substream_decode of a file's bytes, computed once."""
    return substream_decode(D.parse(f), segment_bytes, max_rounds)


def straddles(s, uend, segment_bytes):
    """Segment boundaries inside the unit that fall between an FF and its stuffed 00."""
    return [b for b in range(segment_bytes, uend, segment_bytes) if s[b] == 0 and s[b - 1] == 0xFF]
