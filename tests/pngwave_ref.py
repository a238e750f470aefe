"""Plain Python restatement of the PNG decoder's wave route (attwarp_amd/csrc/pngdec_wave_blocks.hpp) in
the bit domain: windows of 64 segments, Jacobi rounds over the segments' entry bits, the true chain, the write pass in
runs that fit the staging and match buffers, the match-resolution rounds and the acceptance rule.  It decides windows,
rounds, resolution rounds and acceptance of any file before a GPU run; on every accepted file its bytes must equal
tests/pngdec_ref.py's serial decode.  Integer arithmetic only."""
from __future__ import annotations

import functools
import zlib

import png_ref as R
import pngdec_ref as D

WAVE = 64
RING, STAGE, MATCHES, STORED_CHUNK = 32768, 8192, 1024, 16384
MAX_STREAM = 1 << 28
NONE = None
SEGMENT_BYTES, MAX_ROUNDS = 64, 64                     # the defaults of attwarp_amd.png


def _peek(s, pos):
    """The bits from `pos` on (24 at least, zeros behind the stream's end)."""
    return int.from_bytes(s[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)


def _take(s, pos, nb):
    if pos + nb > 8 * len(s):
        return None, pos
    return _peek(s, pos) & ((1 << nb) - 1), pos + nb


def _decode(s, pos, tab):
    e = tab[_peek(s, pos) & 0x7FFF]
    if e is None or pos + e[1] > 8 * len(s):
        return None, pos
    return e[0], pos + e[1]


def token(s, pos, lit, dist):
    """pw_token: (kind, a, b, position behind it); kind 0 literal a, 1 match of a bytes at distance b, 2 end of block, 3 error."""
    sym, pos = _decode(s, pos, lit)
    if sym is None:
        return 3, 0, 0, pos
    if sym < 256:
        return 0, sym, 0, pos
    if sym == 256:
        return 2, 0, 0, pos
    sym -= 257
    if sym >= 29:
        return 3, 0, 0, pos
    v, pos = _take(s, pos, R.LEN_EXTRA[sym])
    if v is None:
        return 3, 0, 0, pos
    ln = R.LEN_BASE[sym] + v
    sym, pos = _decode(s, pos, dist)
    if sym is None or sym >= 30:
        return 3, 0, 0, pos
    v, pos = _take(s, pos, D.DIST_EXTRA[sym])
    if v is None:
        return 3, 0, 0, pos
    return 1, ln, D.DIST_BASE[sym] + v, pos


@functools.lru_cache(maxsize=64)
def _tables(lens, nlen):
    dist = D.build(list(lens[nlen:]), True)
    lit = D.build(list(lens[:nlen]), True)
    return lit, dist


def read_lengths(s, pos):
    """pw_read_lengths: a dynamic block's header behind its three bits -> (lit table, dist table, first symbol's bit) or None."""
    v, pos = _take(s, pos, 14)
    if v is None:
        return None
    nlen, ndist, ncode = 257 + (v & 31), 1 + ((v >> 5) & 31), 4 + (v >> 10)
    if nlen > 286 or ndist > 30:
        return None
    cl = [0] * 19
    for i in range(ncode):
        v, pos = _take(s, pos, 3)
        if v is None:
            return None
        cl[R.CL_ORDER[i]] = v
    ctab = D.build(cl, False)
    if ctab is None:
        return None
    lens, total = [], nlen + ndist
    while len(lens) < total:
        sym, pos = _decode(s, pos, ctab)
        if sym is None:
            return None
        if sym < 16:
            lens.append(sym)
            continue
        val = 0
        if sym == 16:
            if not lens:
                return None
            val, nb, base = lens[-1], 2, 3
        elif sym == 17:
            nb, base = 3, 3
        else:
            nb, base = 7, 11
        v, pos = _take(s, pos, nb)
        if v is None or len(lens) + base + v > total:
            return None
        lens += [val] * (base + v)
    if lens[256] == 0:
        return None
    lit, dist = _tables(tuple(lens), nlen)
    if dist is None or lit is None:
        return None
    return lit, dist, pos


def scan(s, entry, segend, lit, dist):
    """pw_scan: one lane's round -> (exit, bytes, matches, eob start, eob end, error)."""
    if entry is NONE:
        return NONE, 0, 0, NONE, NONE, 0
    if entry >= 8 * len(s):
        return NONE, 0, 0, NONE, NONE, 1
    pos, nb, nm = entry, 0, 0
    while True:
        if pos >= segend:
            return pos, nb, nm, NONE, NONE, 0
        k, a, _, nxt = token(s, pos, lit, dist)
        if k == 0:
            nb += 1
        elif k == 1:
            nb += a
            nm += 1
        elif k == 2:
            return NONE, nb, nm, pos, nxt, 0
        else:
            return NONE, nb, nm, NONE, NONE, 1
        pos = nxt


class Result:
    def __init__(self):
        self.out = bytearray()
        self.windows = self.rounds = self.resolution_rounds = 0
        self.accepted = 0
        self.window_rounds = []                     # rounds of every window, for the table in DESIGN.md

    @property
    def info(self):
        return (self.windows, self.rounds, self.accepted)


def wave_inflate(s, filt_bytes, segment_bytes=SEGMENT_BYTES, max_rounds=MAX_ROUNDS):
    """pw_image over the zlib stream s (its header already accepted) -> Result; Result.out is the filtered bytes when accepted."""
    s = bytes(s)
    n = len(s)
    res = Result()
    out = res.out
    segbits = 8 * segment_bytes
    bit, bfinal = 16, 0
    fail = n >= MAX_STREAM or n < 2
    while not fail:
        if bit >= 8 * n:
            fail = True
            break
        hdr, pos = _take(s, bit, 3)
        if hdr is None:
            fail = True
            break
        bfinal, btype = hdr & 1, hdr >> 1
        if btype == 3:
            fail = True
            break
        if btype == 0:
            at = (pos + 7) >> 3
            if at + 4 > n:
                fail = True
                break
            ln, nln = s[at] | s[at + 1] << 8, s[at + 2] | s[at + 3] << 8
            at += 4
            if ln ^ nln != 0xFFFF or ln > n - at or ln > filt_bytes - len(out):
                fail = True
                break
            out += s[at:at + ln]
            bit = 8 * (at + ln)
        else:
            if btype == 2:
                t = read_lengths(s, pos)
                if t is None:
                    fail = True
                    break
                lit, dist, bit = t
            else:
                lit, dist = D._fixed()
                bit = pos
            wbase = bit
            while True:                                       # windows
                entry = [bit] + [wbase + j * segbits for j in range(1, WAVE)]
                dirty = [True] * WAVE
                lanes = [None] * WAVE
                rounds, converged = 0, False
                while rounds < max_rounds:
                    rounds += 1
                    for j in range(WAVE):
                        if dirty[j]:
                            lanes[j] = scan(s, entry[j], wbase + (j + 1) * segbits, lit, dist)
                        dirty[j] = False
                    changed = False
                    for j in range(1, WAVE):
                        ex = lanes[j - 1][0]
                        if ex is not NONE and ex != entry[j]:
                            entry[j], dirty[j], changed = ex, True, True
                    if not changed:
                        converged = True
                        break
                res.windows += 1
                res.rounds += rounds
                res.window_rounds.append(rounds)
                nl, end, total, bad = WAVE, False, 0, not converged
                if not bad:
                    for j in range(WAVE):
                        _, nb, _, e0, _, er = lanes[j]
                        if er or nb > filt_bytes - len(out) - total:
                            bad = True
                            break
                        total += nb
                        if e0 is not NONE:
                            nl, end = j + 1, True
                            break
                if bad:
                    fail = True
                    break
                if not _write_pass(s, res, lanes, entry, nl, lit, dist, filt_bytes):
                    fail = True
                    break
                if end:
                    bit = lanes[nl - 1][4]
                    break
                bit = lanes[WAVE - 1][0]
                wbase += WAVE * segbits
            if fail:
                break
        if bfinal:
            break
    end = (bit + 7) >> 3
    res.accepted = int(not fail and bfinal == 1 and len(out) == filt_bytes and end <= n and n - end >= 4 and
                       int.from_bytes(s[end:end + 4], "big") == D.adler32(bytes(out)))
    res.adler_pos = end
    return res


def _write_pass(s, res, lanes, entry, nl, lit, dist, filt_bytes):
    """The runs of one window's true chain: emission, resolution rounds, commit.  False: a match before the first byte."""
    out = res.out
    cur = list(entry[:nl])
    stop = [lanes[j][3] if lanes[j][3] is not NONE else lanes[j][0] for j in range(nl)]
    nbytes = [lanes[j][1] for j in range(nl)]
    nmatch = [lanes[j][2] for j in range(nl)]
    a = 0
    while True:
        while a < nl and (cur[a] >= stop[a] or nbytes[a] == 0):
            a += 1
        if a >= nl:
            return True
        run = []                                              # (lane, stage offset, byte budget, match budget)
        if nbytes[a] <= STAGE and nmatch[a] <= MATCHES:
            b, ob, om = a, 0, 0
            while b < nl and ob + nbytes[b] <= STAGE and om + nmatch[b] <= MATCHES:
                run.append((b, ob, nbytes[b], nmatch[b]))
                ob += nbytes[b]
                om += nmatch[b]
                b += 1
        else:
            run.append((a, 0, STAGE, MATCHES))
        produced = len(out)
        stage = bytearray(STAGE)
        pending, roffs, run_bytes = [], [], 0                 # per lane of the run: its matches (dst, len, dist), in order
        for j, ro, bb, mb in run:
            pos, ob, ms = cur[j], 0, []
            while pos < stop[j]:
                k, x, y, nxt = token(s, pos, lit, dist)
                if k == 0:
                    if ob + 1 > bb:
                        break
                    stage[ro + ob] = x
                    ob += 1
                elif k == 1:
                    if ob + x > bb or len(ms) + 1 > mb:
                        break
                    if y > produced + ro + ob:
                        return False
                    ms.append((ro + ob, x, y))
                    ob += x
                else:
                    raise AssertionError("the rounds saw this chain clean")
                pos = nxt
            cur[j] = pos
            nbytes[j] -= ob
            nmatch[j] -= len(ms)
            assert len(run) == 1 or ob == bb
            pending.append(ms)
            roffs.append(ro)
            run_bytes = ro + ob
        assert 0 < run_bytes <= min(STAGE, filt_bytes - produced)
        done = [0] * len(run)
        while True:                                           # resolution rounds
            low = next((pending[i][done[i]][0] for i in range(len(run)) if done[i] < len(pending[i])), None)
            if low is None:
                break
            res.resolution_rounds += 1
            snapshot = list(done)                             # (every lane works against the same `low`; bytes it reads are final)
            for i in range(len(run)):
                ro = roffs[i]
                while done[i] < len(pending[i]):
                    dst, ln, d = pending[i][done[i]]
                    src = dst - d
                    last = min(src + ln, dst)
                    if not (last <= low or src >= ro or low >= ro):
                        break
                    for k in range(ln):
                        q = src + k
                        stage[dst + k] = out[produced + q] if q < 0 else stage[q]
                    done[i] += 1
            assert done != snapshot
        out += stage[:run_bytes]


# ---- whole files --------------------------------------------------------------------------------------------------------------
def decode_stream(s, filt_bytes, segment_bytes=SEGMENT_BYTES, max_rounds=MAX_ROUNDS):
    """pw_image as the host program prints it: zlib stream -> (filtered bytes or None, (windows, rounds, accepted),
    resolution rounds); a stream whose zlib header fails is never given to it: (None, (0, 0, 0), 0)."""
    if D.zlib_header(s) != D.OK:
        return None, (0, 0, 0), 0
    r = wave_inflate(s, filt_bytes, segment_bytes, max_rounds)
    return (bytes(r.out) if r.accepted else None), r.info, r.resolution_rounds


def decode_file(f, segment_bytes=SEGMENT_BYTES, max_rounds=MAX_ROUNDS, force_serial=False, check_crc=True):
    """pngdec_wave_kernel over one 8-bit non-interlaced file -> the same triple, as PngFiles.wave_info() reads it back.  The
    kernel runs pw_image for an image of the serial route (force_serial: for every image) whose chunk CRCs are right -- any
    other has (0, 0, 0) -- and takes its acceptance back when a row's filter byte is above 4."""
    p = D.parse(f)
    rb = 1 + p["W"] * D.CHANNELS[p["color_type"]]
    s = p["stream"]
    if D.zlib_header(s) != D.OK or (check_crc and any(zlib.crc32(b"IDAT" + c) != crc for c, crc in p["chunks"])):
        return None, (0, 0, 0), 0
    if not force_serial and D.decode_stream(s, p["H"] * rb)[2]["route"] != "serial":
        return None, (0, 0, 0), 0
    out, (w, r, acc), rr = decode_stream(s, p["H"] * rb, segment_bytes, max_rounds)
    if acc and any(out[y * rb] > 4 for y in range(p["H"])):
        out, acc = None, 0
    return out, (w, r, acc), rr
