"""Files that put the PNG decoder at its code, scan, chunk, row and carry limits (test_pngdec_limits_ref_cpu.py,
test_pngdec_limits_gpu.py and the host program of test_pngdec_host_cpu.py).  A token-level DEFLATE writer (code lengths
and tokens in, one block out) builds the streams zlib never writes: 15-bit codes on both trees, codes on the two sides of
the primary tables, every repeat code at its smallest and largest count, stored blocks at every bit offset, streams that
end at every distance from a dword, and sync patterns at chosen stream offsets.  Every builder knows the filtered bytes
its file decodes to (filtered_of) and the tags of what it wrote (features); test_pngdec_limits_ref_cpu.py proves both from
the bytes.  Everything is deterministic and cached."""
from __future__ import annotations

import functools
import random
import struct
import zlib

import png_cases as PC
import png_ref as R
import pngdec_cases as C
import pngdec_ref as D

MARKER = C.MARKER
CAP = 4096                                   # filtered bytes of a seeded stream at most (one grey row)
SEEDED = 160
SEED0 = 7000                                 # seeds SEED0, SEED0 + 1, ... : the first SEEDED that give two bytes or more
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def chunk(kind, payload, crc=None):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) if crc is None else crc)


def make_png(W, H, ch, parts):
    """A file around the IDAT payloads `parts` (one stream: one chunk)."""
    if isinstance(parts, (bytes, bytearray)):
        parts = [bytes(parts)]
    return (D.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, C.CTYPE[ch], 0, 0, 0)) +
            b"".join(p[0] if isinstance(p, tuple) else chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b""))


def zstream(deflate, data):
    return b"\x78\x01" + deflate + struct.pack(">I", zlib.adler32(bytes(data)))


# ---- the writer ----------------------------------------------------------------------------------------------------------------
class Writer(R.BitWriter):
    """png_ref.BitWriter that spills whole bytes, so that long streams stay linear."""

    def __init__(self):
        super().__init__()
        self.buf = bytearray()

    def put(self, value, nbits):
        super().put(value, nbits)
        if self.n >= 8:
            k = self.n // 8
            self.buf += (self.acc & ((1 << 8 * k) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def to_bytes(self):
        return bytes(self.buf) + super().to_bytes()


def cl_code(hist):
    """A complete code of at most 7 bits over the code-length symbols in use (two at least)."""
    hist = list(hist)
    if sum(1 for h in hist if h) < 2:
        hist[1 if hist[0] else 0] += 1
    return R.code_lengths(hist, limit=7)


def rle_plan(seq, rng=None):
    """Code lengths -> [(code-length symbol, extra value)] with 16 / 17 / 18; rng: random run counts, else the longest."""
    plan, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            n = min(run, 138)
            if rng is not None:
                n = rng.randint(3, n)
            plan.append((18, n - 11) if n >= 11 else (17, n - 3))
            i += n
        elif v != 0 and run >= 4:
            n = min(run - 1, 6)
            if rng is not None:
                n = rng.randint(3, n)
            plan += [(v, 0), (16, n - 3)]
            i += 1 + n
        else:
            plan.append((v, 0))
            i += 1
    return plan


def expand_plan(plan):
    seq = []
    for s, e in plan:
        if s < 16:
            seq.append(s)
        elif s == 16:
            seq += [seq[-1]] * (3 + e)
        else:
            seq += [0] * ((3 if s == 17 else 11) + e)
    return seq


class Deflate:
    """Blocks into one bit stream; `out` is what they decode to.  Tokens: an int (literal), (length, distance) or (length,
    distance, length symbol), and for broken streams ("lit" | "dist", symbol) -- that symbol's code alone -- and ("bits",
    value, count)."""

    def __init__(self):
        self.w, self.out, self.tags = Writer(), bytearray(), set()
        self.lit_used, self.dist_used = set(), set()          # code lengths used by a token (not by the end-of-block code)

    def stored(self, data=b"", final=False):
        w = self.w
        w.put(int(final), 1)
        w.put(0, 2)
        self.tags.add(f"stored_at_bit{(w.bitpos - 3) % 8}")
        if w.n:
            w.put(0, 8 - w.n)
        assert len(data) <= 65535
        w.buf += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + bytes(data)
        self.out += data
        if len(data) == 0 and final:
            self.tags.add("stored_len0_final")
        if len(data) == 65535:
            self.tags.add("stored_65535")
        return self

    def tokens(self, toks, ll, dl, eob=True):
        w, out = self.w, self.out
        lc, dc = R.canonical_codes(list(ll)), R.canonical_codes(list(dl))
        for t in toks:
            if isinstance(t, int):
                assert ll[t]
                w.put(lc[t], ll[t])
                out.append(t)
                self.lit_used.add(ll[t])
            elif t[0] == "bits":
                w.put(t[1], t[2])
            elif t[0] == "lit":
                w.put(lc[t[1]], ll[t[1]])
            elif t[0] == "dist":
                w.put(dc[t[1]], dl[t[1]])
            else:
                length, dist = t[0], t[1]
                sym = t[2] if len(t) > 2 else R.length_symbol(length)[0]
                k = sym - 257
                ev = length - R.LEN_BASE[k]
                assert ll[sym] and 0 <= ev < (1 << R.LEN_EXTRA[k]) and 1 <= dist <= 32768
                w.put(lc[sym], ll[sym])
                w.put(ev, R.LEN_EXTRA[k])
                d = max(j for j in range(30) if D.DIST_BASE[j] <= dist)
                assert dl[d] and dist <= len(out)
                w.put(dc[d], dl[d])
                w.put(dist - D.DIST_BASE[d], D.DIST_EXTRA[d])
                for _ in range(length):
                    out.append(out[-dist])
                self.lit_used.add(ll[sym])
                self.dist_used.add(dl[d])
                self.tags.add(f"len{length}_sym{sym}" + (f"_{ev}" if sym == 284 and ev == 31 else ""))
                if dist in (2, 3, 4, 32768) and length in (3, 258):
                    self.tags.add(f"len{length}_dist{dist}")
        if eob:
            w.put(lc[256], ll[256])
        return self

    def fixed(self, toks, final=False, eob=True):
        self.w.put(int(final), 1)
        self.w.put(1, 2)
        return self.tokens(toks, FIXED_LIT, FIXED_DIST, eob)

    def dynamic(self, ll, dl, toks, final=False, plan=None, rle=False, hlit=None, hdist=None, hclen=None, cl=None, rng=None, eob=True):
        """One dynamic block.  ll / dl: code lengths by symbol (zeros fill up to HLIT / HDIST, by default the smallest that
        hold them).  plan: the code-length symbols themselves [(symbol, extra value)] -- ll / dl then only serve the tokens;
        else plain lengths, or (rle) runs.  toks None: the header alone.  Nothing is checked: broken headers come from here too."""
        ll, dl = list(ll) + [0] * (288 - len(ll)), list(dl) + [0] * (32 - len(dl))
        if hlit is None:
            hlit = max(257, max(i + 1 for i in range(288) if ll[i]))
        if hdist is None:
            hdist = max([1] + [i + 1 for i in range(32) if dl[i]])
        if plan is None:
            seq = ll[:hlit] + dl[:hdist]
            plan = rle_plan(seq, rng) if rle else [(l, 0) for l in seq]
        hist = [0] * 19
        for s, _ in plan:
            hist[s] += 1
        if cl is None:
            cl = cl_code(hist)
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cl[R.CL_ORDER[i]]])
        w = self.w
        w.put(int(final), 1)
        w.put(2, 2)
        w.put(hlit - 257, 5)
        w.put(hdist - 1, 5)
        w.put(hclen - 4, 4)
        for i in range(hclen):
            w.put(cl[R.CL_ORDER[i]], 3)
        cc = R.canonical_codes(list(cl))
        at = 0
        for s, e in plan:
            w.put(cc[s], cl[s])
            if s >= 16:
                w.put(e, {16: 2, 17: 3, 18: 7}[s])
                n = (11 if s == 18 else 3) + e
                self.tags.add(f"rep{s}_{n}")
                if at < hlit < at + n:
                    self.tags.add(f"rep{s}_across_border")
                at += n
            else:
                at += 1
        self.tags |= {f"hlit{hlit}", f"hdist{hdist}"}
        nd = sum(1 for l in dl[:hdist] if l)
        if nd == 0:
            self.tags.add("nodist")
        if nd == 1 and max(dl) == 1:
            self.tags.add("single_dist")
        if [i for i in range(288) if ll[i]] == [256]:
            self.tags.add("eob_only")
        if toks is not None:
            self.tokens(toks, ll, dl, eob)
        return self

    def bytes(self):
        return self.w.to_bytes()

    def stream(self):
        return zstream(self.w.to_bytes(), self.out)


def lens_of(pairs, n):
    out = [0] * n
    for s, l in pairs:
        out[s] = l
    return out


def fill(n, dist):
    """Matches at `dist` that make n bytes (n >= 3), each 3 .. 258 long."""
    out = []
    while n:
        k = 258 if n >= 261 or n == 258 else (n if n <= 258 else n - 3)
        out.append((k, dist))
        n -= k
    return out


def filler(n, seed):
    """n bytes without 00 and FF: nothing in them is part of a sync pattern."""
    return bytes(random.Random(seed).randrange(1, 255) for _ in range(n))


class Case:
    def __init__(self, name, file, features, filtered, **expect):
        self.name, self.file, self.features, self.filtered, self.expect = name, file, set(features) | {name}, bytes(filtered), expect


def _row(name, df, tags=(), **expect):
    """One grey row around the stream of a Deflate."""
    data = bytes(df.out)
    assert data[0] == 0 and 2 <= len(data) <= CAP, (name, len(data))
    return Case(name, make_png(len(data) - 1, 1, 1, df.stream()), df.tags | set(tags), data, **expect)


# ---- codes ---------------------------------------------------------------------------------------------------------------------
SKEW = list(range(1, 15)) + [15, 15]                      # sixteen codes of 1, 2, ..., 14, 15 and 15 bits


def _code_cases():
    c = []
    # lit15: literals 0 .. 11 and 77 and the lengths 3 and 258 next to the end-of-block code; the 15-bit codes on 77 and 285
    syms = list(range(12)) + [256, 257, 77, 285]
    ll = lens_of(zip(syms, SKEW), 286)
    toks = list(range(12)) + [77, (3, 5), 77, (258, 7), 3, 77]
    df = Deflate().dynamic(ll, [3] * 8, toks, final=True)
    assert 15 in df.lit_used and max(ll) == 15
    c.append(_row("lit15", df))
    # dist15: seven stored rows of 4096 bytes, the eighth from matches over 16 distance symbols, the 15-bit codes on 0 and 29
    img = PC.noise(7, 4095, 1, 31)
    rows7 = C.filtered_cycle(img, 1)
    dsyms = [1, 2, 3, 5, 8, 10, 13, 16, 19, 22, 24, 26, 27, 28, 0, 29]
    dl = lens_of(zip(dsyms, SKEW), 30)
    ll = lens_of([(0, 2), (256, 2), (257, 2), (264, 2)], 286)
    df = Deflate().stored(rows7)
    toks = [0] + [((3, 10)[i & 1], D.DIST_BASE[d] + (D.DIST_EXTRA[d] and 1)) for i, d in enumerate(dsyms)] + [(3, 1), (10, 24577 + 4095)]
    toks += [(10, 1)] * ((4095 - sum(t[0] for t in toks[1:])) // 10)
    toks += [0] * (4095 - sum(t[0] for t in toks[1:]))
    df.dynamic(ll, dl, toks, final=True)
    assert len(df.out) == 8 * 4096 and df.dist_used == set(range(1, 16))
    c.append(Case("dist15", make_png(4095, 8, 1, df.stream()), df.tags | {"dist_code_15_used"}, df.out))
    # codes of exactly 10 and 11 bits / 8 and 9 bits: the two sides of the primary tables
    lens = list(range(1, 9)) + [10, 10, 11, 11, 11, 11]
    syms = list(range(9)) + [256, 100, 200, 257, 260]
    df = Deflate().dynamic(lens_of(zip(syms, lens), 286), [1, 1], list(range(9)) + [100, 200, (3, 1), (6, 2), 200, 100, (6, 1)], final=True)
    assert {10, 11} <= df.lit_used
    c.append(_row("lit_10_11", df))
    lens = list(range(1, 7)) + [8, 8, 9, 9, 9, 9]
    df = Deflate()
    toks = list(range(70)) + [(3 + d % 4, D.DIST_BASE[d]) for d in range(12)] + [(4, D.DIST_BASE[d] + D.DIST_EXTRA[d]) for d in range(8, 12)]
    df.dynamic(lens_of([(i, 7) for i in range(80)] + [(i, 4) for i in range(256, 262)], 286),
               lens_of(zip([11, 10, 9, 8, 7, 6, 0, 1, 2, 3, 4, 5], lens), 30), toks, final=True)
    assert {8, 9} <= df.dist_used
    c.append(_row("dist_8_9", df))
    # every symbol has a code: HLIT = 286, HDIST = 30
    ll = [8] * 226 + [9] * 60
    dl = [4] * 2 + [5] * 28
    df = Deflate().dynamic(ll, dl, [0] + list(range(200, 256)) + [(258, 1), (17, 30), (227, 19)], final=True, rle=True)
    assert {"hlit286", "hdist30"} <= df.tags
    c.append(_row("hlit286_hdist30", df))
    ll = lens_of([(i, 3) for i in range(7)] + [(256, 3)], 286)
    df = Deflate().dynamic(ll, [0], [0, 1, 2, 3, 4, 5, 6, 6, 5], final=True)
    assert {"hlit257", "hdist1", "nodist"} <= df.tags
    c.append(_row("hlit257_hdist1_nodist", df))
    ll = lens_of([(0, 2), (9, 2), (256, 2), (258, 2)], 286)
    df = Deflate().dynamic(ll, [0, 0, 1], [0, 9, 9, 0, (4, 3), 9, (4, 3)], final=True)
    assert "single_dist" in df.tags
    c.append(_row("single_dist", df))
    df = Deflate().dynamic(lens_of([(256, 1)], 286), [0], [])
    assert "eob_only" in df.tags
    df.dynamic(ll, [0, 0, 1], [0, 9, 0, 9, (4, 3)], final=True)
    c.append(_row("eob_only_then_block", df))
    return c


# ---- repeat codes --------------------------------------------------------------------------------------------------------------
def _repeat_cases():
    c = []
    z = lambda n: (18, n - 11) if n >= 11 else (17, n - 3)
    plans = {"rep16_3": [(3, 0), (16, 0), (3, 0), (3, 0), (3, 0), z(138), z(111), (3, 0), (0, 0)],
             "rep16_6": [(3, 0), (16, 3), z(138), z(111), (3, 0), (0, 0)],
             "rep17_3": [(2, 0)] * 3 + [z(3), z(138), z(112), (2, 0), (0, 0)],
             "rep17_10": [(2, 0)] * 3 + [z(10), z(138), z(105), (2, 0), (0, 0)],
             "rep18_11": [(2, 0)] * 3 + [z(11), z(138), z(104), (2, 0), (0, 0)],
             "rep18_138": [(2, 0)] * 3 + [z(138), z(115), (2, 0), (0, 0)]}
    for name, plan in plans.items():
        seq = expand_plan(plan)
        assert len(seq) == 258 and seq[256]
        used = [i for i in range(256) if seq[i]]
        df = Deflate().dynamic(seq[:257], seq[257:], used + used[::-1], final=True, plan=plan, hlit=257, hdist=1)
        assert name in df.tags
        c.append(_row(name, df))
    # a 16-run over 257, 258 and four distance lengths; then an 18-run over 257 .. 259 and eight distance lengths
    planA = [(2, 0), z(138), z(117), (2, 0), (16, 3)]
    seq = expand_plan(planA)
    assert len(seq) == 259 + 4
    df = Deflate().dynamic(seq[:259], seq[259:], [0, 0, 0, 0, 0, (3, 1), (4, 2), (3, 3), (4, 4)], plan=planA, hlit=259, hdist=4)
    assert "rep16_across_border" in df.tags
    planB = [(1, 0), z(138), z(117), (1, 0), z(11), (1, 0)]
    seq = expand_plan(planB)
    assert len(seq) == 260 + 9
    df.dynamic(seq[:260], seq[260:], [0] * 20, plan=planB, hlit=260, hdist=9, final=True)
    assert "rep18_across_border" in df.tags
    c.append(_row("rep_across_border", df))
    return c


# ---- lengths, distances, stored blocks, tails, the unit border -------------------------------------------------------------
def _match_cases():
    c = []
    lits = [0] + list(range(10, 40))
    c.append(_row("len258_sym285", Deflate().fixed(lits + [(258, 31)], final=True)))
    c.append(_row("len258_sym284_31", Deflate().fixed(lits + [(258, 31, 284), 7, (258, 9, 284)], final=True)))
    for d in (2, 3, 4):
        c.append(_row(f"overlap_d{d}", Deflate().fixed(lits + [(258, d), 5, (258, d)], final=True)))
    row = b"\x00" + PC.noise(1, 32767, 1, 41).tobytes()
    for first in (3, 258):
        df = Deflate().stored(row).fixed([(first, 32768)] + fill(32768 - first, 32768), final=True)
        assert bytes(df.out) == row + row
        c.append(Case(f"len{first}_dist32768", make_png(32767, 2, 1, df.stream()), df.tags, df.out))
    return c


def _stored_cases():
    c = []
    rest = filler(40, 3)
    for b in range(8):
        df = Deflate().fixed([0] + [150 + i for i in range((b - 2) % 8)])
        assert df.w.bitpos % 8 == b
        c.append(_row(f"stored_at_bit{b}", df.stored(rest, final=True)))
    c.append(_row("stored_len0_final", Deflate().fixed([0] + list(rest)).stored(b"", final=True)))
    f = C.filtered_cycle(PC.noise(15, 4368, 1, 5))
    df = Deflate().stored(f, final=True)
    c.append(Case("stored_65535", make_png(4368, 15, 1, df.stream()), df.tags, f))
    # the final Huffman block starts 3 .. 14 bytes in front of the Adler-32: every change of the bit reader from its dword
    # look-ahead to single bytes happens inside that block
    head = b"\x00" + filler(30, 4)
    for j in range(12):
        df = Deflate().stored(head).fixed([60 + i for i in range(j + 1)], final=True)
        c.append(_row(f"tail_{j}", df))
    return c


def _reach_cases():
    c, k = [], 9
    for name, dist, route, chain in (("reach_exact", k, "unit", 2), ("reach_one_more", k + 1, "serial", 0)):
        df = Deflate().fixed([0] + list(range(20, 50))).stored(b"").fixed(list(range(100, 100 + k)) + [(40, dist), 7], final=True)
        c.append(_row(name, df, route=route, chain=chain, nkept=2))
    assert len(c[0].file) == len(c[1].file) and sum(a != b for a, b in zip(c[0].file, c[1].file)) > 0
    return c


# ---- the marker scan: stored-only streams, the payload starts at stream offset 7 -------------------------------------------
def _stored_row(payload):
    return b"\x78\x01\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xFFFF) + payload + struct.pack(">I", zlib.adler32(payload))


def _with_patterns(n, offsets, seed):
    """n payload bytes (the first 0) with 00 00 FF FF at the given STREAM offsets."""
    p = bytearray(b"\x00" + filler(n - 1, seed))
    for off in offsets:
        assert 1 <= off - 7 and off - 7 + 4 <= n
        p[off - 7:off - 3] = MARKER
    return bytes(p)


def _scan_cases():
    c = []
    for k in range(8):
        off = 2 + 8 * 5 + k
        p = _with_patterns(200, [off], 50 + k)
        c.append(Case(f"scan_k{k}", make_png(199, 1, 1, _stored_row(p)), (), p, kept=[2, off + 4], route="unit", chain=1))
    for off in range(2046, 2051):
        p = _with_patterns(2100, [off], off)
        c.append(Case(f"scan_tile_{off}", make_png(2099, 1, 1, _stored_row(p)), (), p, kept=[2, off + 4], route="unit", chain=1))
        # the same offset as the LEN / NLEN of a real empty stored block: its header byte stands at off - 1
        p = b"\x00" + filler(2099, off + 10)
        df = Deflate().stored(p[:off - 8]).stored(b"").stored(p[off - 8:], final=True)
        s = df.stream()
        assert s[off:off + 4] == MARKER and s.count(MARKER) == 1
        c.append(Case(f"scan_tile_true_{off}", make_png(2099, 1, 1, s), df.tags, p, kept=[2, off + 4], route="unit", chain=2))
    # the payload ends with the pattern, so the kept position is the Adler-32's first byte; the thread that finds it stands
    # less than 12 bytes in front of the stream's end and reads byte by byte, the pattern its candidate 0, 1, 2 or 3
    for k in range(4):
        p = b"\x00" + filler(98 + k, 60 + k) + MARKER
        assert (len(p) + 3 - 2) % 8 == k
        c.append(Case("scan_tail" + (f"_k{k}" if k else ""), make_png(len(p) - 1, 1, 1, _stored_row(p)), (), p,
                      kept=[2, 7 + len(p)], route="unit", chain=1))
    # 275 patterns, one every 16 bytes; 255 are kept, the last of them at 4083 in the second tile of 2048 candidates
    offs = [15 + 16 * i for i in range(275)]
    p = _with_patterns(4400, offs, 61)
    assert p[2200] == 0
    c.append(Case("scan_cap_second_tile", make_png(2199, 2, 1, _stored_row(p)), (), p,
                  kept=[2] + [19 + 16 * i for i in range(255)], route="unit", chain=1))
    return c


# ---- IDAT chunks ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rgba_stream():
    f = C.filtered_cycle(PC.photo(70, 9, 4, 12))
    s = zlib.compress(f, 6)
    assert len(s) > 600
    return f, s


def _chunk_cases():
    f, s = _rgba_stream()
    h = len(s) // 2
    c = [Case("idat_empty_first_mid_last", make_png(9, 70, 4, [b"", s[:h], b"", s[h:], b""]), (), f)]
    for n in (255, 256, 257, 511, 512, 513):
        c.append(Case(f"idat_len_{n}", make_png(9, 70, 4, [s[:n], s[n:]]), (), f))
    c.append(Case("idat_all_empty_but_one", make_png(9, 70, 4, [b"", b"", s, b"", b""]), (), f))
    return c


# ---- the unfilter carry --------------------------------------------------------------------------------------------------------
def _carry_cases():
    c = []
    for ch in (1, 2, 4):
        for s in range(5):
            f = C.filtered_cycle(PC.noise(129, 7, ch, 70 + 5 * ch + s), s)
            assert {f[r * (1 + 7 * ch)] for r in (63, 64, 128)} == {(s + r) % 5 for r in (63, 64, 128)}
            c.append(Case(f"carry_c{ch}_s{s}", make_png(7, 129, ch, zlib.compress(f, 6)), [f"carry_c{ch}", f"row64_filter{(s + 64) % 5}"], f))
    for H in (63, 64, 65, 127, 128):
        for W in (1, 2):
            f = C.filtered_cycle(PC.noise(H, W, 4, 100 + H + W), H + W)
            c.append(Case(f"carry_h{H}_w{W}", make_png(W, H, 4, zlib.compress(f, 6)), [f"carry_h{H}"], f))
    f = C.filtered_plain(PC.noise(65, 7, 3, 99), 3)
    c.append(Case("avg_row64_c3", make_png(7, 65, 3, zlib.compress(f, 6)), (), f))
    return c


# ---- seeded dynamic-Huffman streams ------------------------------------------------------------------------------------------
def random_tree(rng, n, maxlen=15, deep=0.5):
    """Code lengths of a complete code over n symbols (n == 1: one code of one bit), at most maxlen bits."""
    if n < 2:
        return [1] * n
    leaves = [1, 1]
    while len(leaves) < n:
        cand = [i for i, l in enumerate(leaves) if l < maxlen]
        i = max(cand, key=lambda i: leaves[i]) if rng.random() < deep else rng.choice(cand)
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    return leaves


def _extra(rng, eb):
    return (0, (1 << eb) - 1, rng.randrange(1 << eb))[rng.randrange(3)]


def seeded_stream(seed):
    """-> (Deflate, info) of one to four dynamic blocks; info: sync (empty stored blocks between the blocks), lit_max /
    dist_max (the longest code a token used), lit_used / dist_used (every length used), mod16."""
    rng = random.Random(seed)
    df = Deflate()
    nblocks, sync = rng.randint(1, 4), seed % 3 == 0
    local = sync and rng.random() < 0.7                   # matches stay inside their unit: the unit route
    unit0 = 0
    for b in range(nblocks):
        lits = [0] + rng.sample(range(1, 256), rng.choice([0, 1, 2, 7, 30, 100, 255, rng.randint(0, 255)]))
        lsyms = rng.sample(range(257, 286), rng.randint(0, 29))
        dsyms = rng.sample(range(30), rng.randint(0, 30))
        syms = lits + [256] + lsyms
        rng.shuffle(syms)
        ll = lens_of(zip(syms, random_tree(rng, len(syms), 15, rng.random())), 286)
        dl = lens_of(zip(dsyms, random_tree(rng, len(dsyms), 15, rng.random())), 30)
        toks, made = ([0], 1) if b == 0 else ([], 0)
        for _ in range(rng.randint(0, 90)):
            have = len(df.out) + made
            reach = have - unit0 if local else have
            near = [d for d in dsyms if D.DIST_BASE[d] <= reach]
            if lsyms and near and rng.random() < 0.5:
                s, d = rng.choice(lsyms), rng.choice(near)
                length = R.LEN_BASE[s - 257] + _extra(rng, R.LEN_EXTRA[s - 257])
                dist = D.DIST_BASE[d] + _extra(rng, D.DIST_EXTRA[d])
                if dist > reach:
                    dist = rng.randint(D.DIST_BASE[d], reach)
                if have + length > CAP:
                    break
                toks.append((length, dist, s))
                made += length
            else:
                if have + 1 > CAP:
                    break
                toks.append(rng.choice(lits))
                made += 1
        hlit = rng.randint(max(257, max(i + 1 for i in range(286) if ll[i])), 286)
        hdist = rng.randint(max([1] + [i + 1 for i in range(30) if dl[i]]), 30)
        seq = ll[:hlit] + dl[:hdist]
        plan = rle_plan(seq, rng) if rng.random() < 0.6 else [(l, 0) for l in seq]
        used = sorted({s for s, _ in plan} | set(rng.sample(range(19), rng.randint(0, 3))))
        if len(used) < 2:
            used = sorted(set(used) | {0, 18})
        cl = lens_of(zip(used, random_tree(rng, len(used), 7, rng.random())), 19)
        df.dynamic(ll, dl, toks, final=b == nblocks - 1, plan=plan, hlit=hlit, hdist=hdist, cl=cl)
        if sync and b < nblocks - 1:
            df.stored(b"")
            unit0 = len(df.out)
    info = dict(sync=sync, lit_max=max(df.lit_used), dist_max=max(df.dist_used, default=0), lit_used=set(df.lit_used),
                dist_used=set(df.dist_used), mod16=len(df.out) % 16, blocks=nblocks)
    return df, info


@functools.lru_cache(maxsize=None)
def seeded():
    """[(name, Case, info)]: the first SEEDED streams from SEED0 on that give more than one byte."""
    out, seed = [], SEED0
    while len(out) < SEEDED:
        df, info = seeded_stream(seed)
        if len(df.out) >= 2:
            name = f"seed_{seed}"
            out.append((name, _row(name, df, tags=["seeded"]), info))
        seed += 1
    return out


# ---- the row limit -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def limit_rowmax():
    """[Case]: the widest rows of one and of four channels (49152 and 49149 bytes of ATTWARP_PNGDEC_MAX_ROW_BYTES), 65 rows, a full flush between the rows: 65 units, 64 kept sync
    points behind the stream's start."""
    c = []
    for name, (H, W, ch) in (("rowmax_c1", (65, 49151, 1)), ("rowmax_c4", (65, 12287, 4))):
        img = PC.photo(H, W, ch, 3 + ch)
        f = C.filtered_cycle(img, 1)
        rb = 1 + W * ch
        assert rb <= D.MAX_ROW_BYTES < rb + ch                # (no wider image of ch channels is decoded)
        co = zlib.compressobj(6)
        s = b"".join(co.compress(f[r * rb:(r + 1) * rb]) + (co.flush(zlib.Z_FULL_FLUSH) if r < H - 1 else b"") for r in range(H)) + co.flush()
        flushes = H - 1
        assert s.count(MARKER) == flushes
        c.append(Case(name, make_png(W, H, ch, s), ["rowmax"], f, route="unit", chain=flushes + 1, nkept=flushes + 1, image=img))
    return c


@functools.lru_cache(maxsize=None)
def good_cases():
    """[Case] of every good limit file but the two row-limit ones."""
    c = (_code_cases() + _repeat_cases() + _match_cases() + _stored_cases() + _reach_cases() + _scan_cases() + _chunk_cases() +
         _carry_cases() + [k for _, k, _ in seeded()])
    assert len({k.name for k in c}) == len(c)
    return c


def limit_good():
    """[(name, file, features)]; features: the tags of what the builder knows it wrote, the case's own name among them."""
    return [(k.name, k.file, k.features) for k in good_cases()]


def case(name):
    return next(k for k in good_cases() + (limit_rowmax() if name.startswith("rowmax") else []) if k.name == name)


def filtered_of(name):
    return case(name).filtered


def scan_kept():
    """{name: the kept positions, written out by the builder} of every scan case, the two truncated ones included."""
    out = {k.name: k.expect["kept"] for k in good_cases() if "kept" in k.expect}
    out.update(SCAN_TRUNC_KEPT)
    return out


# ---- malformed -----------------------------------------------------------------------------------------------------------------
SCAN_TRUNC_KEPT = {"scan_trunc_plus1": [2, 60], "scan_trunc_plus0": [2]}
TAIL = b"\x00" * 8 + b"\x00\x00\x00\x01"


def _m(stream, W=63, H=1, ch=1):
    return make_png(W, H, ch, stream)


def _aligned_cut(make, eb):
    """The bytes of make(k) (k literals of nine bits in front) for the first k that leaves fewer than eb bits in the last byte."""
    for k in range(8):
        df = make(k)
        if (-df.w.bitpos) % 8 < eb:
            return b"\x78\x01" + df.bytes()
    raise AssertionError


@functools.lru_cache(maxsize=None)
def limit_malformed():
    """[(name, file, status)]: the status the restatement gives (None: whatever the serial route finds)."""
    E = D
    c = []
    z = lambda n: (18, n - 11) if n >= 11 else (17, n - 3)
    two = lens_of([(0, 1), (256, 1)], 286)
    hdr = lambda **kw: b"\x78\x01" + Deflate().dynamic(kw.pop("ll", two), kw.pop("dl", [1]), kw.pop("toks", None), final=True, **kw).bytes() + TAIL
    c.append(("rep_past_total", _m(hdr(plan=[(2, 0)] * 3 + [z(138), z(118)], hlit=257, hdist=1)), E.E_CODE_LENGTHS))
    c.append(("rep16_first", _m(hdr(plan=[(16, 0), (2, 0)])), E.E_CODE_LENGTHS))
    for n in (287, 288):
        c.append((f"hlit{n}", _m(hdr(hlit=n)), E.E_CODE_LENGTHS))
    for n in (31, 32):
        c.append((f"hdist{n}", _m(hdr(hdist=n)), E.E_CODE_LENGTHS))
    c.append(("no_eob", _m(hdr(ll=lens_of([(i, 2) for i in range(4)], 286), hlit=257, toks=[0, 1, 2, 3], eob=False)), E.E_CODE_LENGTHS))
    c.append(("lit_incomplete", _m(hdr(ll=lens_of([(0, 2), (256, 2)], 286), toks=[0, 0])), E.E_CODE_LENGTHS))
    c.append(("dist_incomplete", _m(hdr(dl=[2, 2], toks=[0, 0])), E.E_CODE_LENGTHS))
    c.append(("hclen4_all_zero", _m(hdr(plan=[], cl=[0] * 19, hclen=4)), E.E_CODE_LENGTHS))
    ll = lens_of([(0, 2), (1, 2), (256, 2), (257, 2)], 286)
    c.append(("single_dist_other_bit", _m(hdr(ll=ll, dl=[1], toks=[0, 1, 1, ("lit", 257), ("bits", 1, 1), 1, 0])), E.E_SYMBOL))
    c.append(("dist_symbol_30", _m(b"\x78\x01" + Deflate().fixed([0, 7, 7, ("lit", 257), ("dist", 30), 7], final=True).bytes() + TAIL), E.E_SYMBOL))
    c.append(("cut_len_extra", _m(_aligned_cut(lambda k: Deflate().fixed([0] + [200] * k + [("lit", 284)], final=True, eob=False), 5)), E.E_TRUNCATED))
    c.append(("cut_dist_extra", _m(_aligned_cut(lambda k: Deflate().fixed([0, 0] + [200] * k + [("lit", 257), ("dist", 3 + 26)], final=True, eob=False), 13)), E.E_TRUNCATED))
    full = Deflate().dynamic(two, [1], [0] * 64, final=True, hclen=19).bytes()
    c.append(("cut_code_lengths", _m(b"\x78\x01" + full[:5]), E.E_TRUNCATED))
    c.append(("cut_stored_header", _m(b"\x78\x01\x01\x40\x00"), E.E_TRUNCATED))
    c.append(("cut_stored_payload", _m(b"\x78\x01\x01\x40\x00\xbf\xff" + b"\x00" + filler(39, 7)), E.E_TRUNCATED))
    row = [0] + list(filler(63, 8))
    whole = Deflate().fixed(row, final=True).stream()
    for j in range(4):
        c.append((f"adler_short_{j}", _m(whole[:len(whole) - 4 + j]), E.E_TRUNCATED))
    c.append(("overflow_by_match", _m(Deflate().fixed(row[:61] + [(4, 1)], final=True).stream()), E.E_OVERFLOW))
    c.append(("overflow_by_stored", _m(Deflate().stored(bytes(row) + b"\x01", final=True).stream()), E.E_OVERFLOW))
    s = bytearray(C.photo_streams()["full_flush"])
    at = s.index(MARKER) + 4
    for pos in range(at + 8, len(s) - 4):
        t = bytes(s[:pos]) + bytes([s[pos] ^ 0x10]) + bytes(s[pos + 1:])
        try:
            zlib.decompress(t)
        except zlib.error:
            break
    assert t.count(MARKER) == 1
    c.append(("broken_second_unit", make_png(53, 37, 3, t), None))
    img = PC.noise(129, 7, 3, 88)
    for name, r in (("filter5_row64", 64), ("filter5_row0_of_h129", 0)):
        f = bytearray(C.filtered_cycle(img))
        f[r * 22] = 5
        c.append((name, make_png(7, 129, 3, zlib.compress(bytes(f), 6)), E.E_FILTER))
    _, s = _rgba_stream()
    first = s[:257]
    for name, i in (("crc_flip_first", 0), ("crc_flip_last", 256)):
        bad = first[:i] + bytes([first[i] ^ 0x04]) + first[i + 1:]
        c.append((name, make_png(9, 70, 4, [(chunk(b"IDAT", bad, zlib.crc32(b"IDAT" + first)),), s[257:]]), E.E_CRC))
    c.append(("crc_wrong_on_empty_chunk", make_png(9, 70, 4, [s, (chunk(b"IDAT", b"", zlib.crc32(b"IDAT") ^ 1),)]), E.E_CRC))
    # the pattern is candidate 6 of the thread at offset 50, which reads byte by byte (fewer than 12 bytes are left) and
    # splices the pattern's last two bytes in from its third dword
    p = _with_patterns(200, [56], 9)
    full = _stored_row(p)
    c.append(("scan_trunc_plus1", _m(full[:61], W=199), E.E_TRUNCATED))
    c.append(("scan_trunc_plus0", _m(full[:60], W=199), E.E_TRUNCATED))
    for j in range(4):
        t = bytearray(whole)
        t[len(t) - 4 + j] ^= 0x20
        c.append((f"adler_byte{j}", _m(bytes(t)), E.E_ADLER))
    assert len({n for n, _, _ in c}) == len(c)
    return c
