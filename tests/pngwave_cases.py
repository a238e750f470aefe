"""Files that put the PNG decoder's wave route at its segment, round, token, match, stored-block and
output limits, built with the token-level writer of tests/pngdec_limit_cases.py.  Every builder knows the filtered bytes its
file decodes to and asserts, from the writer's own bit positions, that the edge it is named after is where it says;
test_pngwave_ref_cpu.py proves the rest from the files' bytes.  Segment edges are those of segment_bytes = 16 unless the
name says otherwise.  Big files hold only the bytes 0 .. 4, so that any split into rows gives valid filter bytes."""
from __future__ import annotations

import functools
import random
import zlib

import pngdec_limit_cases as L
from pngdec_limit_cases import Case, Deflate, make_png

SEG = 128                                    # bits of a 16-byte segment
NAMES = (["short_block", "blocks_70", "eob_ends_segment", "eob_starts_segment", "token48_edges", "windows_2", "windows_3",
          "fixed_then_dynamic"] + [f"empty_stored_at_bit{b}" for b in range(8)] +
         ["out_of_phase_64", "one_bit_literals_256", "matches_only_window", "dist32768_len3_wrap", "dist32768_len258_wrap"] +
         [f"len258_dist{d}_edge" for d in (1, 2, 3)] +
         ["match_chain_64", "match_half_before_window", "reach_first_byte", "stored_65535_then_dist32768", "empty_final_stored"] +
         [f"size_mod16_{r}" for r in range(16)] + ["ring_wraps_twice"])
MALFORMED_NAMES = ["reach_before_first_byte"]


def small(n, seed):
    """n bytes of 0 .. 4, the first 0."""
    rng = random.Random(seed)
    return bytes([0] + [rng.randrange(5) for _ in range(n - 1)])


def _file(name, df, W=None, H=1, tags=(), **expect):
    data = bytes(df.out)
    if W is None:
        W = len(data) - 1
    assert H * (1 + W) == len(data) and 1 + W <= 49152 and all(data[r * (1 + W)] <= 4 for r in range(H)), (name, len(data))
    return Case(name, make_png(W, H, 1, df.stream()), df.tags | set(tags), data, **expect)


def _begin(df, kind, final=False):
    """The header of a fixed block alone -> the bit of its first symbol."""
    assert kind == "fixed"
    df.w.put(int(final), 1)
    df.w.put(1, 2)
    return df.w.bitpos


def _segment_cases():
    c = []
    c.append(_file("short_block", Deflate().fixed([0, 5, 6], final=True)))
    df = Deflate()
    for b in range(70):
        df.fixed([0 if b == 0 else 7] + [10 + (b + i) % 100 for i in range(9)], final=b == 69)
    c.append(_file("blocks_70", df, blocks=70))
    # fixed codes: literals below 144 have 8 bits, those from 144 on 9, the end-of-block code 7
    df = Deflate()
    base = _begin(df, "fixed")
    df.tokens([0] + [20 + i for i in range(13)] + [200], L.FIXED_LIT, L.FIXED_DIST)
    assert df.w.bitpos - base == SEG                       # the end-of-block code's last bit is the segment's last
    df.fixed([1, 2, 3], final=True)
    c.append(_file("eob_ends_segment", df))
    df = Deflate()
    base = _begin(df, "fixed")
    df.tokens([0] + [20 + i for i in range(15)], L.FIXED_LIT, L.FIXED_DIST, eob=False)
    assert df.w.bitpos - base == SEG                       # the end-of-block code's first bit is the next segment's first
    df.tokens([], L.FIXED_LIT, L.FIXED_DIST)
    df.fixed([1, 2, 3], final=True)
    c.append(_file("eob_starts_segment", df))
    # a 48-bit token -- 15-bit length code, 5 extra bits, 15-bit distance code, 13 extra bits -- with a segment edge 7, 17, 27
    # and 40 bits behind its first bit; literal 0 has a 1-bit code and moves the token to any bit
    syms = [0, 1, 2, 3, 4, 256, 5, 6, 7, 8, 9, 10, 11, 12, 13, 284]
    ll = L.lens_of(zip(syms, L.SKEW), 286)
    dsyms = [1, 2, 3, 5, 8, 10, 13, 16, 19, 22, 24, 26, 27, 28, 0, 29]
    dl = L.lens_of(zip(dsyms, L.SKEW), 30)
    assert ll[284] == 15 and dl[29] == 15 and ll[0] == 1
    df = Deflate().stored(small(24700, 11))
    probe = Deflate().dynamic(ll, dl, [], final=True)       # (the header's length: the same in every stream)
    hdr_bits = probe.w.bitpos - ll[256]
    toks, at, edges = [], 0, []
    for k, inside in enumerate((7, 17, 27, 40)):
        start = (2 * k + 1) * SEG - inside
        toks += [0] * (start - at)
        toks.append((227 + 3 * k, 24577 + 11 * k, 284))
        edges.append((start, inside))
        at = start + 48
    toks += [0] * 9
    before = df.w.bitpos
    df.dynamic(ll, dl, toks, final=True)
    first = before + hdr_bits
    assert df.w.bitpos == first + at + 9 + ll[256]
    for start, inside in edges:                                # the edge lies in the code / extra bits it is meant for
        assert start % SEG + inside == SEG and (0 < inside < 15 or 15 < inside < 20 or 20 < inside < 35 or 35 < inside < 48)
    assert [(0 < i < 15, 15 < i < 20, 20 < i < 35, 35 < i < 48) for _, i in edges] == [tuple(j == k for j in range(4)) for k in range(4)]
    c.append(_file("token48_edges", df, tags=["token48"]))
    for name, n in (("windows_2", 1100), ("windows_3", 2200)):   # 8-bit literals: 1024 stream bytes fill a window
        c.append(_file(name, Deflate().fixed([0] + [1 + i % 140 for i in range(n)], final=True), windows=2 if n == 1100 else 3))
    ll2 = L.lens_of([(i, 3) for i in range(7)] + [(256, 3)], 286)
    c.append(_file("fixed_then_dynamic", Deflate().fixed([0, 9, 8, 7]).dynamic(ll2, [0], [1, 2, 3, 4, 5, 6, 6, 5], final=True)))
    rest = list(L.filler(40, 3))
    for b in range(8):
        df = Deflate().fixed([0] + [150 + i for i in range((b - 2) % 8)])
        assert df.w.bitpos % 8 == b
        c.append(_file(f"empty_stored_at_bit{b}", df.stored(b"").fixed(rest, final=True), tags=["empty_stored_between"]))
    return c


def _round_cases():
    # four 2-bit codes: literal 0 is 00.  One literal, one 3-bit match (2-bit length code, 1-bit distance code), then 4060
    # literals 0: the tokens stand on ODD bits from bit 5 on and every bit is 0, so a lane that enters on its segment's first
    # bit decodes literals 0 on EVEN bits for ever and hands the next lane the guess it already has.  Only the true chain
    # moves: segment k is right after k rounds, and the end-of-block code stands in segment 63.
    ll = L.lens_of([(0, 2), (1, 2), (256, 2), (257, 2)], 286)
    df = Deflate()
    m = 4060
    df.dynamic(ll, [1], [0, (3, 1)] + [0] * m, final=True)
    eob_start = 5 + 2 * m
    assert 63 * SEG <= eob_start < 64 * SEG and "single_dist" in df.tags
    return [_file("out_of_phase_64", df, rounds=64, windows=1)]


def _token_cases():
    c = []
    ll = L.lens_of([(0, 1), (256, 1)], 286)
    c.append(_file("one_bit_literals_256", Deflate().dynamic(ll, [0], [0] * 20000, final=True)))
    c.append(_file("matches_only_window", Deflate().fixed([0] + [(4, 1)] * 1500, final=True)))
    return c


def _match_cases():
    c = []
    # the ring wraps at 65536: the match's bytes, and so its source 32768 behind, lie on both sides
    for first, n0, pad in ((3, 65534, 3), (258, 65400, 2)):
        df = Deflate().stored(small(n0, 20 + first)).fixed([(first, 32768)] + [1] * pad, final=True)
        assert n0 < 65536 < n0 + first and len(df.out) % 2 == 0
        c.append(_file(f"dist32768_len{first}_wrap", df, W=len(df.out) // 2 - 1, H=2))
    for d in (1, 2, 3):                                       # 15 literals of 8 bits, then the 13-bit token over bit 128
        df = Deflate()
        base = _begin(df, "fixed", final=True)
        df.tokens([0, 1, 2] + [30 + i for i in range(12)], L.FIXED_LIT, L.FIXED_DIST, eob=False)
        start = df.w.bitpos - base
        df.tokens([(258, d), 9], L.FIXED_LIT, L.FIXED_DIST)
        assert start < SEG < start + 13
        c.append(_file(f"len258_dist{d}_edge", df))
    # 64 periods of 128 bits = one per lane: 13 literals of 8 bits, one of 9, one match (3, 17) of 7 + 5 + 3 bits.  A period
    # makes 17 bytes, so every match copies the match of the period before: resolution rounds = matches = 64
    df = Deflate().stored(small(20, 31))
    base = _begin(df, "fixed", final=True)
    toks = []
    for j in range(64):
        toks += [1 + (j + i) % 100 for i in range(7)] + [(3, 17)] + [2 + (j + i) % 90 for i in range(6)] + [150 + j % 50]
    df.tokens(toks, L.FIXED_LIT, L.FIXED_DIST)
    assert df.w.bitpos - base == 64 * SEG + 7
    c.append(_file("match_chain_64", df, resolution_rounds=64))
    df = Deflate().stored(small(10, 32)).fixed([7, 8, 9, (6, 6), 5], final=True)
    c.append(_file("match_half_before_window", df))
    df = Deflate().fixed([0, 1, 2, 3, 4, (5, 5), 6], final=True)
    c.append(_file("reach_first_byte", df))
    return c


def _stored_cases():
    c = []
    df = Deflate().stored(small(65535, 41)).fixed([(10, 32768)] + [2] * 5, final=True)
    assert len(df.out) == 2 * 32775
    c.append(_file("stored_65535_then_dist32768", df, W=32774, H=2))
    c.append(_file("empty_final_stored", Deflate().fixed([0] + list(L.filler(30, 5))).stored(b"", final=True)))
    return c


def _output_cases():
    c = []
    for r in range(16):
        n = 32 + (r if r else 16)
        c.append(_file(f"size_mod16_{r}", Deflate().fixed([0] + list(L.filler(n - 1, 50 + r)), final=True)))
        assert len(c[-1].filtered) % 16 == r
    data = small(70000, 61)
    assert all(data[r * 35000] <= 4 for r in range(2))
    s = zlib.compress(data, 6)
    c.append(Case("ring_wraps_twice", make_png(34999, 2, 1, s), ["ring_wraps_twice"], data))
    return c


@functools.lru_cache(maxsize=None)
def good_cases():
    c = _segment_cases() + _round_cases() + _token_cases() + _match_cases() + _stored_cases() + _output_cases()
    assert [k.name for k in c] == NAMES
    return c


def good():
    """[(name, file)]"""
    return [(k.name, k.file) for k in good_cases()]


def case(name):
    return next(k for k in good_cases() if k.name == name)


@functools.lru_cache(maxsize=None)
def malformed():
    """[(name, file, status)]: the match of reach_first_byte one byte further (distance 6 behind five bytes)."""
    import pngdec_ref as D
    df = Deflate().fixed([0, 1, 2, 3, 4, ("lit", 259), ("dist", 4), ("bits", 1, 1), 6], final=True)
    good_ = Deflate().fixed([0, 1, 2, 3, 4, ("lit", 259), ("dist", 4), ("bits", 0, 1), 6], final=True)
    assert good_.bytes() == Deflate().fixed([0, 1, 2, 3, 4, (5, 5), 6], final=True).bytes()
    return [("reach_before_first_byte", make_png(10, 1, 1, b"\x78\x01" + df.bytes() + L.TAIL), D.E_DISTANCE)]
