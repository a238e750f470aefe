"""The corpus of the PNG encoder's match="lz" route (attwarp_amd/csrc/png.hip): pages of glyphs and images
built to reach each limit of the token rule of tests/pnglz_ref.py.  A case is (name, image [H,W,C] uint8, filter, order,
match, expect); test_pnglz_ref_cpu.py proves every entry of `expect` from the restatement before test_pnglz_gpu.py runs the
case through the kernels, so a builder that stops reaching its limit fails there.  Deterministic, numpy only, no fonts.

The made-to-order segments use filter "none" on one grey row: the filtered bytes are a zero and the pixels.  Their filler
is ONE repeated byte (distance-1 runs, a single key), so the only keys of the segment are those of the planted patterns and
a planted pattern's candidate is not displaced by a colliding filler position."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import png_cases as K
import png_ref as R
import pnglz_ref as Z

SEG = R.SEG_BYTES
FILL = 7


class Case(NamedTuple):
    name: str
    image: np.ndarray
    filter: str
    order: str
    match: str
    expect: dict


def _rng(seed):
    return np.random.default_rng(9900 + seed)


# ---- pages ---------------------------------------------------------------------------------------------------------------------
def glyph_page(seed, H, W, C):
    """A white page of 40 random 8 x 12 glyphs whose set pixels carry random grey shades 0 .. 199: glyphs 9 pixels apart in
    lines 18 rows apart, each drawn with probability 0.82."""
    rng = _rng(seed)
    glyphs = [np.where(rng.random((12, 8)) < 0.45, rng.integers(0, 200, (12, 8)), 255).astype(np.uint8) for _ in range(40)]
    page = np.full((H, W), 255, np.uint8)
    for y in range(4, H - 12, 18):
        for x in range(4, W - 8, 9):
            if rng.random() < 0.82:
                page[y:y + 12, x:x + 8] = glyphs[int(rng.integers(0, 40))]
    return np.ascontiguousarray(np.repeat(page[:, :, None], C, 2))


# ---- made-to-order segments ------------------------------------------------------------------------------------------------------
def row_image(seg):
    """Filtered bytes of one segment (the first one 0: filter "none") -> the grey one-row image that has them."""
    seg = np.asarray(seg, np.uint8)
    assert seg[0] == 0 and 2 <= seg.size <= SEG
    return np.ascontiguousarray(seg[1:].reshape(1, -1, 1))


def pattern(rng, n, avoid=(FILL,)):
    """n bytes, no two neighbours equal, none of `avoid`."""
    out = []
    while len(out) < n:
        b = int(rng.integers(8, 256))
        if b not in avoid and (not out or out[-1] != b):
            out.append(b)
    return np.array(out, np.uint8)


class Plan:
    """A segment of filler with planted byte strings; nothing is planted twice on the same place."""

    def __init__(self, n):
        self.d = np.full(n, FILL, np.uint8)
        self.d[0] = 0
        self.used = np.zeros(n, bool)
        self.used[0] = True

    def put(self, at, data):
        data = np.asarray(data, np.uint8)
        assert at >= 1 and at + data.size <= self.d.size and not self.used[max(at - 1, 0):at + data.size + 1].any(), at
        self.d[at:at + data.size] = data
        self.used[at:at + data.size] = True

    def pair(self, rng, src, dst, n, ends=(1, 2)):
        """The same n bytes at src and at dst, each followed by a different byte, so the match is n long exactly."""
        p = pattern(rng, n, (FILL,) + ends)
        self.put(src, np.concatenate([p, [ends[0]]]))
        self.put(dst, np.concatenate([p, [ends[1]]]))


def far_lengths():
    """Far matches of 4, 5 and 258 bytes and a repeated string of 3, which is no match (FAR_MIN = 4)."""
    rng, pl = _rng(1), Plan(2600)
    pl.pair(rng, 10, 512, 3)
    pl.pair(rng, 20, 768, 4)
    pl.pair(rng, 30, 1024, 5)
    pl.pair(rng, 1300, 2304, 258, ends=(3, 4))
    return pl.d, {"matches": [(4, 748), (5, 994), (258, 1004)], "no_far_length": 3, "route": Z.ROUTE_LZ}


def segment_end_cut():
    """A match that the segment's last byte cuts: 40 planted bytes, the first 9 of them again at the very end."""
    rng, pl = _rng(2), Plan(777)
    p = pattern(rng, 40)
    pl.put(100, p)
    pl.d[768:777] = p[:9]
    return pl.d, {"matches": [(9, 668)], "last_token_ends_at_n": True}


def max_distance(n):
    """The largest distance a segment of n bytes allows: its first four bytes again as its last four (distance n - 4); the
    60 bytes before them repeat an early string, so the LZ block is the shorter one."""
    rng, pl = _rng(3), Plan(n)
    p = pattern(rng, 3)
    pl.d[1:4] = p
    pl.used[1:5] = True
    pl.d[4] = 1
    q = pattern(rng, 200)
    pl.put(600, q)
    pl.put(n - 4 - 201, np.concatenate([q, [2]]))
    pl.d[n - 4] = 0
    pl.d[n - 3:n] = p
    return pl.d, {"matches": [(4, n - 4)], "max_dist_symbol": 28, "route": Z.ROUTE_LZ}


def all_distance_symbols():
    """Every distance symbol a segment can hold (0 .. 28; symbol 29 starts at 24,577, beyond any position), each at its base
    and at base + 2^extra - 1 (symbol 28: at the largest distance that leaves room for the match)."""
    rng, pl = _rng(4), Plan(SEG)
    want, L = [], 12
    dists = sorted({d for s in range(1, 29) for d in (Z.DIST_BASE[s], Z.DIST_BASE[s] + (1 << Z.DIST_EXTRA[s]) - 1)})
    dists = [min(d, SEG - 600) for d in dists]
    at = 256
    for d in dists:                   # the copy at a block start (near ones), its source d bytes before it
        dst = max(at, -(-(d + 1) // 256) * 256)
        while pl.used[dst - 1:dst + L + 2].any() or pl.used[dst - d - 1:dst - d + L + 2].any():
            dst += 256 if d < 256 else 32       # (from distance 256 on any position sees the source: it lies in an earlier block)
        if d <= 16:                   # source and copy overlap: d different bytes, repeated up to L bytes behind the block start
            period = rng.permutation(np.arange(100, 250))[:d].astype(np.uint8)
            pl.put(dst - d, np.concatenate([np.tile(period, 2 + L // d)[:d + L], [1]]))
        else:
            pl.pair(rng, dst - d, dst, L, ends=(1, 2))
        want.append((L, d))
        at = dst + 256 if d < 256 else at
    return pl.d, {"distances": [d for _, d in want], "dist_symbols": list(range(29)), "route": Z.ROUTE_LZ}


def perms(copies):
    """A zero and the same 255 different bytes once, twice (the second copy is one match of 255 at distance 255, symbol 15)
    or three times, the third behind two more zeros: the second zero, at 512, and the copy behind it repeat the segment's
    first 256 bytes at distance 512 (symbol 17).  One copy: no distance at all."""
    p = _rng(5).permutation(np.arange(1, 256)).astype(np.uint8)
    return np.concatenate([[0], p] + [[p], [p, [0, 0], p]][copies - 2] if copies > 1 else [[0], p]).astype(np.uint8)


def overlap(period):
    """Content of period 2 or 3: position 256 matches 258 bytes at distance `period`, the two overlapping."""
    vals = np.array([11, 22, 33][:period], np.uint8)
    d = np.tile(vals, 400)[:780].copy()
    d[0] = 0
    return d


def tie_run_far():
    """A far match of 5 ends on the first 50 of a run; at position 517 four more 50s follow (distance 1, length 4) and the
    candidate, the four 50s at 301, also matches 4: distance 1 wins."""
    pl = Plan(700)
    pl.put(100, [60, 61, 62, 63, 50, 1])
    pl.put(300, [9, 50, 50, 50, 50, 8, 1])
    pl.put(512, [60, 61, 62, 63, 50, 50, 50, 50, 50, 5, 2])
    return pl.d


def two_far():
    """Two earlier strings with the key of position 1024: the nearer one (shorter match) is the candidate, the farther and
    longer one is never looked at."""
    rng, pl = _rng(6), Plan(1300)
    p = pattern(rng, 30)
    pl.put(100, np.concatenate([p, [1]]))
    pl.put(600, np.concatenate([p[:6], [2]]))
    pl.put(1024, np.concatenate([p, [3]]))
    return pl.d, {"matches": [(6, 424)], "no_match": (30, 924)}


def colliding_keys():
    """Two different keys with one hash: the candidate exists, the match is 0 bytes long, the position is a literal."""
    rng = _rng(7)
    a = pattern(rng, 4)
    ha = int(Z.hashes(bytes(a))[0])
    while True:
        b = pattern(rng, 4)
        if int(Z.hashes(bytes(b))[0]) == ha and b[0] != a[0]:
            break
    pl = Plan(600)
    pl.put(100, np.concatenate([a, [1]]))
    pl.put(512, np.concatenate([b, [2]]))
    return pl.d, {"candidate": (512, 100), "literal_at": 512}


def twins():
    """Two rows of one segment each with the same content: the second segment never refers to the first."""
    rng = _rng(8)
    row = np.tile(np.concatenate([pattern(rng, 300), np.full(100, FILL, np.uint8)]), 31)[:12399]
    return np.ascontiguousarray(np.stack([row, row]).reshape(2, -1, 1))


def three_routes():
    """Segments of 40 rows: glyphs (LZ), noise (stored), a soft ramp (RLE), glyphs again."""
    rng = _rng(9)
    page = glyph_page(10, 160, 600, 1)[:, :, 0]
    noise = rng.integers(0, 256, (80, 600)).astype(np.uint8)
    ramp = (np.add.outer(np.arange(80), np.arange(600)) // 7 + rng.integers(0, 2, (80, 600))).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([page[:80], noise, ramp, page[80:]])[:, :, None])


# ---- distance histograms as deep as the code-length limiter's limit ----------------------------------------------------------------------
DIST_SYMBOL = [0] + [Z.dist_symbol(k)[0] for k in range(1, SEG + 1)]


def vocabulary(rng, V=128):
    """V words of four bytes (x, m1, m2, m3), x different per word, m1 .. m3 shared.  Whatever the order of the words, a
    segment built of them has four keys per word -- (x m1 m2 m3) and the three that straddle into the next word, which
    depend on that word's x alone -- and no word's key shares its hash with any other of them: a word's candidate is always
    its own latest occurrence in an earlier block."""
    while True:
        m = [int(v) for v in rng.permutation(np.arange(200, 256))[:3]]

        def h(b):
            return int(Z.hashes(bytes(b))[0])
        xs, own, span = [], set(), set()
        for x in rng.permutation(np.arange(8, 200)):
            x = int(x)
            h0 = h([x] + m)
            hs = {h([m[0], m[1], m[2], x]), h([m[1], m[2], x, m[0]]), h([m[2], x, m[0], m[1]])}
            if h0 in own or h0 in span or h0 in hs or hs & own:
                continue
            xs.append(x)
            own.add(h0)
            span |= hs
            if len(xs) == V:
                return xs, m


@functools.lru_cache(maxsize=None)
def deep_distances(nsym, nblocks, seed=0):
    """A segment whose LZ tokens have a distance histogram with Fibonacci counts 1, 1, 2, 3, 5, ... over `nsym` symbols (the
    two largest classes take the surplus), so its Huffman tree is nsym - 1 deep: 17 symbols need the 15-bit limiter, 16 are
    exactly 15 deep without it.  Layout: a zero, 255 different bytes, a dictionary of 128 words (:func:`vocabulary`; two
    256-byte blocks), then `nblocks` blocks of 64 words.  Every word there is one match of 4 bytes (the next word differs
    from the one behind its source) at distance position - latest occurrence in an earlier block; the words are dealt slot by
    slot so that each distance symbol gets its count: the far symbols (the small counts) from words left unused for many
    blocks, symbols 12 .. 17 from the previous block's words.  -> the segment's bytes."""
    rng = np.random.default_rng(seed)
    far = [28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18][17 - nsym:]
    order = far + [12, 13, 17, 14, 15, 16]
    assert len(order) == nsym
    f = [1, 1]
    while len(f) < nsym:
        f.append(f[-1] + f[-2])
    need = dict(zip(order, f))
    tol = {s: 0 for s in order}
    tol[17], tol[14], tol[15], tol[16] = 10, 20, 10 ** 6, 10 ** 6
    xs, m = vocabulary(np.random.default_rng(seed))
    V = len(xs)
    seq = [(256 + 4 * w, w) for w in range(V)]                # the dictionary
    pos = 256 + 4 * V
    last = {w: p for p, w in seq}                            # the word's latest occurrence in a finished block
    nxt = {seq[k][0]: seq[k + 1][1] for k in range(V - 1)}   # position of a word -> the word behind it
    got = {s: 0 for s in order}
    prev_src = None                                          # the source of the previous token
    for B in range(nblocks):
        state = (dict(got), len(seq), prev_src)
        for attempt in range(200):
            used, block, added, ok = set(), [], [], True
            for j in range(64):
                p = pos + 4 * j
                best = None
                for w in rng.permutation(V):
                    w = int(w)
                    if w in used or (prev_src is not None and nxt.get(prev_src) == w):
                        continue
                    s = DIST_SYMBOL[p - last[w]]
                    if s not in need or got[s] >= need[s] + tol[s]:
                        continue
                    short = got[s] < need[s]                 # far symbols first, then the emptiest near one, surplus to 16 and 15
                    rank = (0 if (s >= 18 and short) else 1 if short else 2,
                            -s if s >= 18 else got[s] / need[s] if short else {16: 0, 15: 1}.get(s, 2))
                    if best is None or rank < best[0]:
                        best = (rank, w, s)
                if best is None:
                    ok = False
                    break
                _, w, s = best
                got[s] += 1
                used.add(w)
                block.append((p, w))
                nxt[seq[-1][0]] = w
                added.append(seq[-1][0])
                prev_src = last[w]
                seq.append((p, w))
            if ok:
                break
            got, prev_src = dict(state[0]), state[2]         # a dead end: this block again, in another random order
            del seq[state[1]:]
            for q in added:
                del nxt[q]
        else:
            raise AssertionError("deep_distances: no arrangement found")
        for p, w in block:
            last[w] = p
        pos += 256
    assert all(got[s] >= need[s] for s in order), got
    d = np.zeros(pos, np.uint8)
    d[1:256] = np.arange(1, 256)
    for p, w in seq:
        d[p:p + 4] = [xs[w]] + m
    return d


def overlay_like(H, W, seed):
    """A photo-like image under a half-transparent Jet-like heat map of a smooth bump, as the drivers' `_masked.png`."""
    yy, xx = np.mgrid[0:H, 0:W]
    v = np.exp(-(((yy - H * 0.4) / (H * 0.3)) ** 2 + ((xx - W * 0.6) / (W * 0.25)) ** 2))
    jet = np.stack([np.clip(1.5 - np.abs(4 * v - 3), 0, 1), np.clip(1.5 - np.abs(4 * v - 2), 0, 1), np.clip(1.5 - np.abs(4 * v - 1), 0, 1)], -1)
    return (0.5 * K.photo(H, W, 3, seed) + 0.5 * 255 * jet).astype(np.uint8)



@functools.lru_cache(maxsize=None)
def size_decision():
    """One planted string of 64 bytes, copied with k of its bytes: the LZ block's advantage grows with k.  -> {difference
    RLE bytes - LZ bytes: segment} for the differences 0 (a tie: RLE) and 1 (LZ by one byte)."""
    found = {}
    for seed in range(40):
        rng = _rng(100 + seed)
        p = pattern(rng, 64)
        for k in range(4, 64):
            pl = Plan(600)
            pl.put(100, np.concatenate([p, [1]]))
            pl.put(512, np.concatenate([p[:k], [2]]))
            info = []
            Z.encode_segment(pl.d.tobytes(), info)
            diff = info[0]["sizes"][0] - info[0]["sizes"][1]
            if diff in (0, 1) and diff not in found and any(t[0] == "match" and t[2] > 1 for t in info[0]["tokens"]):
                found[diff] = pl.d
        if len(found) == 2:
            return found
    raise AssertionError("size_decision: no tie / one-byte case found")


TAILS = ((1, "rgb", [12, 13, 17, 23, 24, 36]), (3, "rgb", [1, 2, 5, 7, 8, 12]), (3, "bgr", [3, 6, 8]))


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, image, filt="none", order="rgb", match="lz", **expect):
        image = np.ascontiguousarray(image)
        assert image.dtype == np.uint8 and image.ndim == 3
        out.append(Case(name, image, filt, order, match, expect))

    small = glyph_page(11, 60, 200, 1)
    add("small_first", small, "sub", has_lz=True)
    add("glyph_grey", glyph_page(1, 500, 600, 1), "sub", has_lz=True, ratio=0.80)
    add("glyph_rgb", glyph_page(2, 400, 300, 3), "sub", has_lz=True, ratio=0.80)
    add("glyph_grey_as_rle", glyph_page(1, 500, 600, 1), "sub", match="rle")
    for filt, order in (("paeth", "rgb"), ("adaptive", "rgb"), ("sub", "bgr"), ("paeth", "bgr"), ("adaptive", "bgr")):
        img = glyph_page(3, 90, 150, 3)
        img[:, :, 1] //= 2                                  # (three different channels: the order matters)
        img[:, :, 2] = 255 - img[:, :, 2]
        add(f"glyph_{filt}_{order}", img, filt, order, has_lz=True)
    d, e = far_lengths()
    add("far_lengths", row_image(d), **e)
    d, e = segment_end_cut()
    add("segment_end_cut", row_image(d), **e)
    d, e = max_distance(SEG)
    add("max_distance_grey", row_image(d), **e)
    d, e = max_distance(SEG - 2)                            # 8191 RGB pixels: rows of 24,574 bytes
    add("max_distance_rgb", d[1:].reshape(1, -1, 3), **e)
    d, e = all_distance_symbols()
    add("all_distance_symbols", row_image(d), **e)
    add("distances_none", row_image(perms(1)), dist_used=0, no_lz=True)
    add("distances_one", row_image(perms(2)), dist_used=1, matches=[(255, 255)], route=Z.ROUTE_LZ)
    add("distances_two", row_image(perms(3)), dist_used=2, matches=[(255, 255), (256, 512)], route=Z.ROUTE_LZ)
    add("overlap_period_2", row_image(overlap(2)), matches=[(258, 2)], route=Z.ROUTE_LZ)
    add("overlap_period_3", row_image(overlap(3)), matches=[(258, 3)], route=Z.ROUTE_LZ)
    add("tie_run_far", row_image(tie_run_far()), token_at=(517, ("match", 4, 1)), candidate=(517, 301), matches=[(5, 412)])
    d, e = two_far()
    add("two_far_candidates", row_image(d), **e)
    d, e = colliding_keys()
    add("colliding_keys", row_image(d), **e)
    for w in (1, 2, 3):                                     # segments of 2, 3 and 4 bytes: shorter than, and just, one key
        add(f"short_{w}", np.full((1, w, 1), 200, np.uint8), no_lz=True)
    add("short_rows", np.full((5, 1, 1), 9, np.uint8), "sub", no_lz=True)
    add("twins", twins(), segments_equal=(0, 1), route=Z.ROUTE_LZ)
    add("small_middle", small, "sub", has_lz=True)
    sd = size_decision()
    add("size_tie", row_image(sd[0]), size_diff=0, route=Z.ROUTE_RLE)
    add("size_lz_by_one", row_image(sd[1]), size_diff=1, route=Z.ROUTE_LZ)
    add("noise", _rng(12).integers(0, 256, (40, 300, 3)).astype(np.uint8), "sub", routes={Z.ROUTE_STORED})
    add("three_routes", three_routes(), "sub", routes={Z.ROUTE_RLE, Z.ROUTE_LZ, Z.ROUTE_STORED})
    add("photo", K.photo(120, 160, 3, 4), "sub", no_lz=True)
    add("photo_paeth", K.photo(90, 100, 1, 5), "paeth", no_lz=True)
    add("flat", np.full((70, 500, 3), 128, np.uint8), "sub", no_lz=True)
    add("overlay", overlay_like(120, 160, 6), "sub", no_lz=True)
    add("distance_limiter", row_image(deep_distances(17, 70)), dist_used=17, dist_depth=16, dist_limited=True, route=Z.ROUTE_LZ)
    add("distance_depth_15", row_image(deep_distances(16, 52)), dist_used=16, dist_depth=15, dist_limited=False, max_dist_code=15,
        route=Z.ROUTE_LZ)
    for C, order, widths in TAILS:
        for i, W in enumerate(widths):
            rb = 1 + W * C                                  # rows that repeat every fourth row, 700 filtered bytes or more
            img = np.tile(_rng(20 + W + C).integers(0, 4, (4, W, C)) * 60, (max(10, 700 // (4 * rb) + 1), 1, 1)).astype(np.uint8)
            add(f"tail_{C}_{order}_{W}", img, ("sub", "paeth", "adaptive")[i % 3], order, odd_placement=i % 2 == 0)
    add("small_last", small, "sub", has_lz=True)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (file, [route per segment], [info per segment]) of the restatement; "rle" cases are png_ref's file."""
    c = case(name)
    if c.match == "rle":
        f = R.encode(c.image, c.filter, c.order)
        facts = [0 if seg[0] else 2 for seg in segment_bytes(f, c)]
        return f, facts, None
    info = []
    f, routes = Z.encode(c.image, c.filter, c.order, info)
    return f, routes, info


def segment_bytes(f, c):
    """The deflate bytes of every segment of an "rle" file of png_ref (re-encoded segment by segment)."""
    fs = R.filtered_stream(c.image, c.filter, c.order)
    return [R.encode_segment(fs[r0:r0 + nr].tobytes()) for r0, nr in R.segments(*fs.shape)]


def guard_batch():
    """A sub-batch whose files put segments at every address residue mod 4 (test_pnglz_gpu.py checks that)."""
    return ["small_first", "tail_1_rgb_13", "far_lengths", "tail_3_rgb_5", "three_routes", "tail_3_bgr_3", "distances_two", "short_2",
            "distance_limiter"]
