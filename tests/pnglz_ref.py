"""Plain numpy / Python restatement of the PNG encoder's second token route, match="lz" (attwarp_amd/csrc/png.hip,
png_lz_blocks.hpp), on top of png_ref: the kernel must produce the same bytes.

File layout, filters, segment geometry and the stored form are png_ref's.  Per segment three forms are sized and the
shortest is written, ties to the earlier one: png_ref's block (RLE, route 0), the LZ block (route 1), one stored block
(route 2).  The LZ tokens of a segment d[0 .. N):

  key(i)   the four bytes at i as a little-endian word, for every i with i + 4 <= N;  hash = (key * HASH_MUL mod 2^32) >> 20
  cand(i)  the LARGEST j with hash(j) == hash(i) among the positions of EARLIER 256-position blocks (j < i - i % 256);
           one candidate per position, none for the first block and for the last three positions
  far(i)   the common prefix of d[i ..] and d[cand(i) ..], at most min(258, N - i) (the two may overlap); it counts from
           FAR_MIN = 4 bytes (colliding hashes with other bytes give less and count as nothing)
  run(i)   how often d[i - 1] repeats from i on, at most min(258, N - i); it counts from 3 bytes, as in png_ref
  token    far(i) > run(i): a match of far(i) at distance i - cand(i); else run(i) >= 3: a match at distance 1; else the
           literal d[i].  Equal lengths go to distance 1; of two far candidates only the nearer block's is ever looked at.
  parse    greedy from position 0: the next token starts where this one ends.

Nothing reaches over the segment's first or last byte, so distances are at most N - 4 <= 24,572."""
from __future__ import annotations

import struct

import numpy as np

import png_ref as R

HASH_MUL = 0x9E3779B1
HASH_BITS = 12
BLOCK = 256
FAR_MIN = 4
MAX_LEN = 258
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + (286 + 30) * 4
ROUTE_RLE, ROUTE_LZ, ROUTE_STORED = 0, 1, 2

DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def dist_symbol(d):
    """distance 1 .. 32768 -> (symbol, extra bits, extra value), from RFC 1951's table."""
    for k in range(29, -1, -1):
        if d >= DIST_BASE[k]:
            return k, DIST_EXTRA[k], d - DIST_BASE[k]
    raise ValueError(d)


def hashes(d):
    """hash of every position i with i + 4 <= N (uint32 array of N - 3 entries, empty below 4 bytes)."""
    d = np.frombuffer(bytes(d), np.uint8).astype(np.uint64)
    if d.size < 4:
        return np.zeros(0, np.int64)
    key = d[:-3] | d[1:-2] << np.uint64(8) | d[2:-1] << np.uint64(16) | d[3:] << np.uint64(24)
    return (((key * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)).astype(np.int64)


def candidates(d):
    """cand(i) for every position (-1: none)."""
    n = len(d)
    h = hashes(d)
    cand = np.full(n, -1, np.int64)
    head = np.full(1 << HASH_BITS, -1, np.int64)
    for b0 in range(0, h.size, BLOCK):
        idx = np.arange(b0, min(b0 + BLOCK, h.size))
        cand[idx] = head[h[idx]]
        np.maximum.at(head, h[idx], idx)
    return cand


def common_prefix(d, i, c, cap):
    k = 0
    while k < cap and d[i + k] == d[c + k]:
        k += 1
    return k


def token_at(d, cand, i):
    """The token that starts at i: ('lit', value) or ('match', length, distance)."""
    n = len(d)
    cap = min(MAX_LEN, n - i)
    run = common_prefix(d, i, i - 1, cap) if i else 0
    far = common_prefix(d, i, int(cand[i]), cap) if cand[i] >= 0 else 0
    if far >= FAR_MIN and far > run:
        return ("match", far, i - int(cand[i]))
    if run >= 3:
        return ("match", run, 1)
    return ("lit", d[i])


def tokens(data):
    d = bytes(data)
    cand = candidates(d)
    out, i = [], 0
    while i < len(d):
        t = token_at(d, cand, i)
        out.append(t)
        i += t[1] if t[0] == "match" else 1
    return out


def histograms(toks):
    hl, hd = [0] * 286, [0] * 30
    for t in toks:
        if t[0] == "lit":
            hl[t[1]] += 1
        else:
            hl[R.length_symbol(t[1])[0]] += 1
            hd[dist_symbol(t[2])[0]] += 1
    hl[256] += 1
    return hl, hd


def dist_lengths(hd):
    """Code lengths of the 30 distance symbols: png_ref's builder and limiter; with no used symbol symbol 0, with one
    used symbol that one, gets the single 1-bit code."""
    used = [s for s, f in enumerate(hd) if f]
    if len(used) < 2:
        lens = [0] * 30
        lens[used[0] if used else 0] = 1
        return lens
    return R.code_lengths(hd)


def lz_block(data):
    """-> (bits of the dynamic block, a function that writes the segment's bytes)."""
    toks = tokens(data)
    hl, hd = histograms(toks)
    ll, dl = R.code_lengths(hl), dist_lengths(hd)
    bits = HEADER_BITS + sum(h * l for h, l in zip(hl, ll)) + sum(hl[257 + k] * R.LEN_EXTRA[k] for k in range(29))
    bits += sum(h * (l + e) for h, l, e in zip(hd, dl, DIST_EXTRA))

    def write():
        lc, dc = R.canonical_codes(ll), R.canonical_codes(dl)
        w = R.BitWriter()
        w.put(4, 3)                       # BFINAL = 0, BTYPE = 10
        w.put(29, 5)                      # HLIT = 286
        w.put(29, 5)                      # HDIST = 30
        w.put(15, 4)                      # HCLEN = 19
        for s in R.CL_ORDER:
            w.put(4 if s < 16 else 0, 3)
        for l in ll + dl:
            w.put(R._rev4(l), 4)
        assert w.n == HEADER_BITS
        for t in toks:
            if t[0] == "lit":
                w.put(lc[t[1]], ll[t[1]])
            else:
                s, eb, ev = R.length_symbol(t[1])
                w.put(lc[s], ll[s])
                w.put(ev, eb)
                s, eb, ev = dist_symbol(t[2])
                w.put(dc[s], dl[s])
                w.put(ev, eb)
        w.put(lc[256], ll[256])
        assert w.n == bits
        w.put(0, 3)
        return w.to_bytes() + b"\x00\x00\xff\xff"
    return bits, write, toks


def rle_bytes(data):
    """Size of png_ref's dynamic form of the segment (whether or not png_ref would store it)."""
    hist = R.histogram(R.tokens(data))
    lens = R.code_lengths(hist)
    bits = R.HEADER_BITS + sum(h * l for h, l in zip(hist, lens)) + sum(hist[257 + k] * (R.LEN_EXTRA[k] + 1) for k in range(29))
    return (bits + 3 + 7) // 8 + 4


def encode_segment(data, info=None):
    """One segment's filtered bytes -> (its deflate bytes, route)."""
    data = bytes(data)
    n = len(data)
    bits, write, toks = lz_block(data)
    sizes = [rle_bytes(data), (bits + 3 + 7) // 8 + 4, n + 5]
    route = sizes.index(min(sizes))       # (the first of equal sizes: RLE, LZ, stored)
    if info is not None:
        info.append({"route": route, "sizes": sizes, "tokens": toks, "n": n})
    if route == ROUTE_RLE:
        out = R.encode_segment(data)
    elif route == ROUTE_LZ:
        out = write()
    else:
        out = b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + data
    assert len(out) == sizes[route]
    return out, route


def encode(image, filt="sub", order="rgb", info=None):
    """uint8 [H,W] / [H,W,1] / [H,W,3] -> (the PNG file's bytes, [route per segment]).  ``info``: a list that receives one
    dict per segment (route, the three sizes, the LZ tokens)."""
    a = R._as_hwc(image, order)
    H, W, C = a.shape
    filtered = R.filtered_stream(a, filt)
    parts, body, routes = [], [], []
    for r0, nr in R.segments(H, 1 + W * C):
        d = filtered[r0:r0 + nr].tobytes()
        parts.append(R.adler_partial(d))
        seg, route = encode_segment(d, info)
        body.append(seg)
        routes.append(route)
    z = b"\x78\x01" + b"".join(body) + b"\x01\x00\x00\xff\xff" + struct.pack(">I", R.adler_combine(parts))
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 0 if C == 1 else 2, 0, 0, 0)
    out = b"\x89PNG\r\n\x1a\n" + R.chunk(b"IHDR", ihdr) + R.chunk(b"IDAT", z) + R.chunk(b"IEND", b"")
    assert len(out) <= R.bound(H, W, C)
    return out, routes
