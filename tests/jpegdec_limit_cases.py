"""Files that put the JPEG decoder at its size, ring, scan and segment limits (test_jpegdec_limits_ref_cpu.py,
test_jpegdec_limits_gpu.py, and the two host programs): narrow and extremely long images from Pillow's writer, hand-written
grey streams with tables of their own whose blocks are as long as a block can be, restart files whose markers sit at chosen
offsets, and marker-less files whose data ends on, next to or far in front of a segment boundary.  Every builder is cached:
a module builds its files once.  test_jpegdec_limits_ref_cpu.py proves, from the bytes, that each file has the property its
name promises."""
from __future__ import annotations

import functools

import numpy as np

import jpegdec_cases as C
import jpegdec_ref as D
import jpegdec_sync_cases as SC

# ---- 1. geometry: Pillow is the judge -------------------------------------------------------------------------------------------
NARROW_W = tuple(range(1, 9))
NARROW_H = (1, 2, 3, 4, 5, 9, 17, 40)
NARROW_GREY_W = (1, 3, 4)


@functools.lru_cache(maxsize=None)
def narrow():
    """Noise at quality 90 at every width 1..8, every sampling: the widths at which a chroma plane has one or two columns
    (replicated, not filtered) and the first at which it has three."""
    out, seed = [], 0
    for W in NARROW_W:
        for H in NARROW_H:
            for sub in (0, 1, 2):
                out.append((f"narrow_{W}x{H}_s{sub}", C.write(C.noise(W, H, 3, seed), quality=90, subsampling=sub)))
                seed += 1
            if W in NARROW_GREY_W:
                out.append((f"narrow_{W}x{H}_grey", C.write(C.noise(W, H, 1, seed), quality=90)))
                seed += 1
    return out


@functools.lru_cache(maxsize=None)
def extreme():
    """The longest images libjpeg's writer makes (65500), in either direction."""
    return [
        ("wide_65500x1_s2", C.write(C.noise(65500, 1, 3, 1), quality=50, subsampling=2)),
        ("tall_1x65500_s2", C.write(C.noise(1, 65500, 3, 2), quality=50, subsampling=2)),
        ("tall_1x65500_s2_ri", C.write(C.noise(1, 65500, 3, 3), quality=50, subsampling=2, restart_marker_rows=1)),   # 4094 units
        ("wide_65500x2_s1", C.write(C.noise(65500, 2, 3, 4), quality=50, subsampling=1)),
    ]


# ---- 2. hand-written streams: one code of every length, so the longest code has 16 bits --------------------------------------------
DC_LONG = ([1] * 16, list(range(16)))                      # '0' -> category 0, ..., FFFE -> category 15
AC_LONG = ([1] * 16, list(range(16)))                      # '0' -> EOB, ..., FFFE -> run 0, size 15
SHORT_BLOCK = ((0, 0), (0, 0))                                 # category 0 and EOB: two bits


def long_block(values):
    """64 values of 15 bits each (as written: the top bit set is a positive coefficient): 64 x 31 bits = 248 data bytes."""
    assert len(values) == 64 and all(0 <= v < 1 << 15 for v in values)
    return tuple((15, v) for v in values)


def _codes(counts, symbols):
    return {sym: (code, l) for (l, code), sym in D.code_table(counts, symbols).items()}


def encode(blocks, dc, ac, ri=0):
    """Blocks of a grey file, each ((DC category, value bits), (AC run << 4 | size, value bits), ...) -> (the entropy data,
    restart markers included, EOI not; the raw (start, end) of every block: its first byte, and the byte behind its last
    with that one's stuffed 00)."""
    dcc, acc = _codes(*dc), _codes(*ac)
    units = [blocks[i:i + ri] for i in range(0, len(blocks), ri)] if ri else [blocks]
    out, spans = bytearray(), []
    for u, unit in enumerate(units):
        w, marks = C.BitWriter(), []
        for blk in unit:
            a = len(w.bits)
            w.put(*dcc[blk[0][0]])
            w.put(blk[0][1], blk[0][0])
            for rs, v in blk[1:]:
                w.put(*acc[rs])
                w.put(v, rs & 15)
            marks.append((a, len(w.bits)))
        raw = w.bytes()
        offs, i = [], 0
        while i < len(raw):
            offs.append(i)
            i += 2 if raw[i] == 0xFF else 1
        offs.append(len(raw))
        spans += [(len(out) + offs[a >> 3], len(out) + offs[(b + 7) >> 3]) for a, b in marks]
        out += raw
        if u + 1 < len(units):
            out += bytes([0xFF, 0xD0 + (u & 7)])
    return bytes(out), spans


ALL_ONES = long_block([0x7FFF] * 64)                       # 432 raw bytes after stuffing


def _long_blocks(name):
    if name == "long_8":
        return [ALL_ONES] * 8, 1, 0
    if name == "long_mixed_12":                              # every third block has two bits: long blocks begin at other phases
        return [SHORT_BLOCK if i % 3 == 2 else ALL_ONES for i in range(12)], 1, 0
    if name == "long_ri5_12":                                # units of 5, 5 and 2 blocks: two longer than the ring, one short
        return [ALL_ONES] * 10 + [SHORT_BLOCK, ALL_ONES], 1, 5
    assert name == "long_random"
    r = np.random.RandomState(41)                            # seeded values of either sign; one block stays the longest there is
    return [ALL_ONES if i == 5 else long_block([int(v) for v in r.randint(0, 1 << 15, 64)]) for i in range(8)], 255, 0


LONG_NAMES = ("long_8", "long_mixed_12", "long_ri5_12", "long_random")


@functools.lru_cache(maxsize=None)
def long_streams():
    """{name: (file, block spans, restart interval)}."""
    out = {}
    for name in LONG_NAMES:
        blocks, q, ri = _long_blocks(name)
        data, spans = encode(blocks, DC_LONG, AC_LONG, ri)
        out[name] = (C.hand_file(8 * len(blocks), 8, data, DC_LONG, AC_LONG, q, ri), spans, ri)
    return out


@functools.lru_cache(maxsize=None)
def long_files():
    return [(n, long_streams()[n][0]) for n in LONG_NAMES]


@functools.lru_cache(maxsize=None)
def long_cuts():
    """long_8 cut in the middle of its second block and ten bytes into its fifth; nothing behind the cut."""
    blocks, q, _ = _long_blocks("long_8")
    data, spans = encode(blocks, DC_LONG, AC_LONG)
    cuts = (("long_8_cut_1_5", C._safe(data, (spans[1][0] + spans[1][1]) // 2)), ("long_8_cut_4_10", C._safe(data, spans[4][0] + 10)))
    return [(n, C.hand_file(64, 8, data[:at], DC_LONG, AC_LONG, q, eoi=b"")) for n, at in cuts]


# ---- 3. restart markers at chosen offsets -----------------------------------------------------------------------------------------
def scan_offsets(s):
    """(offsets of the FF of every restart marker in front of the data's end, offset of the FF that ends the data or None)."""
    rst, i = [], 0
    while i < len(s):
        if s[i] == 0xFF:
            nx = s[i + 1] if i + 1 < len(s) else None
            if nx == 0 or (nx is not None and 0xD0 <= nx <= 0xD7):
                if nx:
                    rst.append(i)
                i += 2
                continue
            return rst, i
        i += 1
    return rst, None


def restart_file(mcux, mcuy, lead=0, fill=0, seed=0):
    """A grey file of mcux x mcuy blocks with DRI 1.  Every block is "DC category 15, EOB" in the tiny tables: 18 bits, three
    bytes, none of them FF, so the markers are five bytes apart; `lead` bytes the decoder never reaches stand behind the first
    unit's block, so the first marker's FF is at 3 + lead; `fill` FF bytes stand in front of the EOI."""
    r = np.random.RandomState(seed)
    out = bytearray()
    n = mcux * mcuy
    for u in range(n):
        v = int(r.randint(0, 1 << 15))
        if (v >> 1) & 0xFF == 0xFF:                            # (the middle byte)
            v ^= 2
        w = C.BitWriter()
        w.put(0b10, 2)
        w.put(v, 15)
        w.put(0, 1)
        b = w.bytes()
        assert len(b) == 3 and 0xFF not in b
        out += b
        if u == 0:
            out += b"\x55" * lead
        if u + 1 < n:
            out += bytes([0xFF, 0xD0 + (u & 7)])
    return C.hand_file(8 * mcux, 8 * mcuy, bytes(out), ri=1, eoi=b"\xff" * fill + b"\xff\xd9")


RST_AT_2047, RST_AT_2048 = ("rst_ff_2047", 408), ("rst_ff_2048", 409)       # (name, which marker)


@functools.lru_cache(maxsize=None)
def restart_files():
    return [
        (RST_AT_2047[0], restart_file(42, 10, lead=4, seed=1)),         # 7 + 5 * 408 = 2047
        (RST_AT_2048[0], restart_file(42, 10, lead=0, seed=2)),         # 3 + 5 * 409 = 2048
        ("eoi_ff_2047", restart_file(409, 1, lead=4, seed=3)),          # 7 + 5 * 408
        ("eoi_ff_2048", restart_file(41, 10, lead=0, seed=4)),          # 3 + 5 * 409
        ("rst_1230_units", restart_file(41, 30, lead=1, seed=5)),
        ("fill_1", restart_file(5, 4, fill=1, seed=6)),
        ("fill_3000", restart_file(5, 4, fill=3000, seed=7)),
    ]


@functools.lru_cache(maxsize=None)
def restart_damaged():
    """The marker on the tile boundary removed, doubled and given the next index, and one fill byte in front of a restart
    marker (which ends the data for this decoder: E_RESTART, where libjpeg skips the fill byte and decodes)."""
    by = dict(restart_files())
    out = []
    for name, which in (RST_AT_2047, RST_AT_2048):
        out += [(f"{name}_{mode}", C._drop_rst(by[name], which, mode)) for mode in ("missing", "extra", "index")]
    segs, tail = C.split(by["fill_1"])
    at = scan_offsets(tail)[0][7]
    out.append(("fill_before_rst", C.join(segs, tail[:at] + b"\xff" + tail[at:])))
    return out


# ---- 4. sub-stream boundaries and the cap ---------------------------------------------------------------------------------------
END_SEEDS = (0, 600)
END_RESIDUES = (0, 1, 31)


@functools.lru_cache(maxsize=None)
def data_ends():
    """Three marker-less noise files whose data ends (the EOI's offset) at 0, 1 and 31 modulo 32."""
    found = {}
    for seed in range(*END_SEEDS):
        f = C.write(C.noise(24, 16, 3, seed), quality=75, subsampling=seed % 3)
        r = (len(D.parse(f)["stream"]) - 2) % 32
        if r in END_RESIDUES and r not in found:
            found[r] = (f"end_mod32_{r}", f)
            if len(found) == len(END_RESIDUES):
                return [found[r] for r in END_RESIDUES]
    raise AssertionError("no file for every residue found")


BEHIND = (1, 32, 101)


@functools.lru_cache(maxsize=None)
def behind_end():
    """The file whose data ends on a boundary with 1, 32 and 101 bytes behind its EOI: whole segments behind the data."""
    name, f = data_ends()[0]
    junk = (b"\xff\xd0\x00\x00\xff\x00" + bytes(26) + b"\xff\xd1\xff\x00" + bytes(65))[:101]
    return [(f"{name}_plus_{k}", f + junk[:k]) for k in BEHIND]


def padded(f, stream_len):
    """f with zeros behind its EOI up to `stream_len` bytes behind the SOS header."""
    n = len(D.parse(f)["stream"])
    assert n <= stream_len
    return f + bytes(stream_len - n)


@functools.lru_cache(maxsize=None)
def smallest_plans():
    """(name, file, segment_bytes, planned segments): the shortest stream that is planned, and one byte less."""
    f = SC.good_file(SC.SHORT)
    return [("short_64", padded(f, 64), 32, 2), ("short_63", padded(f, 63), 32, 0),
            ("short_1024", padded(f, 1024), 512, 2), ("short_1023", padded(f, 1023), 512, 0)]


CAP_SEGMENTS, CAP_BYTES = 1 << 14, 32


@functools.lru_cache(maxsize=None)
def cap_files():
    """One picture just under the cap of 16384 segments of 32 bytes, padded behind its EOI to the cap exactly and to one
    byte more."""
    f = C.write(C.smooth_detail(1300, 940), quality=95, subsampling=0)
    return [("cap_16384", padded(f, CAP_SEGMENTS * CAP_BYTES)), ("cap_16384_plus_1", padded(f, CAP_SEGMENTS * CAP_BYTES + 1))]
