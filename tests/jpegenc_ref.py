"""numpy restatement of the JPEG encoder (attwarp_amd/csrc/jpegenc.hip, jpegenc_blocks.hpp): the bytes of
``Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s, restart_marker_rows=r)`` from T.81 and the IJG library's
published integer arithmetic.  No Pillow in here; tests/test_jpegenc_ref_cpu.py proves it against Pillow, the GPU tests
prove the kernels against it.

Steps: (1) colour in 16-bit fixed point, (2) edges: input replicated to the right and down to a multiple of the vertical
factor, DOWN-SAMPLED rows replicated below that (``early=True`` is the wrong order, kept to show that the cases tell them
apart), (3) h2v2 / h2v1 down-sampling with the alternating bias, (4) jfdctint's islow DCT, (5) quantisation by q << 3 with
rounding half away from zero, (6) interleaved MCUs with dummy blocks, (7) Huffman coding with the Annex K tables, byte
stuffing, restart markers, and the file layout.

``encode`` joins an interval's bits as one string; ``assemble_by_units`` / ``assemble_batch`` (at the end) put the same file
together unit by unit the way launches 3 .. 7 do, and take one seeded ``defect`` (tests/test_jpegenc_limits_ref_cpu.py).
"""
import numpy as np

UNIT_MCUS = 16                        # MCUs one entropy unit of the device encoder holds at most (JE_UNIT_MCUS)
MAX_DIM = 65500
SUBSAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
SUBSAMPLING_IDS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}

STD_LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
STD_CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                         47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])          # natural index of zigzag position k

# Annex K.3: BITS (codes of length 1 .. 16) and VALS
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
TABLES = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)            # in the order of the DHT segments: class / id 00 10 01 11


def huffman_codes(bits, vals):
    """T.81 Annex C: symbol -> (code, length)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


CODES = [huffman_codes(*t) for t in TABLES]


def quant_tables(quality):
    """jpeg_quality_scaling + jpeg_add_quant_table with force_baseline: natural order, luma and chroma."""
    if not 1 <= quality <= 100:
        raise ValueError(f"quality {quality} (1 .. 100)")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_LUMA_Q, STD_CHROMA_Q)]


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def geometry(H, W, ncomp, sub):
    hmax, vmax = SUBSAMPLINGS[sub] if ncomp == 3 else (1, 1)
    return hmax, vmax, -(-W // (8 * hmax)), -(-H // (8 * vmax))


def planes(img, sub, early=False):
    """[H,W] / [H,W,1] / [H,W,3] (RGB) uint8 -> the component planes, padded to whole MCUs by the edge rule."""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    H, W, C = a.shape
    hmax, vmax, mx, my = geometry(H, W, C, sub)
    yy = np.minimum(np.arange(my * 8 * vmax), H - 1)
    xx = np.minimum(np.arange(mx * 8 * hmax), W - 1)
    if C == 1:
        return [a[:, :, 0].astype(np.int64)[yy][:, xx]]
    y, cb, cr = ycc(a)
    out = [y[yy][:, xx]]
    r = np.arange(my * 8)
    rc = r if early else np.minimum(r, -(-H // vmax) - 1)      # down-sampled rows below the last real one repeat IT
    c = np.arange(mx * 8)
    rows = [np.minimum(rc * vmax + k, H - 1) for k in range(vmax)]
    cols = [np.minimum(c * hmax + k, W - 1) for k in range(hmax)]
    for p in (cb, cr):
        if (hmax, vmax) == (1, 1):
            out.append(p[rows[0]][:, cols[0]])
        elif (hmax, vmax) == (2, 1):
            out.append((p[rows[0]][:, cols[0]] + p[rows[0]][:, cols[1]] + (c & 1)[None, :]) >> 1)
        else:
            s = p[rows[0]][:, cols[0]] + p[rows[0]][:, cols[1]] + p[rows[1]][:, cols[0]] + p[rows[1]][:, cols[1]]
            out.append((s + 1 + (c & 1)[None, :]) >> 2)
    return out


def fdct(blocks):
    """jfdctint.c (islow) on [n,8,8] samples with 128 already subtracted -> [n,8,8] coefficients, scaled by 8."""
    F = dict(a=2446, b=3196, c=4433, d=6270, e=7373, f=9633, g=12299, h=15137, i=16069, j=16819, k=20995, l=25172)

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    def one(d, first):
        t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
        t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        n = 11 if first else 15
        o = [None] * 8
        o[0] = (t10 + t11) * 4 if first else descale(t10 + t11, 2)
        o[4] = (t10 - t11) * 4 if first else descale(t10 - t11, 2)
        z1 = (t12 + t13) * F["c"]
        o[2] = descale(z1 + t13 * F["d"], n)
        o[6] = descale(z1 - t12 * F["h"], n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * F["f"]
        t4, t5, t6, t7 = t4 * F["a"], t5 * F["j"], t6 * F["l"], t7 * F["g"]
        z1, z2, z3, z4 = -z1 * F["e"], -z2 * F["k"], -z3 * F["i"] + z5, -z4 * F["b"] + z5
        o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
        return o
    b = np.asarray(blocks, np.int64)
    rows = np.stack(one([b[:, :, k] for k in range(8)], True), axis=2)           # along each row
    out = np.stack(one([rows[:, k, :] for k in range(8)], False), axis=1)        # down each column
    assert np.abs(out).max(initial=0) < 1 << 31
    return out


def quantize(coef, q):
    """[n,8,8] coefficients (scaled by 8), q [64] natural -> rounded half away from zero."""
    div = (q.reshape(8, 8) << 3)[None]
    mag = (np.abs(coef) + (div >> 1)) // div
    return np.where(coef < 0, -mag, mag)


def scan_blocks(img, quality, sub, early=False):
    """The blocks of the scan in order: (component, table id, [64] zigzag coefficients), dummy blocks included."""
    a = np.asarray(img)
    ncomp = 1 if a.ndim == 2 else a.shape[2]
    H, W = a.shape[:2]
    hmax, vmax, mx, my = geometry(H, W, ncomp, sub)
    qt = quant_tables(quality)
    comps = []
    for ci, p in enumerate(planes(a, sub, early)):
        hb, wb = p.shape[0] // 8, p.shape[1] // 8
        blk = p.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8) - 128
        z = quantize(fdct(blk), qt[min(ci, 1)]).reshape(hb, wb, 64)[:, :, ZIGZAG]
        comps.append(z)
    real_w, real_h = -(-W // 8), -(-H // 8)
    out = []
    for m in range(mx * my):
        r, c = divmod(m, mx)
        mcu = []
        for by in range(vmax):
            for bx in range(hmax):
                row, col = r * vmax + by, c * hmax + bx
                if row < real_h and col < real_w:
                    mcu.append((0, 0, comps[0][row, col]))
                else:                                          # a dummy block: no AC, the DC of the block before it
                    src = mcu[-1] if row < real_h else mcu[by * hmax - 1]
                    z = np.zeros(64, np.int64)
                    z[0] = src[2][0]
                    mcu.append((0, 0, z))
        for ci in range(1, ncomp):
            mcu.append((ci, 1, comps[ci][r, c]))
        out.append(mcu)
    return out, (hmax, vmax, mx, my)


def _size(v):
    return int(abs(int(v))).bit_length()


def _low(v, n):
    v = int(v)
    return format((v if v >= 0 else v - 1) & ((1 << n) - 1), f"0{n}b") if n else ""


def block_bits(z, pred, tid, used=None):
    """One block's bits as a string of 0 / 1; ``used``: a set that collects (table index, symbol)."""
    dc, ac = CODES[2 * tid], CODES[2 * tid + 1]
    d = int(z[0]) - pred
    n = _size(d)
    if used is not None:
        used.add((2 * tid, n))
    s = [format(dc[n][0], f"0{dc[n][1]}b"), _low(d, n)]
    run = 0
    for k in range(1, 64):
        v = int(z[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            s.append(format(ac[0xf0][0], f"0{ac[0xf0][1]}b"))
            run -= 16
            if used is not None:
                used.add((2 * tid + 1, 0xf0))
        n = _size(v)
        sym = run << 4 | n
        if used is not None:
            used.add((2 * tid + 1, sym))
        s.append(format(ac[sym][0], f"0{ac[sym][1]}b") + _low(v, n))
        run = 0
    if run:
        s.append(format(ac[0][0], f"0{ac[0][1]}b"))
        if used is not None:
            used.add((2 * tid + 1, 0))
    return "".join(s)


def header(H, W, ncomp, quality, sub, interval):
    qt = quant_tables(quality)
    hmax, vmax = SUBSAMPLINGS[sub] if ncomp == 3 else (1, 1)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2 if ncomp == 3 else 1):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(v) for v in qt[t][ZIGZAG])
    out += b"\xff\xc0" + (8 + 3 * ncomp).to_bytes(2, "big") + b"\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        out += bytes([c + 1, (hmax << 4 | vmax) if c == 0 else 0x11, min(c, 1)])
    for t in range(4 if ncomp == 3 else 2):
        bits, vals = TABLES[t]
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([(t & 1) << 4 | t >> 1]) + bytes(bits) + bytes(vals)
    if interval:
        out += b"\xff\xdd\x00\x04" + interval.to_bytes(2, "big")
    out += b"\xff\xda" + (6 + 2 * ncomp).to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        out += bytes([c + 1, 0x11 * min(c, 1)])
    return bytes(out + b"\x00\x3f\x00")


def block_bound_bits(quality, ncomp):
    """Bits one block takes at most: the DC (a code of at most 11 bits and 11 low bits), and per AC position a symbol of at
    most 16 bits and the largest category its quantiser leaves: coefficients are below 1024 + 2 before division (T.81: 11
    bits for 8-bit samples, and the islow DCT's rounding), so a value is at most (1026 + q / 2) / q."""
    worst = 0
    for q in quant_tables(quality)[:2 if ncomp == 3 else 1]:
        worst = max(worst, 22 + sum(16 + int((1026 + (int(v) >> 1)) // int(v)).bit_length() for v in q[1:]))
    return worst


def bound(H, W, ncomp, quality=75, sub="4:2:0", restart_rows=0):
    """Bytes a file takes at most (attwarp_jpegenc_bound): header, every block at block_bound_bits, every byte stuffed, per
    interval one byte of padding (stuffed) and a marker, EOI."""
    hmax, vmax, mx, my = geometry(H, W, ncomp, sub)
    bpm = hmax * vmax + 2 if ncomp == 3 else 1
    nint = -(-my // restart_rows) if restart_rows else 1
    bits = mx * my * bpm * block_bound_bits(quality, ncomp)
    return len(header(H, W, ncomp, quality, sub, 1 if restart_rows else 0)) + 2 * ((bits + 7) // 8 + nint) + 2 * nint + 2


def encode(img, quality=75, subsampling="4:2:0", restart_rows=0, order="rgb", early=False, info=None):
    """uint8 [H,W] / [H,W,1] / [H,W,3] -> the file's bytes.  ``info``: a dict that receives what the cases' ``expect`` states
    (symbols used, stuffed bytes, unit bit lengths, ...)."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or 0 in a.shape:
        raise ValueError(f"uint8 [H,W] / [H,W,1] / [H,W,3] expected, got {a.dtype} {a.shape}")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"unknown subsampling {subsampling!r}")
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim == 3 and order == "bgr":
        a = a[:, :, ::-1]
    H, W = a.shape[:2]
    if H > MAX_DIM or W > MAX_DIM:
        raise ValueError(f"size {W} x {H} (at most {MAX_DIM})")
    ncomp = 1 if a.ndim == 2 else 3
    mcus, (hmax, vmax, mx, my) = scan_blocks(a, quality, subsampling, early)
    interval = restart_rows * mx
    if interval > 65535:
        raise ValueError(f"restart interval {interval} (at most 65535)")
    used, unit_bits, unit_strings, ff_ends, stuffed = set(), [], [], [], 0
    out = bytearray(header(H, W, ncomp, quality, subsampling, interval))
    head = len(out)
    step = interval or len(mcus)
    raw_ff_straddle = 0
    for i, m0 in enumerate(range(0, len(mcus), step)):
        if i:
            out += bytes([0xff, 0xd0 + (i - 1) % 8])
        pred = [0] * ncomp
        bits, cuts = [], []
        for m in range(m0, min(m0 + step, len(mcus))):
            if (m - m0) % UNIT_MCUS == 0:
                cuts.append(sum(len(b) for b in bits))
            for ci, tid, z in mcus[m]:
                bits.append(block_bits(z, pred[ci], tid, used))
                pred[ci] = int(z[0])
        s = "".join(bits)
        cuts.append(len(s))
        unit_bits += [b - a_ for a_, b in zip(cuts[:-1], cuts[1:])]
        unit_strings += [s[a_:b] for a_, b in zip(cuts[:-1], cuts[1:])]
        s += "1" * (-len(s) % 8)
        data = int(s, 2).to_bytes(len(s) // 8, "big")
        for c in cuts[1:-1]:                                  # an FF byte that holds bits of two units
            if c % 8 and data[c // 8] == 0xff:
                raw_ff_straddle += 1
        stuffed += data.count(b"\xff")
        ff_ends.append(data.endswith(b"\xff"))
        out += data.replace(b"\xff", b"\xff\x00")
    out += b"\xff\xd9"
    if info is not None:
        info.update(symbols=used, unit_bits=unit_bits, stuffed=stuffed, ff_ends=ff_ends, ff_straddle=raw_ff_straddle,
                    header_bytes=head, mcus=len(mcus), intervals=-(-len(mcus) // step), geometry=(hmax, vmax, mx, my),
                    blocks=[z for m in mcus for _, _, z in m], unit_strings=unit_strings, upi=-(-step // UNIT_MCUS))
    return bytes(out)


# ---- the assembly: launches 3 .. 7 of jpegenc.hip restated unit by unit ------------------------------------------------------------
# ``encode`` joins an interval's bits as one string.  The device never has that string: every unit (at most UNIT_MCUS MCUs of
# one interval) has its own, and five launches put the file together from prefix sums.  The functions below compute the file
# THAT way, so that a case can be judged on the CPU for whether it would notice an error in the assembly: ``defect`` seeds
# exactly one.  The defects live in this file only; nothing of the kind is built into or run through the kernels.
SCAN_CHUNK = 256                      # JE_NT: items one round of the three scan kernels takes
UST_POISON, OUT_POISON = 0xA5, 0x5A   # what a byte nobody wrote holds here (the device never zeroes either buffer)
DEFECTS = {
    "bits_carry_dropped": "(a) jpegenc_scan_bits_kernel: units of the second and later chunks get no carry",
    "bytes_carry_dropped": "(a) jpegenc_scan_bytes_kernel: units of the second and later chunks get no carry",
    "files_carry_dropped": "(a) jpegenc_scan_files_kernel: files of the second and later chunks get no carry",
    "interval_in_chunk": "(b) fpos = pre + 2 * ((s - chunk base) // upi): the earlier intervals counted inside the chunk",
    "straddle_one_unit": "(c) the straddling byte: this unit's bits, then the NEXT unit's slot for all the rest; 1-bits only "
                         "where the unit itself is the interval's last (the walk never leaves the one following unit, and "
                         "what lies behind that unit's string are the zeros of its slot)",
    "empty_unit_no_marker": "(d) a last unit that owns no byte writes nothing, its RSTn / EOI included",
    "empty_unit_marker_late": "(d) a last unit that owns no byte places its RSTn / EOI one byte late",
    "upos0_without_interval": "(e) upos0 = base // 8: an interval starts IN the byte the one before it padded",
    "rst_not_modulo": "(f) RSTn = D0 + interval, not modulo 8",
    "row_address_32bit": "(g) the source fetch: y * pitch wrapped to 32 bits (source_rows, not the assembly)",
}


class AssemblyError(Exception):
    """The (defective) assembly left its buffers: a negative offset, or a store or load outside them."""


def _excl_scan(values, drop_carry=False):
    """Exclusive sums the way the scan kernels take them: chunks of SCAN_CHUNK, a carry between them -> (sums, total)."""
    pre, carry = [], 0
    for base in range(0, len(values), SCAN_CHUNK):
        run = 0
        for v in values[base:base + SCAN_CHUNK]:
            pre.append((0 if drop_carry and base else carry) + run)
            run += v
        carry += run
    return pre, carry


def _store(buf, at, data):
    if at < 0 or at + len(data) > len(buf):
        raise AssemblyError(f"store of {len(data)} bytes at {at} of {len(buf)}")
    buf[at:at + len(data)] = data


def unit_plan(img, quality=75, subsampling="4:2:0", restart_rows=0, order="rgb"):
    """What launches 1 and 2 and the planner leave for the assembly: the header, one bit string per unit, the units of a full
    interval, the file's bound; and ``file``, the bytes ``encode`` makes of the same image."""
    info = {}
    data = encode(img, quality, subsampling, restart_rows, order, info=info)
    a = np.asarray(img)
    ncomp = 3 if a.ndim == 3 and a.shape[2] == 3 else 1
    return dict(header=data[:info["header_bytes"]], units=info["unit_strings"], upi=info["upi"], file=data, stuffed=info["stuffed"],
                ff_ends=info["ff_ends"], bound=bound(a.shape[0], a.shape[1], ncomp, quality, subsampling, restart_rows))


def _assemble_image(plan, defect, out, file_off, unit_info):
    """Launches 3, 4, 5 and 7 for one image whose file starts at ``file_off`` of ``out``."""
    units, upi, header = plan["units"], plan["upi"], plan["header"]
    n = len(units)
    nint = -(-n // upi)
    bits = [len(u) for u in units]
    pre, total = _excl_scan(bits, defect == "bits_carry_dropped")                       # 3. scan_bits
    ust = bytearray([UST_POISON]) * ((sum(bits) + 7) // 8 + nint + 8)
    nbytes, nff, upos = [0] * n, [0] * n, [0] * n
    for s in range(n):                                                                  # 4. gather: je_place, then the bytes
        interval = s // upi                                                             # (JeUnit.interval: the host's, not a scan's)
        f = interval * upi
        unit_end = min(f + upi, n)
        last = s == unit_end - 1
        base = pre[f]
        off = pre[s] - base
        end = off + bits[s]
        ibits = (pre[unit_end] if unit_end < n else total) - base
        if off < 0 or ibits < 0:
            raise AssemblyError(f"unit {s}: bit offset {off} of {ibits}")
        upos0 = base // 8 + (0 if defect == "upos0_without_interval" else interval)
        j0 = (off + 7) // 8
        j1 = ((ibits if last else end) + 7) // 8
        if j1 < j0:
            raise AssemblyError(f"unit {s}: owns [{j0}, {j1})")
        full = end // 8
        nfull = max(full - j0, 0)
        if nfull:                                                                       # whole bytes of its own bits, by shift
            q = 8 * j0 - off
            own = int(units[s][q:q + 8 * nfull], 2).to_bytes(nfull, "big")
            _store(ust, upos0 + j0, own)
            nff[s] += own.count(0xff)
        if j1 > j0 + nfull:                                                             # the one straddling byte, bit by bit
            j, v, voff, vend, byte = j1 - 1, s, off, end, 0
            for t in range(8):
                pos = 8 * j + t
                if defect == "straddle_one_unit":
                    if pos >= vend and v == s and s + 1 < unit_end:
                        v, voff, vend = s + 1, vend, vend + bits[s + 1]
                    inside = pos < ibits or not last
                else:
                    while pos >= vend and v + 1 < unit_end:
                        v, voff, vend = v + 1, vend, vend + bits[v + 1]
                    inside = pos < ibits
                bit = 1
                if inside:
                    q = pos - voff
                    if q < 0:
                        raise AssemblyError(f"unit {s}: bit {q} of unit {v}")
                    bit = int(units[v][q]) if q < bits[v] else 0
                byte = byte << 1 | bit
            _store(ust, upos0 + j, bytes([byte]))
            nff[s] += byte == 0xff
        nbytes[s], upos[s] = j1 - j0, upos0 + j0
    sums, total_bytes = _excl_scan([a + b for a, b in zip(nbytes, nff)], defect == "bytes_carry_dropped")       # 5. scan_bytes
    fpos = [p + 2 * ((s % SCAN_CHUNK if defect == "interval_in_chunk" else s) // upi) for s, p in enumerate(sums)]
    for s in range(n):                                                                  # 7. write
        dst = file_off + len(header) + fpos[s]
        if upos[s] + nbytes[s] > len(ust):
            raise AssemblyError(f"unit {s}: load of {nbytes[s]} bytes at {upos[s]} of {len(ust)}")
        _store(out, dst, bytes(ust[upos[s]:upos[s] + nbytes[s]]).replace(b"\xff", b"\xff\x00"))
        if s == 0:
            _store(out, file_off, header)
        if s == min((s // upi + 1) * upi, n) - 1:
            at = dst + nbytes[s] + nff[s]
            if nbytes[s] == 0 and defect == "empty_unit_no_marker":
                continue
            if nbytes[s] == 0 and defect == "empty_unit_marker_late":
                at += 1
            k = s // upi
            _store(out, at, bytes([0xff, 0xd9 if s == n - 1 else (0xd0 + (k if defect == "rst_not_modulo" else k & 7)) & 255]))
    unit_info.append(dict(owned=nbytes, owning_none=sum(b == 0 for b in nbytes), nff=nff, upos=upos, fpos=fpos))
    return len(header) + total_bytes + 2 * (nint - 1) + 2


def assemble_batch(plans, defect=None, info=None):
    """The files of a batch of :func:`unit_plan` s, put together the way launches 3 .. 7 do -> (files, offsets[B + 1]).
    ``defect``: a key of DEFECTS.  ``info``: a list that receives one dict per image: ``owned`` (bytes of the unstuffed stream
    each unit owns), ``owning_none`` (units that own none), ``nff``, ``upos``, ``fpos``.  AssemblyError where the (defective)
    arithmetic leaves the buffers."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")
    out = bytearray([OUT_POISON]) * sum(p["bound"] for p in plans)
    # A file's bytes do not depend on where it lies, so every image is written into a buffer of its own first (at its bound,
    # as `out` is sized) and moved to its offset once launch 6 has run; files that a defect lays over each other are
    # moved in the order of the batch.
    unit_info, lengths, own = [], [], []
    for p in plans:
        own.append(bytearray([OUT_POISON]) * p["bound"])
        lengths.append(_assemble_image(p, defect, own[-1], 0, unit_info))
    offsets, total = _excl_scan(lengths, defect == "files_carry_dropped")                # 6. scan_files
    offsets.append(total)
    for buf, off, n in zip(own, offsets, lengths):
        _store(out, off, buf[:n])
    if info is not None:
        info.extend(unit_info)
    return [bytes(out[a:a + n]) for a, n in zip(offsets, lengths)], offsets


def assemble_by_units(img, quality=75, subsampling="4:2:0", restart_rows=0, order="rgb", defect=None, info=None):
    """:func:`encode`'s file, computed unit by unit the way the device does.  ``info``: a dict that receives ``owned`` and
    ``owning_none`` (see :func:`assemble_batch`) besides the places of every unit."""
    got = []
    files, _ = assemble_batch([unit_plan(img, quality, subsampling, restart_rows, order)], defect, got)
    if info is not None:
        info.update(got[0])
    return files[0]


def source_rows(dense, pitch, defect=None, fill=0):
    """What the transform kernel fetches of an image whose row y starts ``y * pitch`` bytes behind its first pixel:
    ``dense`` itself; with ``defect="row_address_32bit"`` the product taken as an int32, where a byte that belongs to no
    row of the view (in front of it, or in the gap between two rows) reads as ``fill``."""
    a = np.asarray(dense)
    if defect is None:
        return a
    if defect != "row_address_32bit":
        raise ValueError(f"unknown defect {defect!r}")
    flat = a.reshape(a.shape[0], -1)
    H, row = flat.shape
    start = ((np.arange(H, dtype=np.int64) * pitch + (1 << 31)) & 0xffffffff) - (1 << 31)        # as an int32 product
    addr = start[:, None] + np.arange(row, dtype=np.int64)[None, :]
    y, x = addr // pitch, addr % pitch
    ok = (y >= 0) & (y < H) & (x < row)
    return np.where(ok, flat[np.clip(y, 0, H - 1), np.minimum(x, row - 1)], fill).astype(np.uint8).reshape(a.shape)
