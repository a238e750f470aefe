"""The PNG encoder's restatement (tests/png_ref.py) against independent judges, without a GPU: Pillow decodes every
file, zlib inflates every stream to an independently written filter's output, the CRC / Adler combine steps equal zlib's,
and the stream stays within two points of zlib's own Z_RLE level-1 encoder (plus the fixed cost per segment)."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases as K
import png_ref as R

CASES = K.cases()
IDS = [c[0] for c in CASES]


def spec_filter(a, ftypes):
    """The specification's formulas on the whole image: a [H,W,C] uint8, one filter type per row -> [H, 1 + W C] bytes."""
    H, W, C = a.shape
    x = np.zeros((H + 1, W * C + C), np.int64)
    x[1:, C:] = a.reshape(H, W * C)
    cur, left, up, ul = x[1:, C:], x[1:, :-C], x[:-1, C:], x[:-1, :-C]
    p = left + up - ul
    pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    pred = np.stack([np.zeros_like(cur), left, up, (left + up) // 2, paeth])[np.asarray(ftypes), np.arange(H)]
    return np.concatenate([np.asarray(ftypes, np.uint8)[:, None], ((cur - pred) % 256).astype(np.uint8)], 1)


def file_order(img, order):
    return img[:, :, ::-1] if order == "bgr" and img.shape[2] == 3 else img


@pytest.mark.parametrize("name,img,filt,order", CASES, ids=IDS)
def test_file_decodes_inflates_and_stays_small(name, img, filt, order):
    png = K.reference(name, filt, order)
    want = file_order(img, order)
    got = np.asarray(Image.open(io.BytesIO(png)))
    assert np.array_equal(got.reshape(want.shape), want)
    assert len(png) <= R.bound(*img.shape)
    z = R.idat_payload(png)
    raw = zlib.decompress(z)
    H, W, C = img.shape
    stream = np.frombuffer(raw, np.uint8).reshape(H, 1 + W * C)
    ftypes = stream[:, 0]
    if filt != "adaptive":
        assert (ftypes == R.FILTERS[filt]).all()
    assert np.array_equal(stream, spec_filter(want, ftypes))
    if filt == "adaptive":                                   # each row took the cheapest filter, ties to the lower number
        for r in range(H):
            cost = [int(np.abs(spec_filter(want, np.full(H, t))[r, 1:].view(np.int8).astype(np.int64)).sum()) for t in range(5)]
            assert ftypes[r] == int(np.argmin(cost)), (r, cost)
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    rle = c.compress(raw) + c.flush()
    nseg = len(R.segments(H, 1 + W * C))
    print(f"{name}: {len(z)} bytes, zlib Z_RLE level 1 {len(rle)}, ratio {len(z) / len(rle):.4f}, {nseg} segment(s)")
    assert len(z) <= 1.02 * len(rle) + 192 * nseg + 16


def test_adaptive_case_uses_several_filters():
    img = K.adaptive_image()
    assert len(set(R.filtered_stream(img, "adaptive")[:, 0].tolist())) >= 3


def test_crc_and_adler_combine_equal_zlib():
    rng = np.random.default_rng(9)
    for n in (0, 1, 2, 255, 256, 257, 1000, 24581):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert R.crc32(d) == zlib.crc32(d)
        assert R.crc32_sliced(d) == zlib.crc32(d)
        for cut in (0, n // 3, n):
            assert R.crc32_combine(zlib.crc32(d[:cut]), zlib.crc32(d[cut:]), n - cut) == zlib.crc32(d)
            parts = [R.adler_partial(p) for p in (d[:cut], d[cut:cut + 7], d[cut + 7:])]
            assert R.adler_combine(parts) == zlib.adler32(d)
    assert R.xpow8(0) == 0x80000000 and R.crc32_combine(0x12345678, 0, 0) == 0x12345678


def test_length_limit_case_needs_the_limiter():
    img = K.fibonacci_image()
    hist = R.histogram(R.tokens(R.filtered_stream(img, "none").tobytes()))
    assert sorted(h for h in hist[1:256] if h)[-1] == 1597 and sum(1 for h in hist if h) >= 17
    assert max(R.huffman_depths(hist)) > 15                  # the unlimited tree is too deep ...
    lens = R.code_lengths(hist)
    assert max(lens) <= 15                                   # ... the limited one is not, and is still a complete code
    assert sum(2.0 ** -l for l in lens if l) == 1.0


def test_token_rule_at_the_run_lengths():
    for n in K.RUN_LENGTHS:
        toks = R.tokens(bytes([5]) * n)
        assert toks[0] == ("lit", 5)
        assert sum(1 if k == "lit" else v for k, v in toks) == n
        assert all(3 <= v <= 258 for k, v in toks if k == "len")
        r = n - 1
        assert [v for k, v in toks if k == "len"] == [258] * (r // 258) + ([r % 258] if r % 258 >= 3 else [])


def test_stored_fallback_and_single_symbol_blocks():
    z = R.idat_payload(K.reference("noise_stored", "sub", "rgb"))
    assert z[2] == 0x00                                      # a stored block follows the zlib header
    img = next(i for n, i, f, o in CASES if n == "single_symbol")
    lens = R.code_lengths(R.histogram(R.tokens(R.filtered_stream(img, "none").tobytes())))
    assert [(s, l) for s, l in enumerate(lens) if l] == [(0, 1), (256, 1)]      # one literal and the end of block


def test_limits():
    with pytest.raises(ValueError):
        R.encode(np.zeros((2, R.MAX_ROW_BYTES, 1), np.uint8))
    assert len(R.encode(np.zeros((2, R.MAX_ROW_BYTES - 1, 1), np.uint8))) <= R.bound(2, R.MAX_ROW_BYTES - 1, 1)


def test_planner_matches_the_restatement():
    """attwarp_png_bound / attwarp_png_plan on the host (no launch): segments, bound, IHDR chunk and the CRC tables."""
    import ctypes
    import struct
    from attwarp_amd import _lib
    lib = _lib.load()
    shapes = [(1, 1, 1), (1, 1, 3), (500, 500, 3), (97, 85, 3), (193, 85, 3), (2, R.MAX_ROW_BYTES - 1, 1), (1500, 1, 1), (3000, 7, 3)]
    for H, W, C in shapes:
        assert lib.attwarp_png_bound(H, W, C) == R.bound(H, W, C)
    for bad in [(2, R.MAX_ROW_BYTES, 1), (2, 8192, 3), (0, 5, 3), (5, 0, 3), (5, 5, 2), (5, 5, 4)]:
        assert lib.attwarp_png_bound(*bad) == 0
    rec = (_lib.PngImage * len(shapes))()
    for r, (H, W, C) in zip(rec, shapes):
        r.src, r.H, r.W, r.C, r.pitch, r.order, r.filter = 0x1000, H, W, C, W * C + 3, _lib.BGR, _lib.PNG_FILTER_IDS["paeth"]
    n = lib.attwarp_png_table_bytes(rec, len(shapes))
    assert n > 0
    table = np.zeros(n, np.uint8)
    _lib.call("attwarp_png_plan", rec, len(shapes), table.ctypes.data, n)
    h = _lib.PngHeader.from_address(table.ctypes.data)
    segs = [s for H, W, C in shapes for s in R.segments(H, 1 + W * C)]
    assert (h.B, h.nseg, h.table_bytes) == (len(shapes), len(segs), n)
    assert h.out_bytes == sum(R.bound(*s) for s in shapes)
    assert list(h.crc_pow8) == R.CRC_POW8 and h.idat_head_crc == zlib.crc32(b"IDAT\x78\x01")
    seg_dt = np.dtype([("image", "<i4"), ("row0", "<i4"), ("nrows", "<i4"), ("n", "<i4"), ("scratch_off", "<u8"), ("after", "<u8")])
    got = table[h.off_segs:h.off_segs + len(segs) * seg_dt.itemsize].view(seg_dt)
    k = 0
    for b, (H, W, C) in enumerate(shapes):
        rb = 1 + W * C
        img = table[h.off_images + 80 * b:h.off_images + 80 * (b + 1)].tobytes()
        assert img[48:73] == R.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0 if C == 1 else 2, 0, 0, 0))
        for r0, nr in R.segments(H, rb):
            g = got[k]
            assert (g["image"], g["row0"], g["nrows"], g["n"], g["after"]) == (b, r0, nr, nr * rb, (H - r0 - nr) * rb)
            assert g["scratch_off"] % 16 == 0 and (k == 0 or g["scratch_off"] >= got[k - 1]["scratch_off"] + got[k - 1]["n"] + 8)
            k += 1
    assert h.scratch_bytes >= got[-1]["scratch_off"] + got[-1]["n"] + 8 and got[0]["scratch_off"] >= 24 * len(segs)
    rec[0].pitch = 0                                          # a pitch below the row
    assert lib.attwarp_png_table_bytes(rec, len(shapes)) == 0
