"""The corpus of the JPEG encoder's tests: small named images with their parameters and an ``expect`` that
tests/test_jpegenc_ref_cpu.py proves from the restatement (tests/jpegenc_ref.py) before the GPU test encodes the same cases.
A case is ``(name, image, keywords of R.encode, expect)``; :func:`measure` gives what ``expect`` is compared with."""
import functools
import itertools

import numpy as np

import jpegenc_ref as R

SIZES = ((1, 1), (1, 17), (17, 1), (8, 8), (16, 16), (17, 9), (33, 47), (40, 25), (24, 40), (7, 70))     # (H, W)
LAYOUTS = ("grey", "4:4:4", "4:2:2", "4:2:0")
QUALITIES = (1, 30, 75, 95, 100)
AC_SYMBOLS_USED = (162, 162)         # AC symbols of the luma / chroma table that the corpus codes: all 162 of each


def noise(h, w, c, seed):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)
    return a[:, :, 0] if c == 1 else a


def photo(h, w, c, seed):
    """Photo-like content: smooth gradients, an edge and some grain."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for k in range(c):
        v = 128 + 90 * np.sin((x * (k + 1) + 3 * y) / (7.0 + k)) * np.cos(y / (5.0 + 2 * k)) + 25 * rng.standard_normal((h, w))
        v[h // 3:, w // 2:] += 40 - 30 * k
        chans.append(v)
    a = np.clip(np.stack(chans, 2), 0, 255).astype(np.uint8)
    return a[:, :, 0] if c == 1 else a


def basis(u, v, amp=100, blocks=1):
    """``blocks`` grey 8 x 8 blocks side by side of the DCT basis function (u, v) (u across): after quantisation at quality 50
    only the DC and that coefficient remain."""
    y, x = np.mgrid[0:8, 0:8]
    b = 128 + amp * np.cos((2 * x + 1) * u * np.pi / 16) * np.cos((2 * y + 1) * v * np.pi / 16)
    return np.tile(np.clip(np.rint(b), 0, 255).astype(np.uint8), (1, blocks))


def _zz(k):
    return int(R.ZIGZAG[k]) % 8, int(R.ZIGZAG[k]) // 8          # (u, v) of zigzag position k


# Blocks that between them code every AC symbol of a table: (table, quality) -> (k, p, amplitude at k, amplitude at p), the
# basis function of zigzag position k, on top of a small one at p where p > 0, so that the coefficient at k follows a run of
# k - p - 1 zeros (of k - 1 where p is 0).  An amplitude above 127 is clipped to a squarer wave, which carries the larger
# values.  At quality 100 every divisor is 1, so the values reach category 10 and the small amplitude at p is 0.2 of a grey
# level; at 50 the zeros between are safe from the pixels' rounding.  Found by a search over the restatement and pruned to a
# cover; test_corpus_reaches_what_it_claims proves that with them the corpus codes all 162 symbols of both tables.
SYMBOL_BLOCKS = {
    ("luma", 50): (
        (1,0,46.7,0), (1,0,155.6,0), (2,0,50.9,0), (2,0,169.7,0), (3,0,59.4,0), (3,0,118.8,0), (4,0,36,0), (4,0,72,0),
        (4,0,144,0), (5,0,21.2,0), (5,0,42.4,0), (5,0,169.7,0), (5,1,169.7,1.9), (5,2,169.7,3), (6,0,17,0), (6,0,67.9,0),
        (7,0,42,0), (7,0,84,0), (7,0,168,0), (8,0,19.5,0), (8,0,39,0), (8,0,78,0), (8,0,156,0), (9,0,29.7,0), (9,0,59.4,0),
        (10,0,76.4,0), (10,0,152.7,0), (11,0,25.5,0), (11,0,102,0), (12,0,24,0), (12,0,96,0), (13,0,28.5,0), (13,0,57,0),
        (13,0,114,0), (14,0,25.5,0), (14,0,101.8,0), (15,0,42.4,0), (15,0,84.9,0), (15,0,124.5,0), (16,0,39,0), (16,0,78,0),
        (16,0,156,0), (20,4,169.7,3), (20,5,169.7,1.8)
    ),
    ("luma", 100): (
        (1,0,39.6,0), (1,0,158.4,0), (2,0,33.9,0), (2,0,67.9,0), (2,0,135.8,0), (2,0,158.4,0), (2,1,67.9,0.2), (2,1,135.8,0.2),
        (3,0,33.9,0), (3,0,67.9,0), (4,0,48,0), (4,0,96,0), (4,1,140.8,0.2), (5,0,33.9,0), (5,0,67.9,0), (5,0,158.4,0),
        (5,1,158.4,0.2), (6,0,17,0), (6,0,28.3,0), (7,0,24,0), (7,0,48,0), (7,0,96,0), (7,1,112,0.2), (8,0,24,0), (8,0,48,0),
        (8,0,96,0), (9,0,17,0), (9,0,28.3,0), (9,3,135.8,0.2), (9,3,158.4,0.2), (10,0,17,0), (10,0,33.9,0), (10,0,67.9,0),
        (10,0,135.8,0), (11,0,24,0), (11,0,48,0), (11,0,96,0), (11,4,140.8,0.2), (12,0,24,0), (12,0,48,0), (12,0,96,0),
        (12,1,140.8,0.2), (12,3,112,0.2), (13,0,20,0), (13,0,96,0), (14,0,17,0), (14,0,33.9,0), (14,0,67.9,0), (14,0,135.8,0),
        (14,5,99.6,0.2), (16,0,24,0), (16,0,48,0), (16,0,96,0), (16,0,160,0), (16,1,70.4,0.2), (16,3,140.8,0.2),
        (17,2,35.2,0.2), (19,4,17.6,0.3), (20,12,135.8,0.2), (21,6,135.8,0.2), (23,10,56,0.2), (27,15,158.4,0.2)
    ),
    ("chroma", 50): (
        (1,0,76.4,0), (2,0,76.4,0), (3,0,101.8,0), (3,0,169.7,0), (4,0,63,0), (4,0,126,0), (5,0,50.9,0), (5,0,101.8,0),
        (5,1,169.7,3.2), (6,0,49.9,0), (7,0,78,0), (7,0,156,0), (7,1,156,3.2), (8,0,39,0), (8,0,78,0), (8,0,156,0),
        (9,0,99.7,0), (11,0,99,0), (12,0,84,0), (13,0,99,0), (13,0,145.2,0), (14,0,105,0), (15,0,105,0), (16,0,148.5,0),
        (20,4,154,5.2), (20,5,175,4.2)
    ),
    ("chroma", 100): (
        (1,0,33.9,0), (1,0,158.4,0), (2,0,33.9,0), (2,0,67.9,0), (2,0,135.8,0), (2,0,158.4,0), (2,1,17,0.2), (2,1,67.9,0.2),
        (2,1,135.8,0.2), (3,0,17,0), (3,0,33.9,0), (3,0,67.9,0), (3,1,14.1,0.2), (4,0,24,0), (4,0,48,0), (4,0,96,0),
        (4,1,140.8,0.2), (5,0,17,0), (5,0,33.9,0), (5,0,67.9,0), (5,0,158.4,0), (5,1,158.4,0.2), (6,0,17,0), (6,0,28.3,0),
        (7,0,12,0), (7,0,24,0), (7,0,48,0), (7,0,96,0), (7,1,112,0.2), (8,0,12,0), (8,0,24,0), (8,0,48,0), (8,0,96,0),
        (9,0,17,0), (9,0,28.3,0), (9,3,135.8,0.2), (9,3,158.4,0.2), (10,0,4.2,0), (10,0,8.5,0), (10,0,17,0), (10,0,33.9,0),
        (10,0,67.9,0), (10,0,135.8,0), (11,0,6,0), (11,0,24,0), (11,0,48,0), (11,0,96,0), (11,4,140.8,0.2), (12,0,6,0),
        (12,0,24,0), (12,0,48,0), (12,0,96,0), (12,1,140.8,0.2), (12,3,112,0.2), (13,0,6,0), (13,0,20,0), (13,0,48,0),
        (13,0,96,0), (14,0,4.2,0), (14,0,17,0), (14,0,33.9,0), (14,0,67.9,0), (14,0,135.8,0), (14,5,3.5,0.2), (15,6,158.4,0.2),
        (16,0,6,0), (16,0,12,0), (16,0,24,0), (16,0,48,0), (16,0,96,0), (16,0,160,0), (16,1,6,0.2), (16,1,70.4,0.2),
        (16,3,140.8,0.2), (17,2,35.2,0.2), (18,3,14,0.2), (19,4,17.6,0.3), (20,12,135.8,0.2), (21,6,135.8,0.2),
        (27,15,158.4,0.2)
    ),
}           # fmt: skip


def symbol_grid(table, quality):
    """The blocks of ``SYMBOL_BLOCKS[table, quality]`` sixteen to a row, the rest of the last row flat: grey for the luma
    table; for the chroma table R = G = 127 - s and B = 128 + s, whose Cb is exactly 128 + s (the step 1 formula)."""
    y, x = np.mgrid[0:8, 0:8]
    blocks = []
    for k, p, ak, ap in SYMBOL_BLOCKS[table, quality]:
        (uk, vk), (up, vp) = _zz(k), _zz(p)
        b = 128 + ak * np.cos((2 * x + 1) * uk * np.pi / 16) * np.cos((2 * y + 1) * vk * np.pi / 16)
        if p:
            b = b + ap * np.cos((2 * x + 1) * up * np.pi / 16) * np.cos((2 * y + 1) * vp * np.pi / 16)
        blocks.append(np.clip(np.rint(b), 0, 255).astype(np.uint8))
    blocks += [np.full((8, 8), 128, np.uint8)] * (-len(blocks) % 16)
    g = np.concatenate([np.concatenate(blocks[i:i + 16], 1) for i in range(0, len(blocks), 16)], 0)
    if table == "luma":
        return g
    return np.stack([255 - g, 255 - g, g], 2)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    n = 0
    for (h, w), layout in itertools.product(SIZES, LAYOUTS):
        c = 1 if layout == "grey" else 3
        img = photo(h, w, c, n) if n % 3 else noise(h, w, c, n)
        kw = dict(quality=QUALITIES[n % 5], subsampling="4:2:0" if layout == "grey" else layout, restart_rows=(n // 5) % 3,
                  order="bgr" if c == 3 and n % 4 == 1 else "rgb")
        out.append((f"{h}x{w}_{layout}", img, kw, {}))
        n += 1
    # the bottom chroma rows: H % 16 == 8 with 4:2:0, noise, so the down-sampled row 11 / 19 differs from a late replication
    for h, w in ((40, 25), (24, 40)):
        out.append((f"edge_{h}x{w}", noise(h, w, 3, 100 + h), dict(quality=95), dict(early_differs=True)))
    # dummy blocks of 4:2:0: last MCU column only, last MCU row only, both
    out.append(("dummy_right", photo(16, 24, 3, 7), dict(quality=75), dict(dummy_right=2, dummy_below=0)))
    out.append(("dummy_below", photo(24, 16, 3, 8), dict(quality=75), dict(dummy_right=0, dummy_below=2)))
    out.append(("dummy_both", photo(24, 24, 3, 9), dict(quality=75, restart_rows=1), dict(dummy_right=3, dummy_below=4)))
    out.append(("dummy_422", photo(9, 40, 3, 10), dict(quality=30, subsampling="4:2:2"), dict(dummy_right=2, dummy_below=0)))
    # symbols
    out.append(("run19", basis(*_zz(20), blocks=2), dict(quality=50), dict(f0_codes=2, symbols_ac_luma={0x00, 0xf0, 0x35})))
    out.append(("run39", basis(*_zz(40), blocks=1), dict(quality=50), dict(f0_codes=2)))
    out.append(("coef63", basis(7, 7, 127, blocks=2), dict(quality=50), dict(f0_codes=6, eob_codes=0)))
    out.append(("zeros", np.full((16, 24), 128, np.uint8), dict(quality=75), dict(eob_codes=6, stuffed=0, unit_bits=[6 * 6])))
    bw = np.zeros((8, 32), np.uint8)
    bw[:, 8:16] = 255
    bw[:, 24:] = 255
    out.append(("dc11", bw, dict(quality=100), dict(dc_categories={11})))
    yb = np.zeros((8, 16, 3), np.uint8)                      # yellow next to blue: Cb 0 next to 255 (DC -1024, then +2040), Cr 148 next to 107
    yb[:, :8] = (255, 255, 0)
    yb[:, 8:] = (0, 0, 255)
    out.append(("dc11_chroma", yb, dict(quality=100, subsampling="4:4:4"), dict(dc_chroma_categories={8, 9, 11})))
    half = np.zeros((8, 8), np.uint8)
    half[:, 4:] = 255
    out.append(("ac10", half, dict(quality=100), dict(max_ac_category=10)))
    # every AC symbol of both tables: grids of basis blocks, grey for the luma table, 4:4:4 colour along Cb for the chroma one
    out.append(("symbols_luma_q50", symbol_grid("luma", 50), dict(quality=50), dict(ac_symbols=(57, 0))))
    out.append(("symbols_luma_q100", symbol_grid("luma", 100), dict(quality=100), dict(ac_symbols=(118, 0), max_ac_category=10)))
    out.append(("symbols_chroma_q50", symbol_grid("chroma", 50), dict(quality=50, subsampling="4:4:4"), dict(ac_symbols=(32, 52))))
    out.append(("symbols_chroma_q100", symbol_grid("chroma", 100), dict(quality=100, subsampling="4:4:4"), dict(ac_symbols=(110, 155))))
    # stuffing (seeds found by search over the restatement)
    out.append(("ff_many", noise(16, 16, 3, 3), dict(quality=100, subsampling="4:4:4"), dict(stuffed_min=1)))
    out.append(("ff_before_eoi", noise(8, 8, 1, 5), dict(quality=100), dict(ff_ends=[True])))
    out.append(("ff_before_rst", noise(24, 8, 1, 2), dict(quality=100, restart_rows=1), dict(ff_ends=[False, True, False])))
    out.append(("ff_straddle", noise(8, 160, 1, 36), dict(quality=100), dict(ff_straddle=1, unit_bits=[12699, 3228])))
    # units of 16 MCUs: exactly one, one and one MCU, many; bit lengths that are a multiple of 32, of 8 only, of neither
    out.append(("one_unit", noise(8, 128, 1, 11), dict(quality=90), dict(units=1)))
    out.append(("unit_plus_mcu_32", noise(8, 136, 1, 67), dict(quality=90), dict(unit_bits=[6496, 398])))
    out.append(("unit_plus_mcu_8", noise(8, 136, 1, 14), dict(quality=90), dict(unit_bits=[6408, 412])))
    out.append(("many_units", photo(64, 272, 3, 12), dict(quality=75, restart_rows=2), dict(units=6, intervals=2)))
    out.append(("many_units_444", photo(40, 72, 3, 13), dict(quality=95, subsampling="4:4:4"), dict(units=3, intervals=1)))
    # more than nine MCU rows with a restart marker per row: RST7 is followed by RST0
    out.append(("rst_wrap", photo(88, 8, 1, 14), dict(quality=75, restart_rows=1), dict(intervals=11, markers=[0xd0 + i % 8 for i in range(10)])))
    out.append(("rst_wrap_420", photo(168, 20, 3, 15), dict(quality=30, restart_rows=1), dict(intervals=11)))
    # the bound's near-worst image: alternating extremes at quality 100
    worst = (np.random.default_rng(21).integers(0, 2, (16, 16, 3)) * 255).astype(np.uint8)
    out.append(("near_worst", worst, dict(quality=100, subsampling="4:4:4"), dict(bound_ratio_min=0.25)))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def _encoded(name):
    _, img, kw, _ = next(c for c in cases() if c[0] == name)
    info = {}
    return R.encode(img, info=info, **kw), info


def reference(name) -> bytes:
    """The restatement's file of a case, computed once."""
    return _encoded(name)[0]


def scan_markers(data: bytes):
    """The RSTn marker bytes inside the entropy data of a file, in order."""
    at = data.index(b"\xff\xda")
    at += 2 + int.from_bytes(data[at + 2:at + 4], "big")
    body = data[at:-2]
    return [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xff and 0xd0 <= body[i + 1] <= 0xd7]


def measure(name) -> dict:
    """What a case's ``expect`` is compared with, from the restatement."""
    _, img, kw, _ = next(c for c in cases() if c[0] == name)
    data, info = _encoded(name)
    a = np.asarray(img)
    H, W = a.shape[:2]
    ncomp = 1 if a.ndim == 2 else a.shape[2]
    hmax, vmax, mx, my = info["geometry"]
    wb, hb = -(-W // 8), -(-H // 8)
    right = below = 0
    if ncomp == 3:
        for r in range(my * vmax):
            for c in range(mx * hmax):
                below += r >= hb
                right += r < hb and c >= wb
    sym = info["symbols"]
    ac = [s for t, s in sym if t in (1, 3)]
    m = dict(dummy_right=right, dummy_below=below, stuffed=info["stuffed"], stuffed_min=min(info["stuffed"], 1), ff_ends=info["ff_ends"],
             ff_straddle=info["ff_straddle"], unit_bits=info["unit_bits"], units=len(info["unit_bits"]), intervals=info["intervals"],
             markers=scan_markers(data), dc_categories={s for t, s in sym if t in (0, 2)}, dc_chroma_categories={s for t, s in sym if t == 2},
             symbols_ac_luma={s for t, s in sym if t == 1}, ac_symbols=(len({s for t, s in sym if t == 1}), len({s for t, s in sym if t == 3})),
             max_ac_category=max([s & 15 for s in ac], default=0),
             f0_codes=sum(int((np.diff(np.flatnonzero(np.r_[1, z[1:]] != 0)) - 1 >> 4).sum()) for z in info["blocks"]),
             eob_codes=sum(int(z[63] == 0) for z in info["blocks"]),
             bound_ratio_min=min(len(data) / R.bound(H, W, ncomp, kw.get("quality", 75), kw.get("subsampling", "4:2:0"), kw.get("restart_rows", 0)), 0.25))
    if "early_differs" in next(c for c in cases() if c[0] == name)[3]:
        m["early_differs"] = R.encode(img, early=True, **kw) != data
    return m


def symbols_used():
    """Every (table, symbol) some case of the corpus codes: tables in DHT order (DC 0, AC 0, DC 1, AC 1)."""
    out = set()
    for name, *_ in cases():
        out |= _encoded(name)[1]["symbols"]
    return out
