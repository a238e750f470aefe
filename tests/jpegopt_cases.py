"""The corpus of the optimised-table tests of the JPEG encoder: named images at the smallest shape that can go
wrong, with their parameters and an ``expect`` that tests/test_jpegopt_ref_cpu.py proves from the restatement
(tests/jpegopt_ref.py) and Pillow before the GPU test encodes the same cases.  A case is ``(name, image, keywords of
jpegopt_ref.encode, expect)``.  ``expect`` keys: ``depths`` / ``nsym`` (per table, DHT order; depth BEFORE limiting),
``depth_ac`` / ``nsym_ac`` (the luma AC table's depth; symbols of the two AC tables), ``shape``, ``header_bytes``,
``file_bytes``, ``max_length`` (the longest code in the file, over its tables), ``units``, ``noticed_by``
(defects of jpegopt_ref.DEFECTS that change this case's file), ``not_longer`` (Pillow's optimised file is not longer than its
plain one: a statement about those two files, not a general claim)."""
import functools

import numpy as np

import jpegenc_cases as K
import jpegenc_ref as R
import jpegopt_ref as O

# Single-coefficient blocks for the limiter images: (zigzag position, amplitude) of jpegenc_cases.basis at quality 50.  Those
# whose AC symbols are exactly {one symbol, EOB} are kept, one per distinct symbol, in this order.
LIMITER_BLOCKS = ((1, 46.7), (1, 155.6), (2, 50.9), (2, 169.7), (3, 59.4), (3, 118.8), (4, 36), (4, 72), (4, 144), (5, 21.2), (5, 42.4),
                  (5, 169.7), (6, 17), (6, 67.9), (7, 42), (7, 84), (7, 168), (8, 19.5), (8, 39), (8, 78), (8, 156), (9, 29.7), (9, 59.4),
                  (10, 76.4), (10, 152.7), (11, 25.5), (11, 102), (12, 24), (12, 96), (13, 28.5), (13, 57), (13, 114), (14, 25.5),
                  (14, 101.8), (15, 42.4), (15, 84.9), (16, 39), (16, 78), (16, 156))


@functools.lru_cache(maxsize=None)
def limiter_symbols():
    """[(AC symbol, 8 x 8 block)] of LIMITER_BLOCKS, distinct symbols only."""
    out, seen = [], set()
    for k, amp in LIMITER_BLOCKS:
        b = K.basis(*K._zz(k), amp=amp)
        mcus, _ = R.scan_blocks(b, 50, "4:4:4")
        _, ac = O.block_symbols(mcus[0][0][2], 0)
        if len(ac) == 2 and ac[1] == 0 and ac[0] not in (0, 0xf0) and ac[0] not in seen:
            seen.add(ac[0])
            out.append((ac[0], b))
    return out


def limiter_copies(n):
    """a1 = 1, a2 = 2, a(k) = a(k - 1) + a(k - 2) + 1: each symbol as frequent as the two rarer ones and the reserved leaf
    together cannot be merged with anything but their tree, so every symbol adds a level."""
    a = [1, 2]
    while len(a) < n:
        a.append(a[-1] + a[-2] + 1)
    return a[:n]


def limiter_image(n):
    """The n-th distinct symbol of limiter_symbols() in limiter_copies(n)[k] blocks, 64 blocks to a row, the last row filled
    with flat blocks: a grey image whose luma AC tree is n + 1 deep before limiting."""
    blocks = []
    for (_, b), copies in zip(limiter_symbols()[:n], limiter_copies(n)):
        blocks += [b] * copies
    blocks += [np.full((8, 8), 128, np.uint8)] * (-len(blocks) % 64)
    return np.concatenate([np.concatenate(blocks[i:i + 64], 1) for i in range(0, len(blocks), 64)], 0)


@functools.lru_cache(maxsize=None)
def table_histograms():
    """[(name, 256 counts, whether libjpeg has an answer)] for the table builder alone (the host program and the table kernel):
    random ones, all 256 symbols equal, one symbol, the limiter sequence to depth 20, and the same sequence 39 levels deep with
    counts up to 10^8, where libjpeg's bits[33] overflows and only the code's validity can be asked for."""
    rng = np.random.default_rng(77)
    out = []
    for k, (n, hi) in enumerate(((3, 5), (12, 100), (40, 1000), (162, 30), (162, 100000), (256, 3), (256, 10 ** 6), (100, 2))):
        h = np.zeros(256, np.int64)
        h[rng.choice(256, n, replace=False)] = rng.integers(1, hi + 1, n)
        out.append((f"random_{k}", h, True))
    out.append(("equal_256", np.full(256, 7, np.int64), True))
    one = np.zeros(256, np.int64)
    one[0x21] = 5
    out.append(("one_symbol", one, True))
    for name, n in (("depth_20", 20), ("depth_39", 39)):
        h = np.zeros(256, np.int64)
        h[255 - 3 * np.arange(n)] = limiter_copies(n)         # the rarest at the largest index
        out.append((name, h, n <= 32))
    assert out[-1][1].max() > 10 ** 8 and out[-1][1].sum() < O.SENTINEL
    return out


def worst(h, w, c, seed):
    a = (np.random.default_rng(seed).integers(0, 2, (h, w, c)) * 255).astype(np.uint8)
    return a[:, :, 0] if c == 1 else a


def tie_image():
    """Two blocks with AC symbols 0x01 and 0x11 once each and the end of block twice: the two rare symbols tie, and which of
    them is listed first depends on the tie rule."""
    return np.concatenate([K.basis(*K._zz(1), amp=46.7), K.basis(*K._zz(2), amp=50.9)], 1)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # tables of a single symbol: one code of one bit each
    out.append(("grey_1x1", np.full((1, 1), 128, np.uint8), dict(), dict(nsym=[1, 1], depths=[1, 1], max_length=1, file_bytes=159, header_bytes=328 - 216 + 2 * 22)))
    out.append(("flat_rgb_16", np.full((16, 16, 3), 128, np.uint8), dict(), dict(nsym=[1, 1, 1, 1], depths=[1, 1, 1, 1], max_length=1)))
    out.append(("column_17x1", K.photo(17, 1, 3, 4), dict(quality=90), dict()))
    # dummy blocks are counted like real ones
    out.append(("dummy_right", K.photo(16, 24, 3, 7), dict(quality=75), dict(not_longer=True)))
    out.append(("dummy_below", K.photo(24, 16, 3, 8), dict(quality=75), dict(not_longer=True)))
    out.append(("dummy_both", K.photo(24, 24, 3, 9), dict(quality=75, restart_rows=1), dict(not_longer=True)))
    out.append(("dummy_422", K.photo(9, 40, 3, 10), dict(quality=30, subsampling="4:2:2"), dict(not_longer=True)))
    out.append(("edge_40x25", K.noise(40, 25, 3, 140), dict(quality=95), dict(not_longer=True)))            # H % 16 == 8
    # the DC predictor goes back to zero at a restart: the DC histogram differs with and without it
    out.append(("restart_1", K.photo(48, 16, 3, 3), dict(quality=90, subsampling="4:2:2", restart_rows=1), dict(noticed_by=["dc_no_restart_reset"])))
    out.append(("restart_2", K.photo(56, 24, 1, 5), dict(quality=85, restart_rows=2), dict(noticed_by=["dc_no_restart_reset"])))
    out.append(("tie", tie_image(), dict(quality=50), dict(noticed_by=["tie_smaller_index", "no_reserved_leaf"], nsym=[1, 3])))
    # the limiter: a tree 18 / 19 / 20 deep, cut to 16 bits
    for n, shape in ((17, (1368, 512)), (18, (2216, 512)), (19, (3584, 512))):
        out.append((f"limiter_{n + 1}", limiter_image(n), dict(quality=50), dict(shape=shape, depth_ac=n + 1, max_length=16,
                                                                                  noticed_by=["clamp_to_16"] if n == 17 else [])))
    # many symbols: the AC symbol counts are jpegenc_cases' (every block there codes its symbols about once, so the codes stay
    # short: 7 to 10 bits)
    out.append(("symbols_luma_q50", K.symbol_grid("luma", 50), dict(quality=50), dict(nsym_ac=(57, 0))))
    out.append(("symbols_luma_q100", K.symbol_grid("luma", 100), dict(quality=100), dict(nsym_ac=(118, 0))))
    out.append(("symbols_chroma_q50", K.symbol_grid("chroma", 50), dict(quality=50, subsampling="4:4:4"), dict(nsym_ac=(32, 52))))
    out.append(("symbols_chroma_q100", K.symbol_grid("chroma", 100), dict(quality=100, subsampling="4:4:4"), dict(nsym_ac=(110, 155))))
    # one image's histogram from more workgroups than a scan chunk holds units; its AC tree is 17 deep, so the limiter runs on
    # plain noise too and the file holds 16-bit codes
    out.append(("noise_520", K.noise(520, 520, 1, 30), dict(quality=30, restart_rows=7), dict(units=270, not_longer=True, depth_ac=17, max_length=16)))
    # a full unit of near-worst content per sampling: the length stays within attwarp_jpegenc_bound_ex
    out.append(("worst_grey", worst(8, 128, 1, 21), dict(quality=100), dict(units=1)))
    out.append(("worst_444", worst(8, 128, 3, 22), dict(quality=100, subsampling="4:4:4"), dict(units=1)))
    out.append(("worst_422", worst(8, 256, 3, 23), dict(quality=100, subsampling="4:2:2"), dict(units=1)))
    out.append(("worst_420", worst(16, 256, 3, 24), dict(quality=100, subsampling="4:2:0"), dict(units=1)))
    # both channel orders
    out.append(("bgr", K.photo(33, 47, 3, 1), dict(quality=75, order="bgr"), dict(not_longer=True)))
    out.append(("rgb", K.photo(33, 47, 3, 1), dict(quality=75), dict(not_longer=True)))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def case(name):
    return next(c for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def _encoded(name, optimize=True):
    _, img, kw, _ = case(name)
    info = {}
    return O.encode(img, optimize=optimize, info=info, **kw), info


def reference(name, optimize=True) -> bytes:
    """The restatement's file of a case, computed once."""
    return _encoded(name, optimize)[0]


def measure(name) -> dict:
    """What a case's ``expect`` is compared with, from the restatement."""
    _, img, kw, _ = case(name)
    data, info = _encoded(name)
    lengths = [n for bits, _ in info["tables"][:len(info["depths"])] for n in range(1, 17) if bits[n - 1]]
    return dict(depths=info["depths"], nsym=info["nsym"], header_bytes=info["header_bytes"], file_bytes=len(data), max_length=max(lengths),
                depth_ac=info["depths"][1], nsym_ac=(info["nsym"][1], info["nsym"][3] if len(info["nsym"]) == 4 else 0), units=len(info["unit_bits"]), blocks=len(info["blocks"]), shape=tuple(np.asarray(img).shape[:2]),
                noticed_by=[d for d in case(name)[3].get("noticed_by", []) if defect_file(name, d) != data])


def defect_file(name, defect):
    """The case's file under a defect of jpegopt_ref.DEFECTS; None where the defective tables lack a symbol the scan codes."""
    _, img, kw, _ = case(name)
    try:
        return O.encode(img, defect=defect, **kw)
    except KeyError:
        return None


def pillow_keywords(kw):
    """Image.save's keywords for a case's (the order is applied to the pixels by the caller)."""
    out = {k: v for k, v in kw.items() if k in ("quality", "subsampling")}
    out["restart_marker_rows"] = kw.get("restart_rows", 0)
    return out
