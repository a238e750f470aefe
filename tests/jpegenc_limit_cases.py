"""Images that put the JPEG encoder's ASSEMBLY (launches 3 .. 7 of attwarp_amd/csrc/jpegenc.hip) at its
unit, scan-chunk, interval and address limits.  tests/jpegenc_cases.py covers what goes into the bit string; these cases cover
how the file is put together from the units' strings.  test_jpegenc_limits_ref_cpu.py proves every case from the restatement
(tests/jpegenc_ref.py: ``encode`` == ``assemble_by_units`` == Pillow, every ``expect``) and shows which seeded defect of the
assembly each class notices; test_jpegenc_limits_gpu.py runs them through the kernels.

A case is ``(name, image, keywords of R.encode, expect)`` as in jpegenc_cases.py; :func:`measure` gives what ``expect`` is
compared with.  Seeds and sizes were found by search over the restatement; every image is as small as its class allows.

Sub-byte units.  A flat grey block costs 6 bits (DC category 0 ``00``, EOB ``1010``), a flat 4:4:4 MCU 14 (luma 6, and ``00``
``00`` for each chroma block), so only an interval's LAST unit can be shorter than a byte: every other unit holds 16 MCUs.
Such a tail begins with the zeros of its DC code inside the straddling byte and ends with an EOB that has a zero in it, so
neither the straddling byte it completes nor the interval's last byte can be ``FF``: no case "behind an FF straddling byte"
exists, and ``ff_ends`` is False for every interval that ends in such a unit."""
import functools

import numpy as np

import jpegenc_cases as K
import jpegenc_ref as R

FAR_H, FAR_W, FAR_PITCH = 60000, 8, 36000     # the last row starts 59999 * 36000 = 2159964000 bytes behind the first: above 2^31
BATCH_SIZES = (255, 256, 257, 600)
MANY_UNITS = "chunks_grey_520"                # the many-unit image of the batches


def flat_rows(h, w, first, rest, k, c=1):
    """A grey (or, c = 3, colour) image of flat blocks: the first ``k`` block columns ``first``, the others ``rest``."""
    img = np.empty((h, w) if c == 1 else (h, w, 3), np.uint8)
    img[...] = rest
    img[:, :8 * k] = first
    return img


def extremes(h, w, c, seed):
    """Random 0 / 255 samples: the content that comes nearest the bound at quality 100."""
    a = (np.random.default_rng(seed).integers(0, 2, (h, w, c)) * 255).astype(np.uint8)
    return a[:, :, 0] if c == 1 else a


def sub_byte():
    """Units shorter than a byte: the tail unit of an interval of 17 flat MCUs."""
    q = dict(quality=75)
    return [
        # [98, 6]: the tail fills the straddling byte exactly, owns no byte, and places EOI behind none
        ("flat129_8x136", np.full((8, 136), 129, np.uint8), q, dict(unit_bits=[98, 6], owned=[13, 0], owning_none=1, ff_ends=[False])),
        # [99, 6]: five bits of the tail in the straddling byte; its own byte holds one of its bits and seven 1-bits
        ("flat130_8x136", np.full((8, 136), 130, np.uint8), q, dict(unit_bits=[99, 6], owned=[13, 1], owning_none=0, ff_ends=[False])),
        ("flat130_16x136_rst", np.full((16, 136), 130, np.uint8), dict(quality=75, restart_rows=1),
         dict(unit_bits=[99, 6, 99, 6], owned=[13, 1, 13, 1], owning_none=0, ff_ends=[False, False], intervals=2)),
        ("flat100_16x136_rst", np.full((16, 136), 100, np.uint8), dict(quality=75, restart_rows=1),
         dict(unit_bits=[102, 6, 102, 6], owned=[13, 1, 13, 1], owning_none=0, ff_ends=[False, False], intervals=2)),
        # [105, 6]: 105 % 8 == 1, so the straddling byte holds one bit of the first unit, the WHOLE tail and one 1-bit
        ("shared_straddle_8x136", flat_rows(8, 136, 99, 96, 1), q, dict(unit_bits=[105, 6], owned=[14, 0], owning_none=1, ff_ends=[False])),
        # the same with a marker behind the unit that owns nothing, twice, then EOI
        ("shared_straddle_24x136_rst", flat_rows(24, 136, 99, 96, 1), dict(quality=75, restart_rows=1),
         dict(unit_bits=[105, 6] * 3, owned=[14, 0] * 3, owning_none=3, ff_ends=[False] * 3, intervals=3)),
        ("flat129_24x136_rst", np.full((24, 136), 129, np.uint8), dict(quality=75, restart_rows=1),
         dict(unit_bits=[98, 6] * 3, owned=[13, 0] * 3, owning_none=3, ff_ends=[False] * 3, intervals=3)),
        # a flat 4:4:4 tail MCU: 14 bits
        ("flat444_8x136", np.full((8, 136, 3), 77, np.uint8), dict(quality=75, subsampling="4:4:4"),
         dict(unit_bits=[232, 14], owned=[29, 2], owning_none=0, ff_ends=[False])),
        # 274 % 8 == 2: six bits of the 14 in the straddling byte, the other eight are one whole byte and the interval ends aligned
        ("flat444_aligned_8x136", flat_rows(8, 136, (60, 130, 195), 130, 1, 3), dict(quality=75, subsampling="4:4:4"),
         dict(unit_bits=[274, 14], owned=[35, 1], owning_none=0, ff_ends=[False])),
    ]


def scan_chunks():
    """More than SCAN_CHUNK = 256 units in one image: the carries of the scans over units, `s // upi` behind the first chunk,
    `upos0` and `RSTn` beyond eleven intervals."""
    return [
        (MANY_UNITS, K.noise(520, 520, 1, 1), dict(quality=30, restart_rows=7), dict(units=270, intervals=10, upi=29, stuffed=137, chunks=2)),
        # 4:2:0, two MCUs per row, the right one half dummy; a restart per MCU row, so a unit per row: 256 and 257 units exactly
        ("chunk_256_420", K.noise(4096, 24, 3, 2), dict(quality=50, restart_rows=1), dict(units=256, intervals=256, upi=1, chunks=1)),
        ("chunk_257_420", K.noise(4104, 24, 3, 3), dict(quality=50, restart_rows=1), dict(units=257, intervals=257, upi=1, chunks=2)),
        # three chunks; 17 MCUs per row, so every interval is a full unit and a one-MCU unit
        ("chunks_three_grey", K.noise(2056, 136, 1, 4), dict(quality=50, restart_rows=1), dict(units=514, intervals=257, upi=2, chunks=3)),
    ]


def extreme():
    """The extreme shapes, all with noise (the planner's limits themselves are test_jpegenc_gpu.py's)."""
    return [
        ("column_grey_rst", K.noise(R.MAX_DIM, 1, 1, 5), dict(quality=75, restart_rows=1),
         dict(units=8188, intervals=8188, upi=1, chunks=32, rst_wraps=1023, stuffed=13148)),
        ("row_grey_rst8", K.noise(1, R.MAX_DIM, 1, 6), dict(quality=75, restart_rows=8), dict(units=512, intervals=1, upi=4094, chunks=2, stuffed=9365)),
        # every MCU dummy-right, the bottom one dummy-below too
        ("column_420", K.noise(R.MAX_DIM, 1, 3, 7), dict(quality=75), dict(units=256, intervals=1, upi=256, chunks=1)),
        ("row8_420_rst16", K.noise(8, R.MAX_DIM, 3, 8), dict(quality=75, restart_rows=16), dict(units=256, intervals=1, upi=4094, chunks=1, stuffed=1664)),
    ]


def near_worst():
    """One full unit of each sampling at the content nearest the bound: random 0 / 255 samples at quality 100.  ``unit_bits`` and
    ``slot_share`` (the unit's bits over blocks x block_bound_bits, the size of its slot) are recorded from the restatement."""
    q = dict(quality=100)
    return [
        ("worst_420_96_blocks", extremes(16, 256, 3, 21), dict(q, subsampling="4:2:0"), dict(unit_bits=[74586], slot_share=0.4509)),
        ("worst_444_48_blocks", extremes(8, 128, 3, 22), dict(q, subsampling="4:4:4"), dict(unit_bits=[38265], slot_share=0.4627)),
        ("worst_422_64_blocks", extremes(8, 256, 3, 23), dict(q, subsampling="4:2:2"), dict(unit_bits=[49708], slot_share=0.4508)),
    ]


def far_rows():
    """Dense 60000 x 8 host images; the GPU test writes them into a view whose rows are FAR_PITCH bytes apart."""
    return [
        ("far_grey", K.noise(FAR_H, FAR_W, 1, 9), dict(quality=75), dict(units=469, chunks=2, last_row_offset_above=1 << 31)),
        ("far_bgr", K.noise(FAR_H, FAR_W, 3, 10), dict(quality=75, order="bgr"), dict(units=235, chunks=1, last_row_offset_above=1 << 31)),
    ]


GROUPS = dict(sub_byte=sub_byte, scan_chunks=scan_chunks, extreme=extreme, near_worst=near_worst, far_rows=far_rows)


@functools.lru_cache(maxsize=None)
def cases():
    out = [c for g in GROUPS.values() for c in g()]
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def group(which):
    """The cases of one class, the very tuples of :func:`cases`."""
    names = {c[0] for c in GROUPS[which]()}
    return [c for c in cases() if c[0] in names]


def case(name):
    return next(c for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def plan(name):
    """R.unit_plan of a case, computed once: the units' bit strings, the header, ``file`` (R.encode's bytes)."""
    _, img, kw, _ = case(name)
    return R.unit_plan(img, **kw)


def reference(name) -> bytes:
    """The restatement's file of a case."""
    return plan(name)["file"]


@functools.lru_cache(maxsize=None)
def assembled(name):
    """The case's file put together unit by unit, and what R.assemble_batch reports of the units."""
    info = []
    files, _ = R.assemble_batch([plan(name)], info=info)
    return files[0], info[0]


def measure(name) -> dict:
    """What a case's ``expect`` is compared with, from the restatement."""
    _, img, kw, _ = case(name)
    p = plan(name)
    _, info = assembled(name)
    a = np.asarray(img)
    ncomp = 3 if a.ndim == 3 else 1
    bits = [len(u) for u in p["units"]]
    n, upi = len(bits), p["upi"]
    nint = -(-n // upi)
    hmax, vmax, mx, my = R.geometry(a.shape[0], a.shape[1], ncomp, kw.get("subsampling", "4:2:0"))
    blocks0 = min(R.UNIT_MCUS, mx * my) * (hmax * vmax + 2 if ncomp == 3 else 1)
    return dict(unit_bits=bits, units=n, intervals=nint, upi=upi, chunks=-(-n // R.SCAN_CHUNK), stuffed=p["stuffed"], ff_ends=p["ff_ends"],
                owned=info["owned"], owning_none=info["owning_none"], rst_wraps=(nint - 1) // 8,
                slot_share=round(bits[0] / (blocks0 * R.block_bound_bits(kw.get("quality", 75), ncomp)), 4),
                last_row_offset_above=(1 << 31) if (a.shape[0] - 1) * FAR_PITCH > 1 << 31 else 0)


# ---- batches of more than SCAN_CHUNK files -------------------------------------------------------------------------------------------
TINY_SIZES = ((1, 1), (1, 17), (17, 1), (8, 8), (3, 5), (9, 16), (17, 9))          # (H, W): 1 x 1 ... 17 x 9


@functools.lru_cache(maxsize=None)
def tiny(i):
    """Tiny image i: sizes, layouts, qualities and restart_rows cycle with periods 7, 4, 5 and 3, so file lengths differ."""
    h, w = TINY_SIZES[i % 7]
    layout = K.LAYOUTS[i % 4]
    c = 1 if layout == "grey" else 3
    img = K.photo(h, w, c, 500 + i) if i % 2 else K.noise(h, w, c, 500 + i)
    kw = dict(quality=K.QUALITIES[i % 5], subsampling="4:2:0" if c == 1 else layout, restart_rows=i % 3, order="bgr" if c == 3 and i % 8 == 5 else "rgb")
    return f"tiny_{i}", img, kw, {}


@functools.lru_cache(maxsize=None)
def tiny_plan(i):
    _, img, kw, _ = tiny(i)
    return R.unit_plan(img, **kw)


@functools.lru_cache(maxsize=None)
def batch(n):
    """A batch of ``n`` files -> [(case, plan)]: tiny images, and the many-unit image first (255), last (256), in the middle
    (257) or at all three places (600)."""
    big = {255: (0,), 256: (255,), 257: (128,), 600: (0, 300, 599)}[n]
    return [(case(MANY_UNITS), plan(MANY_UNITS)) if i in big else (tiny(i), tiny_plan(i)) for i in range(n)]
