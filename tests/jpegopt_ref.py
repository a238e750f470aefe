"""numpy restatement of the JPEG encoder's optimised Huffman tables (attwarp_amd/csrc/jpegopt_blocks.hpp, the jpegopt_*
kernels of jpegenc.hip): the bytes of ``Image.save(f, "JPEG", ..., optimize=True)`` from the symbol counts
of the scan and the IJG library's published ``jpeg_gen_optimal_table``.  No Pillow in here; tests/test_jpegopt_ref_cpu.py
proves it against Pillow, the host and GPU tests prove the table builder and the kernels against it.

:func:`histograms` counts what tests/jpegenc_ref.block_bits codes, :func:`optimal_table` builds one table, :func:`encode`
runs jpegenc_ref's ``header`` and ``encode`` with the image's tables in place of Annex K's.  ``defect`` seeds exactly one
wrong reading of the procedure, in this file only: the case list must notice each.
"""
import contextlib

import numpy as np

import jpegenc_ref as R

SENTINEL = 1_000_000_000              # libjpeg's search starts here: a larger frequency is never selected
DEFECTS = {
    "tie_smaller_index": "the search keeps the FIRST of equal frequencies (< in place of <=)",
    "no_reserved_leaf": "leaf 256 is not added (and none is dropped at the end): a code of all ones may appear",
    "clamp_to_16": "no limiter: code sizes above 16 are clamped to 16 (an over-subscribed code)",
    "dc_no_restart_reset": "the DC predictor runs through the restart markers when the symbols are counted",
}


def _prepared(img, order):
    a = np.asarray(img)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim == 3 and order == "bgr":
        a = a[:, :, ::-1]
    return a


def block_symbols(z, pred):
    """(DC symbol, [AC symbols]) of one block of zigzag coefficients: what jpegenc_ref.block_bits codes."""
    dc = int(abs(int(z[0]) - pred)).bit_length()
    ac, run = [], 0
    for k in range(1, 64):
        v = int(z[k])
        if v == 0:
            run += 1
            continue
        ac += [0xf0] * (run >> 4)
        ac.append((run & 15) << 4 | abs(v).bit_length())
        run = 0
    if run:
        ac.append(0)
    return dc, ac


def histograms(img, quality=75, subsampling="4:2:0", restart_rows=0, order="rgb", defect=None):
    """uint32-sized counts [4][256] in the order of the DHT segments (DC 0, AC 0, DC 1, AC 1), dummy blocks counted like
    real ones, the DC predictor back to zero at every restart interval."""
    a = _prepared(img, order)
    ncomp = 1 if a.ndim == 2 else 3
    mcus, (hmax, vmax, mx, my) = R.scan_blocks(a, quality, subsampling)
    step = restart_rows * mx or len(mcus)
    h = np.zeros((4, 256), np.int64)
    pred = [0] * ncomp
    for m, mcu in enumerate(mcus):
        if m % step == 0 and defect != "dc_no_restart_reset":
            pred = [0] * ncomp
        for ci, tid, z in mcu:
            dc, ac = block_symbols(z, pred[ci])
            pred[ci] = int(z[0])
            h[2 * tid, dc] += 1
            for s in ac:
                h[2 * tid + 1, s] += 1
    return h


def optimal_table(freq, defect=None, info=None):
    """jpeg_gen_optimal_table: 256 counts -> (BITS [16], VALS).  ``info``: receives ``depth``, the longest code before limiting.
    The length counts are sized for the deepest tree 257 leaves allow, where libjpeg's 33 entries overflow."""
    f = [int(v) for v in freq] + [0 if defect == "no_reserved_leaf" else 1]
    assert len(f) == 257 and min(f) >= 0
    codesize, others = [0] * 257, [-1] * 257

    def smallest(skip):
        c, v = -1, SENTINEL
        for i in range(257):
            if f[i] and i != skip and (f[i] < v or (f[i] == v and (defect != "tie_smaller_index" or c < 0))):
                c, v = i, f[i]
        return c
    while True:
        c1 = smallest(-1)
        c2 = smallest(c1)
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        for c, tail in ((c1, c2), (c2, None)):
            codesize[c] += 1
            while others[c] >= 0:
                c = others[c]
                codesize[c] += 1
            if tail is not None:
                others[c] = tail
    depth = max(codesize)
    bits = [0] * 258
    for n in codesize:
        if n:
            bits[min(n, 16) if defect == "clamp_to_16" else n] += 1
    for i in range(256, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    if defect != "no_reserved_leaf":
        i = 16
        while i > 1 and bits[i] == 0:
            i -= 1
        if bits[i]:
            bits[i] -= 1
    vals = [s for n in range(1, 257) for s in range(256) if codesize[s] == n]
    if info is not None:
        info.update(depth=depth)
    return bits[1:17], vals


def tables(hist, ncomp, defect=None, info=None):
    """The image's tables in DHT order; a grey image has two (the other two stay Annex K's, unused)."""
    out, depths = list(R.TABLES), []
    for t in range(4 if ncomp == 3 else 2):
        i = {}
        out[t] = optimal_table(hist[t], defect, i)
        depths.append(i["depth"])
    if info is not None:
        info.update(depths=depths, nsym=[len(out[t][1]) for t in range(len(depths))])
    return tuple(out)


@contextlib.contextmanager
def _tables_swapped(tabs):
    old = R.TABLES, R.CODES
    R.TABLES, R.CODES = tabs, [R.huffman_codes(*t) for t in tabs]
    try:
        yield
    finally:
        R.TABLES, R.CODES = old


def encode(img, quality=75, subsampling="4:2:0", restart_rows=0, order="rgb", optimize=True, defect=None, info=None):
    """uint8 [H,W] / [H,W,1] / [H,W,3] -> the file's bytes; ``optimize=False``: jpegenc_ref.encode.  ``info`` receives
    jpegenc_ref.encode's entries and ``depths`` / ``nsym`` (per table), ``tables`` and ``hist``."""
    if not optimize:
        return R.encode(img, quality, subsampling, restart_rows, order, info=info)
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")
    a = _prepared(img, order)
    hist = histograms(img, quality, subsampling, restart_rows, order, defect)
    extra = {}
    tabs = tables(hist, 1 if a.ndim == 2 else 3, defect, extra)
    with _tables_swapped(tabs):
        data = R.encode(img, quality, subsampling, restart_rows, order, info=info)
    if info is not None:
        info.update(extra, tables=tabs, hist=hist)
    return data


def bound(H, W, ncomp, quality=75, sub="4:2:0", restart_rows=0, optimize=True):
    """attwarp_jpegenc_bound_ex: the standard bound, and for an optimised image one more bit per block (a DC alphabet of 12
    categories and the reserved leaf: a code of up to 12 bits where Annex K's longest has 11).  The header never grows: at most
    12 and 162 symbols per DHT."""
    if not optimize:
        return R.bound(H, W, ncomp, quality, sub, restart_rows)
    hmax, vmax, mx, my = R.geometry(H, W, ncomp, sub)
    bpm = hmax * vmax + 2 if ncomp == 3 else 1
    nint = -(-my // restart_rows) if restart_rows else 1
    bits = mx * my * bpm * (R.block_bound_bits(quality, ncomp) + 1)
    return len(R.header(H, W, ncomp, quality, sub, 1 if restart_rows else 0)) + 2 * ((bits + 7) // 8 + nint) + 2 * nint + 2


def code_words(bits, vals):
    """je_build_huffman's packing: [256] words, length << 16 | code, 0 for a symbol without a code."""
    out = [0] * 256
    for s, (c, n) in R.huffman_codes(bits, vals).items():
        out[s] = n << 16 | c
    return out


def dht_segment(class_id, bits, vals):
    return b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([class_id]) + bytes(bits) + bytes(vals)


def kraft_gap(bits):
    """What a table's lengths leave of the code space, in codes of its longest length: 1 for an optimal table, whose only
    unused code is the reserved all-ones code of that length; negative for an over-subscribed table."""
    longest = max(k + 1 for k in range(16) if bits[k])
    return 2 ** longest - sum(b * 2 ** (longest - k - 1) for k, b in enumerate(bits))
