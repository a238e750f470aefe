"""Baseline JPEG files of a whole ragged batch, decoded on the GPU (csrc/jpegdec.hip): what the reference
does per file with ``Image.open(path).convert('RGB')`` (main_batched.py:95-98, main.py:148-152, functions.py:36,
MN/dataloader.py:216,368).  Only compressed bytes cross to the device; the pixels are Pillow's, bit for bit.
SOF0 / SOF1, 8 bits, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, any restart interval.
With ``progressive=True`` (off by default) also SOF2: the host walks every scan of the file, the device runs one entropy
launch per dependency level of the scans; baseline and progressive files may share a list.
With ``all_layouts=True`` (off by default) a sequential file may also have four components (Adobe CMYK / YCCK), be RGB-coded,
or sample every component by factors of its own (4:4:0, 4:1:1, 4:1:0, a factor of 3, luma coarser than chroma ...): such files
go through a second family of records and kernels, alone or in a list with the others.
With ``all_scans=True`` (off by default; implies both) also the two cross terms they refuse: progressive files of those layouts
and sequential files whose components come in several scans, through a fourth family of scan records over the layout
family's image records.  It is the one switch for a folder somebody else made.

Encoding (csrc/jpegenc.hip): what the reference writes with ``img.save(f"{image_id}.jpg")`` (main.py:163-167)
and ``cv2.imwrite(output_path, warped)`` for a ``.jpg`` path (new_method.py:491): baseline JPEG files of a whole ragged
batch, written on the GPU, byte for byte what ``PIL.Image.save`` writes.  Only compressed bytes cross to the host.
"""
from __future__ import annotations

import ctypes
import os
import struct
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from ._batch import (TABLE, FileBatch, ImageBatch, download, file_bytes, indexed_device, planned_table, raise_first_broken, scattered,
                     split_indices, write_files)

JPEGDEC_MAX_UNITS = _lib.JPEGDEC_MAX_UNITS              # restart intervals per image
JPEGDEC_MAX_BLOCKS = _lib.JPEGDEC_MAX_BLOCKS            # 8x8 blocks per image, all components (exclusive)
JPEGDEC_MAX_SCANS = _lib.JPEGDEC_MAX_SCANS              # scans per progressive image
STATUS_NAMES = _lib.JPEGDEC_STATUS_NAMES
_ORDERS = {"rgb": _lib.RGB, "bgr": _lib.BGR}
_IMAGE_DTYPE = np.dtype(_lib.JpegDecImage)
SEGMENT_BYTES = 256                                     # the sub-streams' defaults: bytes per segment,
MAX_ROUNDS = 64                                         # rounds after which an image falls back to the sequential decode
MAX_SEGMENTS = 1 << 14                                  # an image with more segments is decoded sequentially
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_UNZIGZAG = tuple(_ZIGZAG.index(j) for j in range(64))    # natural position -> place in the zigzag order
_UNSUPPORTED_FRAMES = {0xC2: "progressive", 0xC3: "lossless", 0xC5: "hierarchical", 0xC6: "hierarchical", 0xC7: "hierarchical",
                       0xC9: "arithmetic", 0xCA: "arithmetic", 0xCB: "arithmetic", 0xCD: "arithmetic", 0xCE: "arithmetic",
                       0xCF: "arithmetic"}


def _marker_positions(mv) -> np.ndarray:
    """Offsets of every FF that is followed by neither 00 nor D0..D7 (the last byte counts as followed by nothing): where
    entropy data ends, by the rule of the device's restart scan.  Vectorised over the bytes."""
    b = np.frombuffer(mv, dtype=np.uint8)
    nxt = np.empty(b.size, dtype=np.uint16)
    nxt[:-1] = b[1:]
    nxt[-1:] = 0x100
    return np.flatnonzero((b == 0xFF) & (nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7)))


def scan_geometry(p: dict, comps) -> tuple:
    """(MCUs per row, MCUs) of a scan over the components ``comps`` (indices in frame order) of a parsed frame: a scan of one
    component walks the blocks that cover the component's true size, any other the frame's MCUs."""
    hs, vs = p["hs"], p["vs"]
    if len(comps) == 1:
        h, v = (hs, vs) if comps[0] == 0 else (1, 1)
        cw, ch = -(-p["W"] * h // hs), -(-p["H"] * v // vs)
        return -(-cw // 8), -(-cw // 8) * -(-ch // 8)
    mcux = -(-p["W"] // (8 * hs))
    return mcux, mcux * -(-p["H"] // (8 * vs))


def layout_scan_geometry(W: int, H: int, samp, comps) -> tuple:
    """:func:`scan_geometry` for a frame of any layout (``samp``: [(h, v)] per component): a scan of several components
    walks the FRAME's MCUs, also when it holds a subset of the components."""
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    if len(comps) == 1:
        h, v = samp[comps[0]]
        cw, ch = -(-W * h // hmax), -(-H * v // vmax)
        return -(-cw // 8), -(-cw // 8) * -(-ch // 8)
    mcux = -(-W // (8 * hmax))
    return mcux, mcux * -(-H // (8 * vmax))


def scan_levels(scans) -> List[int]:
    """The dependency level of every scan of one file: 0 if no earlier scan shares a component with it and overlaps its band,
    else 1 + the largest level among those.  Scans of one level write disjoint coefficients."""
    lv = []
    for i, a in enumerate(scans):
        deps = [lv[j] for j, e in enumerate(scans[:i]) if set(a["comps"]) & set(e["comps"]) and e["ss"] <= a["se"] and a["ss"] <= e["se"]]
        lv.append(1 + max(deps) if deps else 0)
    return lv


def _next_segment(mv, n: int, pos: int, behind_scan: bool, progressive: bool, bad, ended):
    """The marker segment at ``pos`` of the n bytes -> ``(marker, payload, offset behind it)``: fill bytes are skipped, markers
    no header may hold are refused.  ``behind_scan``: scan data has been passed, so the file may end anywhere (at EOI, in fill
    bytes, inside a segment) -> None; in front of the first scan a file that ends raises ``ended()``."""
    if pos >= n or (behind_scan and pos + 1 >= n):
        if behind_scan:
            return None                                     # the file ends behind a scan: complete or not, the caller says
        raise ended()
    if mv[pos] != 0xFF:
        raise bad("a marker was expected")
    while mv[pos] == 0xFF:                                  # fill bytes
        pos += 1
        if pos >= n:
            if behind_scan:
                return None
            raise ended()
    m = mv[pos]
    pos += 1
    if behind_scan and m == 0xD9:
        return None
    if m in _UNSUPPORTED_FRAMES and not (m == 0xC2 and progressive):
        raise bad(f"{_UNSUPPORTED_FRAMES[m]} frame (sequential Huffman only)")
    if m == 0xCC:
        raise bad("arithmetic conditioning")
    if m in (0x00, 0x01, 0xD8, 0xD9) or 0xD0 <= m <= 0xD7:
        raise bad(f"marker {m:02x} in the headers")
    if behind_scan and (pos + 2 > n or pos + (mv[pos] << 8 | mv[pos + 1]) > n):
        return None                                         # the file ends inside a segment behind a scan
    if pos + 2 > n:
        raise ended()
    L = mv[pos] << 8 | mv[pos + 1]
    if L < 2:
        raise bad("segment length below 2")
    if pos + L > n:
        raise ended()
    return m, bytes(mv[pos + 2:pos + L]), pos + L


def _read_sof(seg, bad, all_layouts: bool = False) -> tuple:
    """An SOF0 / SOF1 / SOF2 payload -> ``(W, H, [(id, h, v, quantisation table id) per component])``.  ``all_layouts``: four
    components pass too (two, and five or more, never do: Pillow refuses them as well)."""
    if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
        raise bad("bad frame header")
    prec, H, W, nf = struct.unpack(">BHHB", seg[:6])
    if prec != 8:
        raise bad(f"precision {prec} (8 only)")
    if H == 0 or W == 0:
        raise bad(f"size {W} x {H}")
    if nf not in ((1, 3, 4) if all_layouts else (1, 3)):
        raise bad(f"{nf} components ({'1, 3 or 4' if all_layouts else '1 or 3'})")
    return W, H, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)]


def _read_dht(seg, dcs: dict, acs: dict, bad):
    """Every table of a DHT payload into ``dcs`` / ``acs``: id -> (counts, symbols)."""
    q = 0
    while q < len(seg):
        if q + 17 > len(seg):
            raise bad("DHT runs past its segment")
        tc, th = seg[q] >> 4, seg[q] & 15
        if tc > 1 or th > 3:
            raise bad("DHT class / id")
        counts = seg[q + 1:q + 17]
        left = 1
        for c in counts:
            left = 2 * left - c
            if left < 0:
                raise bad("DHT over-subscribed")
        ns = sum(counts)
        if ns > 256 or q + 17 + ns > len(seg):
            raise bad("DHT symbols exceed 256 or run past the segment")
        syms = seg[q + 17:q + 17 + ns]
        if tc == 0 and any(s > 15 for s in syms):
            raise bad("DHT with a DC category above 15")
        (acs if tc else dcs)[th] = (counts, syms)
        q += 17 + ns


def _read_dqt(seg, qts: dict, bad):
    """Every table of a DQT payload into ``qts``: id -> 64 values in natural order."""
    q = 0
    while q < len(seg):
        pq, tq = seg[q] >> 4, seg[q] & 15
        if pq == 1:
            raise bad("16-bit quantisation table")
        if pq > 1 or tq > 3 or q + 65 > len(seg):
            raise bad("bad DQT")
        qts[tq] = [seg[q + 1 + k] for k in _UNZIGZAG]
        q += 65


def _frame_layout(comps, jfif: bool, adobe, bad) -> tuple:
    """The luma sampling factors (hs, vs) of a frame's components; refuses RGB-coded files (by libjpeg's Adobe / JFIF /
    component-id rule) and every sampling layout but 4:4:4, 4:2:2 and 4:2:0."""
    if len(comps) != 3:
        return 1, 1
    if adobe == 0 or (adobe is None and not jfif and bytes(c[0] for c in comps) == b"RGB"):
        raise bad("RGB-coded file (YCbCr only)")
    samp = [(c[1], c[2]) for c in comps]
    if samp[1] != (1, 1) or samp[2] != (1, 1) or samp[0] not in ((1, 1), (2, 1), (2, 2)):
        raise bad(f"sampling layout {samp} (4:4:4, 4:2:2, 4:2:0)")
    return samp[0]


def _any_layout(comps, jfif: bool, adobe, bad) -> tuple:
    """What ``all_layouts`` makes of a frame's components -> ``(hs, vs, None)`` for a file the baseline records hold (grey, or
    YCbCr 4:4:4 / 4:2:2 / 4:2:0), else ``(hmax, vmax, dict(samp=[(h, v) per component], color=...))``.  The colour rule is
    libjpeg's (default_decompress_parms): three components are YCbCr if a JFIF marker was seen, else what the Adobe transform
    says (0: RGB), else RGB only for the component ids ``R``, ``G``, ``B``; four components are CMYK unless an Adobe marker
    names a transform other than 0 (YCCK).  Factors outside 1..4, more than 10 blocks per MCU (T.81 B.2.3) and factors that
    do not divide the frame's largest (libjpeg has no fractional up-sampling) are refused."""
    nf = len(comps)
    if nf == 1:
        return 1, 1, None                                   # (not interleaved: its factors do not count)
    samp = [(c[1], c[2]) for c in comps]
    if any(not 1 <= f <= 4 for hv in samp for f in hv):
        raise bad(f"sampling factors {samp} outside 1..4")
    if sum(h * v for h, v in samp) > _lib.JPEGDEC_MAX_SLOTS:
        raise bad(f"sampling layout {samp}: {sum(h * v for h, v in samp)} blocks per MCU (at most {_lib.JPEGDEC_MAX_SLOTS})")
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    if any(hmax % h or vmax % v for h, v in samp):
        raise bad(f"sampling layout {samp}: a component's factors do not divide the largest (fractional up-sampling)")
    if nf == 3:
        rgb = not jfif and (adobe == 0 if adobe is not None else bytes(c[0] for c in comps) == b"RGB")
        color = "rgb" if rgb else "ycc"
        if color == "ycc" and samp[1] == samp[2] == (1, 1) and samp[0] in ((1, 1), (2, 1), (2, 2)):
            return samp[0] + (None,)
    else:
        color = "cmyk" if adobe in (None, 0) else "ycck"
    return hmax, vmax, dict(samp=samp, color=color)


def _read_sos(seg, most, bad) -> tuple:
    """An SOS payload -> ``([component id], [(DC table id, AC table id)], (Ss, Se, Ah, Al))``.  ``most``: the components a
    scan may hold, at least one (None: the caller checks which it holds)."""
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0] or (most is not None and not 1 <= seg[0] <= most):
        raise bad("bad scan header")
    ns = seg[0]
    return ([seg[1 + 2 * i] for i in range(ns)], [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)],
            (seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15))


def _size_limit(units: int, blocks: int, data_bytes: int, all_scans: bool, bad):
    if units > JPEGDEC_MAX_UNITS or blocks >= JPEGDEC_MAX_BLOCKS or data_bytes >= 1 << 31:
        raise bad(f"size limit: {units} restart intervals{' over all scans' if all_scans else ''} (at most {JPEGDEC_MAX_UNITS}), "
                  f"{blocks} blocks (below {JPEGDEC_MAX_BLOCKS})")


def _baseline(frame, sos, layout, tables, ri: int, data_off: int, n: int, bad, all_layouts: bool = False) -> dict:
    """The result of a sequential file from its one scan: the scan must hold all components with (Ss, Se, Ah, Al) =
    (0, 63, 0, 0); nothing behind its header is looked at.  ``all_layouts``: see :func:`_any_layout`; a file of another
    layout also gets ``layout=True``, ``samp`` and ``color``, and its ``hs``, ``vs`` are the frame's largest factors."""
    (W, H, comps), (ids, tabs, band), (qts, dcs, acs) = frame, sos, tables
    nf = len(comps)
    if ids != [c[0] for c in comps]:
        raise bad("the scan does not hold all components in frame order (more than one scan)")
    if band != (0, 63, 0, 0):
        raise bad("spectral selection / successive approximation")
    hs, vs, other = _any_layout(comps, *layout, bad) if all_layouts else _frame_layout(comps, *layout, bad) + (None,)
    qt, dc, ac = [], [], []
    for c, (td, ta) in zip(comps, tabs):
        if c[3] not in qts or td not in dcs or ta not in acs:
            raise bad("the scan names a table never defined")
        qt.append(qts[c[3]]); dc.append(dcs[td]); ac.append(acs[ta])
    mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
    units = -(-mcus // ri) if ri else 1
    _size_limit(units, mcus * (sum(h * v for h, v in other["samp"]) if other else hs * vs + nf - 1), n - data_off, False, bad)
    p = dict(W=W, H=H, ncomp=nf, hs=hs, vs=vs, ri=ri, qt=qt, dc=dc, ac=ac, data_off=data_off, units=units)
    return dict(p, layout=True, **other) if other else p


def _progressive_scan(comps, sos, sent, latched: dict, tables, bad) -> dict:
    """One scan of a progressive file checked against what the scans before it sent (``sent``: per component and coefficient
    the Al it was last sent with, updated here) -> ``dict(comps, ss, se, ah, al, tables)``.  ``latched``: the quantisation
    table each component had at its first scan (libjpeg latches it there)."""
    (ids, tabs, (ss, se, ah, al)), (qts, dcs, acs) = sos, tables
    ns, frame_ids = len(ids), [c[0] for c in comps]
    if any(i not in frame_ids for i in ids):
        raise bad("the scan names a component the frame does not have")
    ci = [frame_ids.index(i) for i in ids]
    if any(b <= a for a, b in zip(ci, ci[1:])):
        raise bad("the scan's components are not in frame order")
    if ss > se or se > 63 or (ss == 0 and se != 0) or (ss > 0 and ns > 1) or al > 13 or (ah != 0 and al != ah - 1):
        raise bad(f"bad progression: Ss={ss} Se={se} Ah={ah} Al={al} in a scan of {ns} component(s)")
    used = []
    for c, (td, ta) in zip(ci, tabs):
        if ss > 0 and sent[c][0] is None:
            raise bad(f"an AC scan of component {c} before its DC was sent")
        band, before = sent[c][ss:se + 1], ah or None      # (before: the Al every coefficient of the band must have been sent with)
        if band.count(before) != len(band):
            k = next(k for k in range(ss, se + 1) if sent[c][k] != before)
            raise bad(f"a first pass over coefficient {k} of component {c}, which was already sent" if ah == 0 else
                      f"a refinement Ah={ah} of coefficient {k} of component {c}, whose precision is {sent[c][k]}")
        sent[c][ss:se + 1] = [al] * len(band)
        if c not in latched:
            if comps[c][3] not in qts:
                raise bad("the scan names a table never defined")
            latched[c] = qts[comps[c][3]]
        if ss > 0 or ah == 0:                                # (a DC refinement sends raw bits: no table)
            known, t = (acs, ta) if ss > 0 else (dcs, td)
            if t not in known:
                raise bad("the scan names a table never defined")
            used.append(known[t])
    return dict(comps=ci, ss=ss, se=se, ah=ah, al=al, tables=used)


def _sequential_scan(comps, sos, sent, latched: dict, tables, bad) -> dict:
    """One scan of a sequential file of several scans (``all_scans``): band (0, 63, 0, 0), 1 .. 4 components in frame order,
    each component of the file sent exactly once -> ``dict(comps, ss, se, ah, al, tables)`` with ``tables`` the DC table of
    every component of the scan, then the AC table of every component.  ``sent``, ``latched``: as :func:`_progressive_scan`."""
    (ids, tabs, band), (qts, dcs, acs) = sos, tables
    frame_ids = [c[0] for c in comps]
    if not 1 <= len(ids) <= len(comps):
        raise bad("bad scan header")
    if any(i not in frame_ids for i in ids):
        raise bad("the scan names a component the frame does not have")
    ci = [frame_ids.index(i) for i in ids]
    if any(b <= a for a, b in zip(ci, ci[1:])):
        raise bad("the scan's components are not in frame order")
    if band != (0, 63, 0, 0):
        raise bad("spectral selection / successive approximation in a sequential file")
    dc, ac = [], []
    for c, (td, ta) in zip(ci, tabs):
        if sent[c][0] is not None:
            raise bad(f"a second scan of component {c} of a sequential file, which was already sent")
        sent[c][:] = [0] * 64
        if comps[c][3] not in qts or td not in dcs or ta not in acs:
            raise bad("the scan names a table never defined")
        latched[c] = qts[comps[c][3]]
        dc.append(dcs[td]); ac.append(acs[ta])
    return dict(comps=ci, ss=0, se=63, ah=0, al=0, tables=dc + ac, sequential=True)


def parse_jpeg(data, index: int = 0, progressive: bool = False, all_layouts: bool = False, all_scans: bool = False) -> dict:
    """The host's whole part of decoding one file: the walk over the marker segments up to the SOS header.  bytes-like ->
    ``dict(W, H, ncomp, hs, vs, ri, qt, dc, ac, data_off)``: luma sampling factors, the restart interval (0: none), per
    component the quantisation table (64 values, natural order) and the (counts, symbols) of its DC and AC Huffman tables,
    and the offset of the first byte behind the SOS header.  No entropy-coded byte is looked at.  ValueError names what
    is not decoded; a file that ends inside its headers raises OSError.

    ``progressive=True`` also accepts an SOF2 frame (same precision, components and sampling).  The walk then goes over the
    WHOLE file: every marker between the scans is found (vectorised), DHT / DRI / DQT apply in file order, and the result
    has ``progressive=True``, ``ri=0``, empty ``dc`` / ``ac``, the quantisation table each component had at its first scan,
    and ``scans``: per scan ``dict(comps, ss, se, ah, al, ri, tables, off, end, units)`` with the component indices, the
    tables it names resolved to (counts, symbols) (one DC table per component of a DC first pass, one AC table of an AC
    scan) and the byte range of its entropy data in the file.  ValueError for a bad progression, a refinement that does
    not continue the precision sent, a first pass over a coefficient already sent, an AC scan before the component's
    DC, more than :data:`JPEGDEC_MAX_SCANS` scans, and an incomplete file (some coefficient never reached ``Al = 0`` at EOI
    or at the file's end).  A file that ends INSIDE a scan is not refused: the device gives it a status.  One walk for both
    kinds: a sequential file's first SOS ends it (:func:`_baseline`); an SOF2 file's scans go through the same SOS reader.

    ``all_layouts=True`` also accepts, in a sequential file, four components, RGB coding and any sampling factors libjpeg
    decodes (:func:`_any_layout`); the result then has ``layout=True``, ``samp`` ([(h, v)] per component), ``color`` ("ycc",
    "rgb", "cmyk", "ycck") and the frame's largest factors as ``hs``, ``vs``.  The colour rule is then libjpeg's throughout: a
    JFIF file stays YCbCr whatever an Adobe marker says.  A file the baseline records hold parses exactly as without the
    keyword.  Still refused: a progressive file of such a layout, more than one scan, 16-bit quantisation tables, 12-bit,
    arithmetic, lossless and hierarchical files.

    ``all_scans=True`` implies both keywords and also accepts the two cross terms they refuse: an SOF2 frame
    of any layout :func:`_any_layout` accepts (at most 10 blocks per MCU: the slot map of an image record has ten entries),
    under the progression checks above over up to four components; and an SOF0 / SOF1 file of several scans, each with band
    (0, 63, 0, 0) and 1 .. 4 components in frame order, in any order of scans (a plain 4:2:0 file in three scans too).  The
    walk goes over the whole file, and the result has ``scanned=True``, ``sequential`` (the frame is SOF0 / SOF1), ``samp``,
    ``color``, the largest factors as ``hs``, ``vs``, ``ri=0``, empty ``dc`` / ``ac``, and ``scans`` and ``levels`` as
    above; a sequential scan has ``sequential=True`` and names in ``tables`` the DC table of each of its components, then
    the AC table of each.  ValueError for a second scan of a component of a sequential file (*already sent*) and for a
    component never sent at EOI (*incomplete*); a file that ends inside a scan gets a status from the device.  A file one of
    the three other kinds holds parses exactly as with ``progressive=True, all_layouts=True``.  Still refused: 16-bit
    quantisation tables, 12-bit, arithmetic, lossless and hierarchical files, more than :data:`JPEGDEC_MAX_SCANS` scans, more
    than :data:`JPEGDEC_MAX_UNITS` units over all scans."""
    progressive, all_layouts = progressive or all_scans, all_layouts or all_scans
    mv = memoryview(data).cast("B")
    n = len(mv)

    def bad(what):
        return ValueError(f"jpeg: file {index}: {what}")

    def ended():
        return OSError(f"jpeg: file {index}: the file ends inside its headers")

    if n < 2:
        raise ended()
    if mv[0] != 0xFF or mv[1] != 0xD8:
        raise bad("bad signature")
    pos, sof, frame, ri, jfif, adobe = 2, 0, None, 0, False, None
    qts, dcs, acs = {}, {}, {}
    scans, latched, cut = [], {}, False                     # of an SOF2 file
    while True:
        at = _next_segment(mv, n, pos, bool(scans), progressive, bad, ended)
        if at is None:
            break
        m, seg, pos = at
        if m in (0xC0, 0xC1, 0xC2):
            if frame is not None:
                raise bad("a second frame (hierarchical)")
            sof, frame = m & 3, _read_sof(seg, bad, all_layouts)
        elif m == 0xC4:
            _read_dht(seg, dcs, acs, bad)
        elif m == 0xDB:
            _read_dqt(seg, qts, bad)
        elif m == 0xDD:
            if len(seg) != 2:
                raise bad("bad DRI")
            ri = seg[0] << 8 | seg[1]
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\0"
        elif m == 0xEE:
            if seg[:5] == b"Adobe" and len(seg) >= 12:
                adobe = seg[11]
        elif m in (0xDC, 0xDE, 0xDF):
            raise bad("DNL / hierarchical marker")
        elif m == 0xDA:
            if frame is None:
                raise bad("SOS before the frame header")
            W, H, comps = frame
            if sof != 2:
                sos = _read_sos(seg, None, bad)
                # (all_scans: a first scan that does not hold all components in frame order starts a file of several scans)
                if not (all_scans and (scans or sos[0] != [c[0] for c in comps])):
                    return _baseline(frame, sos, (jfif, adobe), (qts, dcs, acs), ri, pos, n, bad, all_layouts)
            if not scans:
                hs, vs, other = _any_layout(comps, jfif, adobe, bad) if all_layouts else _frame_layout(comps, jfif, adobe, bad) + (None,)
                if other and not all_scans:
                    raise bad(f"progressive file of {len(comps)} components, {other['color']}-coded, sampling {other['samp']}: "
                              "all_layouts covers sequential files only")
                if sof != 2 and other is None:               # a plain layout in several scans: the general records hold it too
                    other = dict(samp=[(hs, vs)] + [(1, 1)] * (len(comps) - 1), color="ycc" if len(comps) == 3 else "grey")
                sent = [[None] * 64 for _ in comps]          # per coefficient: the Al it was last sent with
                markers, data_off = _marker_positions(mv), pos
            if len(scans) >= JPEGDEC_MAX_SCANS:
                raise bad(f"more than {JPEGDEC_MAX_SCANS} scans")
            if sof != 2:
                scan = _sequential_scan(comps, sos, sent, latched, (qts, dcs, acs), bad)
            else:
                scan = _progressive_scan(comps, _read_sos(seg, len(comps), bad), sent, latched, (qts, dcs, acs), bad)
            nmcu = (layout_scan_geometry(W, H, other["samp"], scan["comps"]) if other else
                    scan_geometry(dict(W=W, H=H, hs=hs, vs=vs), scan["comps"]))[1]
            k = int(np.searchsorted(markers, pos))
            end = int(markers[k]) if k < markers.size else n
            scans.append(dict(scan, ri=ri, off=pos, end=end, units=-(-nmcu // ri) if ri else 1))
            cut = end + 1 >= n                              # nothing, or a lone FF, behind the data: the file ends inside the scan
            pos = end
    if not cut and any(a != 0 for row in sent for a in row):
        raise bad("incomplete progressive file: some coefficient was never sent or never reached Al = 0" if sof == 2 else
                  "incomplete sequential file: a component was never sent")
    nf, units = len(comps), sum(s["units"] for s in scans)
    slots = sum(h * v for h, v in other["samp"]) if other else hs * vs + nf - 1
    _size_limit(units, -(-W // (8 * hs)) * -(-H // (8 * vs)) * slots, n - data_off, True, bad)
    qt = [latched.get(c, qts.get(comps[c][3], [0] * 64)) for c in range(nf)]
    p = dict(W=W, H=H, ncomp=nf, hs=hs, vs=vs, ri=0, qt=qt, dc=[], ac=[], data_off=data_off, units=units, scans=scans,
             levels=scan_levels(scans))
    return dict(p, scanned=True, sequential=sof != 2, **other) if other else dict(p, progressive=True)


def _substream_plan(substreams, segment_bytes, max_rounds):
    if substreams not in ("auto", True, False):
        raise ValueError("jpeg: substreams must be 'auto', True or False")
    if substreams is False:
        return 0, 0
    sb = SEGMENT_BYTES if segment_bytes is None else int(segment_bytes)
    mr = MAX_ROUNDS if max_rounds is None else int(max_rounds)
    if sb not in (32, 64, 128, 256, 512) or not 1 <= mr <= 65536:
        raise ValueError(f"jpeg: segment_bytes={sb} must be a power of two in 32..512, max_rounds={mr} in 1..65536")
    return sb, mr


SCAN_KINDS = ("dc_first", "dc_refine", "ac_first", "ac_refine")
# The kinds of scan that scan_substreams="auto" cuts: those whose route made JpegFiles.run faster on the marker-less rows of
# tools/jpegprogsync_bench.py, measured by leaving the kind out of all four.  True cuts every kind.
AUTO_SCAN_KINDS = ("ac_first", "ac_refine", "dc_refine")
# The same for the progressive scans of files planned through the layout records (``all_scans``): a constant
# of its own, measured the same way on the marker-less rows of tools/jpegscansync_bench.py.  All four kinds: here the DC first
# pass settles in 2 - 4 rounds and saves 8 - 17 ms when added last; without it "auto" was slower than no keyword on the CMYK rows.
AUTO_LAYOUT_SCAN_KINDS = ("dc_first", "ac_first", "ac_refine", "dc_refine")


def scan_kind(scan: dict) -> str:
    """The kind of a progressive scan of :func:`parse_jpeg`: one of :data:`SCAN_KINDS`."""
    return SCAN_KINDS[(2 if scan["ss"] else 0) + (1 if scan["ah"] else 0)]


def _layout_scan_cut(scan: dict, scan_substreams) -> bool:
    """Whether ``scan_substreams`` asks for a scan of a file planned through the layout records to be cut: never a
    sequential scan; "auto": the kinds of :data:`AUTO_LAYOUT_SCAN_KINDS`."""
    if scan_substreams is False or scan.get("sequential"):
        return False
    return scan_substreams is True or scan_kind(scan) in AUTO_LAYOUT_SCAN_KINDS


def scan_segments(nbytes: int, units: int, segment_bytes: int) -> int:
    """Segments ``attwarp_jpegdec_plan_scans_ex`` plans for a scan of ``nbytes`` of entropy data and ``units`` units (0: one lane)."""
    nseg = -(-nbytes // segment_bytes) if segment_bytes else 0
    return nseg if segment_bytes and units == 1 and nbytes >= 2 * segment_bytes and nseg <= MAX_SEGMENTS else 0


def _put_tables(counts, symbols, tables):
    """(counts, symbols) pairs into the rows of a record's counts [3 or 4, 16] and symbols [3 or 4, 256]."""
    for t, (c, s) in enumerate(tables):
        counts[t] = np.frombuffer(bytes(c), dtype=np.uint8)
        symbols[t, :len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)


def plan(files, mode: str = "RGB", order: str = "rgb", substreams="auto", segment_bytes: Optional[int] = None,
         max_rounds: Optional[int] = None, progressive: bool = False, levels: bool = True, all_layouts: bool = False, _parsed=None,
         all_scans: bool = False, scan_substreams=False):
    """Host only (no device is touched): files -> ``(parsed, table, header)``: :func:`parse_jpeg` of every file and the table
    ``attwarp_jpegdec_plan_ex`` writes for them, which depends on the headers and the files' lengths alone.  ``substreams``:
    "auto" / True cut every marker-less file of at least two segments into ``segment_bytes`` (a power of two in 32..512,
    default :data:`SEGMENT_BYTES`) decoded by one lane each, in at most ``max_rounds`` rounds (default :data:`MAX_ROUNDS`);
    False plans every file for the sequential decode, one wave per restart interval.  Each ``parsed[i]["segments"]`` holds
    the segments planned (0: sequential).

    ``progressive=True`` also plans a list of progressive files (all of the list: :class:`JpegFiles` splits a mixed one)
    through ``attwarp_jpegdec_plan_scans``: every scan of every file, one entropy launch per dependency level
    (``parsed[i]["levels"]``).  ``levels=False`` plans one launch per scan position in file order instead; pixels, statuses
    and coefficients do not depend on it (for tests).  Progressive files take no sub-streams.

    ``all_layouts=True`` also plans a list of files of the other layouts (``parsed[i]["layout"]``; again all of the list)
    through ``attwarp_jpegdec_plan_layouts``, sub-streams included.  A list without such a file gets the table it gets
    without the keyword, byte for byte.

    ``all_scans=True`` (implies both) also plans a list of progressive files of the other layouts and sequential files of
    several scans (``parsed[i]["scanned"]``; again all of the list) through ``attwarp_jpegdec_plan_layout_scans``: every scan
    of every file over the layout family's image records, one entropy launch per dependency level; ``levels`` as above.  A
    list without such a file gets the table it gets with ``progressive=True, all_layouts=True``, byte for byte.

    ``scan_substreams``: "auto" / True (opt-in, default False; "auto" cuts the scan kinds of :data:`AUTO_SCAN_KINDS`, the ones
    measured to pay, True all four) plan a list of plain progressive files through
    ``attwarp_jpegdec_plan_scans_ex``: every scan that is ONE unit (no restart markers) and at least two segments of
    ``segment_bytes`` long (at most 16384 of them) is cut into such segments, its length known from the marker walk, and
    decoded by one lane per segment in front of its level's entropy launch; ``max_rounds`` caps the rounds
    of the first passes.  ``parsed[i]["scan_segments"]`` holds the segments planned per scan (0: one lane).  Pixels and
    statuses do not depend on it; False gives the table of ``attwarp_jpegdec_plan_scans``, byte for byte.  With
    ``all_scans=True`` the marker-less PROGRESSIVE scans of the files planned through the layout records are cut in the same
    way through ``attwarp_jpegdec_plan_layout_scans_ex`` ("auto": the kinds of
    :data:`AUTO_LAYOUT_SCAN_KINDS`); the scans of a sequential file of several scans are never cut (route 0), and False gives
    the table of ``attwarp_jpegdec_plan_layout_scans``, byte for byte."""
    if not (scan_substreams is True or scan_substreams is False or (isinstance(scan_substreams, str) and scan_substreams == "auto")):
        raise ValueError("jpeg: scan_substreams must be 'auto', True or False")
    if mode not in _lib.JPEGDEC_MODE_IDS or order not in _ORDERS:
        raise ValueError(f"jpeg: mode must be one of {sorted(_lib.JPEGDEC_MODE_IDS)}, order one of {sorted(_ORDERS)}")
    sb, mr = _substream_plan(substreams, segment_bytes, max_rounds)
    files = [file_bytes(f) for f in files]
    parsed = _parsed if _parsed is not None else [parse_jpeg(f, i, progressive, all_layouts, all_scans) for i, f in enumerate(files)]
    B = len(parsed)
    prog = [bool(p.get("progressive")) for p in parsed]
    scanned = [bool(p.get("scanned")) for p in parsed]
    if any(scanned) and not all(scanned):
        raise ValueError("jpeg: plan() takes files of one kind; JpegFiles splits a list that holds several kinds")
    other = [bool(p.get("layout") or p.get("scanned")) for p in parsed]
    if any(prog) and not all(prog) and not any(other):
        raise ValueError("jpeg: plan() takes baseline files or progressive files; JpegFiles splits a list that holds both")
    if any(other) and not all(other):
        raise ValueError("jpeg: plan() takes baseline files, progressive files or files of the other layouts; JpegFiles splits a "
                         "list that holds several kinds")
    rec = np.zeros(B, dtype=np.dtype(_lib.JpegDecLayoutImage) if any(other) else _IMAGE_DTYPE)
    lens = [len(memoryview(f).cast("B")) - p["data_off"] for f, p in zip(files, parsed)]
    rec["stream_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    rec["stream_len"] = lens
    for key, name in (("H", "H"), ("W", "W"), ("ncomp", "ncomp"), ("restart_interval", "ri")) + ((("hs", "hs"), ("vs", "vs")) if not any(other) else ()):
        rec[key] = [p[name] for p in parsed]
    if any(other):
        rec["color"] = [_lib.JPEGDEC_COLOR_IDS[p["color"]] for p in parsed]
        for b, p in enumerate(parsed):
            rec["h"][b, :p["ncomp"]] = [h for h, _ in p["samp"]]
            rec["v"][b, :p["ncomp"]] = [v for _, v in p["samp"]]
    rec["mode"] = _lib.JPEGDEC_MODE_IDS[mode]; rec["order"] = _ORDERS[order]
    for b, p in enumerate(parsed):                          # (a progressive file's Huffman tables belong to its scans: none here)
        rec["qt"][b, :p["ncomp"]] = p["qt"]
        _put_tables(rec["dc_counts"][b], rec["dc_symbols"][b], p["dc"])
        _put_tables(rec["ac_counts"][b], rec["ac_symbols"][b], p["ac"])
    rp = ctypes.c_void_p(rec.ctypes.data)
    size, planner = ("attwarp_jpegdec_table_bytes", rp, B), ("attwarp_jpegdec_plan_ex", rp, B, TABLE, sb, mr)
    if any(other):
        size, planner = ("attwarp_jpegdec_layouts_table_bytes", rp, B), ("attwarp_jpegdec_plan_layouts", rp, B, TABLE, sb, mr)
    if any(scanned):
        scans = [(b, s) for b, p in enumerate(parsed) for s in p["scans"]]
        srec = np.zeros(len(scans), dtype=np.dtype(_lib.JpegDecLayoutScan))
        srec["image"] = [b for b, _ in scans]
        srec["ncomp"] = [len(s["comps"]) for _, s in scans]
        srec["comp"] = [(s["comps"] + [0, 0, 0])[:4] for _, s in scans]
        for key, name in (("ss", "ss"), ("se", "se"), ("ah", "ah"), ("al", "al"), ("restart_interval", "ri")):
            srec[key] = [s[name] for _, s in scans]
        srec["sequential"] = [1 if s.get("sequential") else 0 for _, s in scans]
        srec["stream_off"] = [s["off"] - parsed[b]["data_off"] for b, s in scans]
        for i, (_, s) in enumerate(scans):
            nc = len(s["comps"])                            # a sequential scan: its DC tables, then its AC tables
            dc = s["tables"][:nc] if s.get("sequential") else s["tables"] if s["ss"] == 0 else []
            ac = s["tables"][nc:] if s.get("sequential") else s["tables"] if s["ss"] > 0 else []
            _put_tables(srec["dc_counts"][i], srec["dc_symbols"][i], dc)
            _put_tables(srec["ac_counts"][i], srec["ac_symbols"][i], ac)
        size = ("attwarp_jpegdec_layout_scans_table_bytes", rp, B, len(scans))
        planner = ("attwarp_jpegdec_plan_layout_scans", rp, B, srec.ctypes.data, len(scans), TABLE, 1 if levels else 0)
        sb = 0                                              # files planned scan by scan take no sub-streams of the whole file
        ssb = 0
        if scan_substreams is not False:                    # their marker-less progressive scans do, each on its own
            ssb, smr = _substream_plan(True, segment_bytes, max_rounds)
            cuts = [_layout_scan_cut(s, scan_substreams) for _, s in scans]
            slen = np.array([s["end"] - s["off"] if c else 0 for (_, s), c in zip(scans, cuts)], dtype=np.uint64)
            size = ("attwarp_jpegdec_layout_scans_table_bytes_ex", rp, B, len(scans), ssb, smr)
            planner = ("attwarp_jpegdec_plan_layout_scans_ex", rp, B, srec.ctypes.data, len(scans), TABLE, 1 if levels else 0, ssb, smr,
                       slen.ctypes.data)
            for p in parsed:                                # (only with the keyword: without it the parse is what it was)
                p["scan_segments"] = [scan_segments(s["end"] - s["off"], s["units"], ssb) if _layout_scan_cut(s, scan_substreams) else 0
                                      for s in p["scans"]]
    if any(prog):
        scans = [(b, s) for b, p in enumerate(parsed) for s in p["scans"]]
        srec = np.zeros(len(scans), dtype=np.dtype(_lib.JpegDecScan))
        srec["image"] = [b for b, _ in scans]
        srec["ncomp"] = [len(s["comps"]) for _, s in scans]
        srec["comp"] = [(s["comps"] + [0, 0])[:3] for _, s in scans]
        for key, name in (("ss", "ss"), ("se", "se"), ("ah", "ah"), ("al", "al"), ("restart_interval", "ri")):
            srec[key] = [s[name] for _, s in scans]
        srec["stream_off"] = [s["off"] - parsed[b]["data_off"] for b, s in scans]
        for i, (_, s) in enumerate(scans):
            _put_tables(srec["counts"][i], srec["symbols"][i], s["tables"])
        size = ("attwarp_jpegdec_scans_table_bytes", rp, B, len(scans))
        planner = ("attwarp_jpegdec_plan_scans", rp, B, srec.ctypes.data, len(scans), TABLE, 1 if levels else 0)
        sb = 0                                              # progressive files take no sub-streams of the whole file
        ssb = 0
        cuts = [False] * len(scans)
        if scan_substreams is not False:                    # their marker-less scans do, each on its own
            ssb, smr = _substream_plan(True, segment_bytes, max_rounds)
            # "auto": only the kinds that pay (AUTO_SCAN_KINDS); a scan of another kind is planned with no data, so it is not cut
            cuts = [scan_substreams is True or scan_kind(s) in AUTO_SCAN_KINDS for _, s in scans]
            slen = np.array([s["end"] - s["off"] if c else 0 for (_, s), c in zip(scans, cuts)], dtype=np.uint64)
            size = ("attwarp_jpegdec_scans_table_bytes_ex", rp, B, len(scans), ssb, smr)
            planner = ("attwarp_jpegdec_plan_scans_ex", rp, B, srec.ctypes.data, len(scans), TABLE, 1 if levels else 0, ssb, smr, slen.ctypes.data)
        for p in parsed:
            p["scan_segments"] = [scan_segments(s["end"] - s["off"], s["units"], ssb) if scan_substreams is True or scan_kind(s) in AUTO_SCAN_KINDS
                                  else 0 for s in p["scans"]]
    table, header = planned_table(size, planner, _lib.JpegDecHeader, ValueError, "jpeg: ", wrap_plan=True)
    for p, n in zip(parsed, lens):
        nseg = -(-n // sb) if sb else 0
        p["segments"] = nseg if p["units"] == 1 and n >= 2 * sb and nseg <= MAX_SEGMENTS else 0
    return parsed, table, header


def _per_part(method):
    """The one dispatch of a list that holds both kinds: a per-image answer comes from the parts, in input order."""
    def dispatch(self):
        if self.parts is None:
            return method(self)
        return scattered(self.B, ((idx, dispatch(part)) for idx, part in self.parts))
    dispatch.__doc__ = method.__doc__
    return dispatch


class JpegFiles(FileBatch):
    """One batch of JPEG files planned for ``attwarp_jpegdec_decode``: ``files`` is a list of bytes / bytearray / memoryview /
    paths.  The host walks the marker segments (:func:`parse_jpeg`), packs everything behind every file's SOS header back
    to back and uploads it, with the table, in ONE transfer; the plan depends only on what the headers say.  ``mode``:
    "RGB" (what ``Image.open(f).convert("RGB")`` gives), "L" (``.convert("L")``) or "keep" (grey files one channel, colour
    files three); ``order="bgr"`` swaps a 3-channel result.  ``out``: a uint8 device buffer of at least :attr:`out_bytes`
    bytes.  ``substreams``, ``segment_bytes``, ``max_rounds``: see :func:`plan`; ``substreams=False`` decodes every file
    sequentially.  Pixels and statuses do not depend on them.  Unsupported files raise ValueError before any launch.

    ``progressive=True`` also takes progressive files, alone or mixed with baseline files.  A list of one
    kind is one plan and one output buffer.  A mixed list is two plans, one per kind (:attr:`parts`: ``[(indices, JpegFiles
    of that kind)]``), each with its own transfer and output buffer (``out`` must then be None); :meth:`views` and the
    status come back in input order, and the baseline files take exactly the path of a ``progressive=False`` call on them
    alone.  ``levels``: see :func:`plan`.

    ``all_layouts=True`` also takes sequential files of four components (CMYK, YCCK), RGB-coded files and every sampling
    layout libjpeg decodes.  They are a third kind with a plan of its own, so a list may hold all three;
    "keep" gives such a file its own channels (four: Pillow's ``CMYK`` bytes).  A list without such a file takes exactly the
    path it takes without the keyword.

    ``all_scans=True`` is the one switch for a folder somebody else made: it implies both keywords and also takes what both
    refuse, progressive files of the other layouts and sequential files of several scans.  Those are a
    fourth kind with a plan of its own; only files the three other kinds refuse take it, the other parts plan and launch
    exactly as with ``progressive=True, all_layouts=True``, and views and statuses come back in input order.

    ``scan_substreams="auto"`` / True (opt-in) cuts the marker-less scans of the plain progressive files and, with
    ``all_scans``, the marker-less progressive scans of the files of the fourth kind (never a sequential scan) into segments of
    ``segment_bytes`` decoded by one lane each (:func:`plan`): one more launch in front of the entropy launch
    of every level that holds such a scan, constant per plan.  Pixels and statuses do not depend on it;
    :meth:`scan_substream_info` tells what the device did per scan."""

    def __init__(self, files, mode: str = "RGB", order: str = "rgb", out: Optional[torch.Tensor] = None, device=None,
                 substreams="auto", segment_bytes: Optional[int] = None, max_rounds: Optional[int] = None,
                 progressive: bool = False, levels: bool = True, all_layouts: bool = False, all_scans: bool = False, scan_substreams=False):
        files = [file_bytes(f) for f in files]
        if not files:
            raise ValueError("JpegFiles: empty batch")
        if not (scan_substreams is True or scan_substreams is False or (isinstance(scan_substreams, str) and scan_substreams == "auto")):
            raise ValueError("jpeg: scan_substreams must be 'auto', True or False")
        self.parts, self.B, self.mode, self.order = None, len(files), mode, order
        progressive, all_layouts = progressive or all_scans, all_layouts or all_scans
        pre = [parse_jpeg(f, i, progressive, all_layouts, all_scans) for i, f in enumerate(files)] if progressive or all_layouts else None
        # baseline, progressive, other layout, scans of any layout
        which = [1 if p.get("progressive") else 2 if p.get("layout") else 3 if p.get("scanned") else 0 for p in pre or []]
        self.progressive, self.all_layouts = bool(which) and set(which) == {1}, bool(which) and set(which) == {2}
        self.all_scans = bool(which) and set(which) == {3}
        if len(set(which)) > 1:
            if out is not None:
                raise ValueError("JpegFiles: a list of baseline and progressive files decodes into two buffers; out must be None"
                                 if 2 not in which else "JpegFiles: a list of several kinds of files decodes into one buffer per kind; out must be None")
            self.parts = [(idx, JpegFiles([files[i] for i in idx], mode, order, None, device, substreams, segment_bytes, max_rounds, kind == 1, levels,
                                          all_layouts, kind == 3, scan_substreams))
                          for kind, idx in split_indices(which, (0, 1, 2, 3))]
            first = self.parts[0][1]
            self._dev, self.segment_bytes, self.max_rounds = first._dev, first.segment_bytes, first.max_rounds
            self.parsed, self.shapes = (scattered(self.B, ((idx, getattr(part, name)) for idx, part in self.parts)) for name in ("parsed", "shapes"))
            self.compressed_bytes = sum(part.compressed_bytes for _, part in self.parts)
            with torch.cuda.device(self._dev):
                self.status = torch.empty(self.B, device=self._dev, dtype=torch.int32)
                self._index = [torch.tensor(idx, device=self._dev, dtype=torch.int64) for idx, _ in self.parts]
            return
        self._entry = ("attwarp_jpegdec_decode_scans" if self.progressive else "attwarp_jpegdec_decode_layouts" if self.all_layouts
                       else "attwarp_jpegdec_decode_layout_scans" if self.all_scans else "attwarp_jpegdec_decode")
        self.parsed, self.table_host, self.header = plan(files, mode, order, substreams, segment_bytes, max_rounds, progressive, levels, all_layouts, pre,
                                                         all_scans, scan_substreams)
        self._scan_info_off = int(_lib.load().attwarp_jpegdec_scan_info_offset(self.table_host.ctypes.data)) if self.progressive or self.all_scans else 0
        self.segment_bytes, self.max_rounds = _substream_plan(substreams, segment_bytes, max_rounds)      # (0, 0): off
        self._info_off = int(_lib.load().attwarp_jpegdec_info_offset(self.table_host.ctypes.data))
        self._dev = indexed_device(device, out)
        self.shapes = [(p["H"], p["W"], 1 if mode == "L" else 3 if mode == "RGB" else p["ncomp"]) for p in self.parsed]
        srcs = [np.frombuffer(f, dtype=np.uint8)[p["data_off"]:] for f, p in zip(files, self.parsed)]
        self.compressed_bytes = int(self.header.stream_bytes)

        def fill(body):
            at = 0
            for s in srcs:
                body[at:at + s.size] = s
                at += s.size
        self._to_device(fill, out)

    @property
    def out_bytes(self) -> int:
        """Bytes of all decoded images, back to back: the capacity ``out`` needs (a mixed list: of both its buffers)."""
        return sum(part.out_bytes for _, part in self.parts) if self.parts else super().out_bytes

    views = _per_part(FileBatch.views)

    def units(self) -> List[int]:
        """Decoding units (restart intervals) planned per image, from the headers alone: one wave each."""
        return [p["units"] for p in self.parsed]

    def levels(self) -> List[int]:
        """Dependency levels of each image's scans, from the headers alone (0 for a baseline file): the entropy launches of a
        progressive plan number the largest of them."""
        return [1 + max(p["levels"]) if p.get("progressive") or p.get("scanned") else 0 for p in self.parsed]

    @_per_part
    def coefficients(self) -> List[torch.Tensor]:
        """After a :meth:`run`: per image the int16 [blocks, 64] coefficients as they lie in scratch (views); for a file planned
        scan by scan over the layout records (``all_scans``) a list of one int16 [block rows, blocks per row, 64] view per
        component, the padded planes.  For tests; not for one-scan files of the other layouts."""
        if self.all_layouts:
            raise ValueError("JpegFiles.coefficients: not offered for files of the other layouts")
        ims = np.frombuffer(self.table_host, dtype=np.uint8)
        out = []
        if self.all_scans:
            for b, p in enumerate(self.parsed):
                at = int(self.header.off_images) + b * _lib.JPEGDEC_LAYOUT_RECORD_BYTES
                off = int(ims[at + 8:at + 16].view(np.uint64)[0])
                mcux, mcuy = -(-p["W"] // (8 * p["hs"])), -(-p["H"] // (8 * p["vs"]))
                planes = []
                for h, v in p["samp"]:
                    nb = mcux * h * mcuy * v
                    planes.append(self.scratch[off:off + nb * 128].view(torch.int16).view(mcuy * v, mcux * h, 64))
                    off += nb * 128
                out.append(planes)
            return out
        for b, p in enumerate(self.parsed):
            at = int(self.header.off_images) + b * _lib.JPEGDEC_RECORD_BYTES
            coef_off = int(ims[at + 8:at + 16].view(np.uint64)[0])
            blocks = -(-p["W"] // (8 * p["hs"])) * -(-p["H"] // (8 * p["vs"])) * (p["hs"] * p["vs"] + p["ncomp"] - 1)
            out.append(self.scratch[coef_off:coef_off + blocks * 128].view(torch.int16).view(blocks, 64))
        return out

    def substreams(self) -> List[int]:
        """Segments planned per image, from the headers and the files' lengths alone; 0: the image is decoded sequentially
        (it has restart intervals, is shorter than two segments, is progressive, or sub-streams are off)."""
        return [p["segments"] for p in self.parsed]

    @_per_part
    def substream_info(self) -> List[tuple]:
        """After a :meth:`run` (synchronises): per image ``(segments, rounds, accepted)`` as the device left them: the
        segments planned, the rounds its workgroup ran, and 1 if the sub-streams decoded the image, 0 if the sequential
        decode did.  For measurements and tests."""
        raw = self.scratch[self._info_off:self._info_off + self.B * 16].cpu().numpy().view(np.uint32).reshape(self.B, 4)
        return [(int(r[0]), int(r[1]), int(r[2])) for r in raw]

    @_per_part
    def scan_substream_info(self) -> List[list]:
        """After a :meth:`run` (synchronises): per image a list, in file order, of ``(route, segments, rounds, accepted)`` per
        scan as the device left them: route 0 for a scan on one lane, else 1 DC first pass, 2 DC refinement, 3 AC first pass,
        4 AC refinement; the segments planned; the rounds of a first pass; 1 if the segments decoded the scan, 0 if the
        one-lane route did.  A plan without ``scan_substreams`` has no such records: all zeros; a file of one scan (baseline
        or another layout) has no scans here: an empty list.  For measurements and tests."""
        if not (self.progressive or self.all_scans):
            return [[] for _ in self.parsed]
        return self._scan_records(slice(0, 4))

    def _scan_records(self, fields):
        n = sum(len(p["scans"]) for p in self.parsed)
        raw = np.zeros((n, 8), np.uint32)
        if self._scan_info_off:
            raw = self.scratch[self._scan_info_off:self._scan_info_off + n * 32].cpu().numpy().view(np.uint32).reshape(n, 8)
        out, at = [], 0
        for p in self.parsed:
            out.append([tuple(int(x) for x in r[fields]) for r in raw[at:at + len(p["scans"])]])
            at += len(p["scans"])
        return out

    @_per_part
    def scan_substream_ticks(self) -> List[list]:
        """After a :meth:`run` (synchronises): per image and scan, beside :meth:`scan_substream_info`, the 100 MHz ticks its
        workgroup spent in its three parts: a first pass: rounds, sums and checks, write; a refinement: counts and masks,
        skim (a DC refinement: none), write.  Zeros for a scan on one lane.  For measurements."""
        if not (self.progressive or self.all_scans):
            return [[] for _ in self.parsed]
        return self._scan_records(slice(4, 7))

    @_per_part
    def restarts(self) -> List[int]:
        """After a :meth:`run` (synchronises): restart markers the device found in front of each image's data end; units - 1
        in a file that decodes (a progressive file: over all its scans).  For measurements and tests."""
        st = self.scratch[:self.B * 16].cpu().numpy().view(np.uint32).reshape(self.B, 4)
        return [int(r[3]) for r in st]

    def run(self):
        """Five launches on the current stream -> ``(views, status)``: the images, and an int32 [B] device tensor (0: ok,
        else ``STATUS_NAMES[code]``; such an image's pixels are unspecified).  No host synchronisation and no host-dependent
        argument: capturable in a graph.  A progressive plan takes one clear, one restart scan, one entropy launch per
        dependency level, IDCT and colour; a mixed list runs its two plans one after the other."""
        if self.parts is None:
            return super().run()
        with torch.cuda.device(self._dev):
            for (_, part), index in zip(self.parts, self._index):
                self.status.index_copy_(0, index, part.run()[1])
        return self.views(), self.status


def decode_jpeg(files, mode: str = "RGB", order: str = "rgb", device=None, substreams="auto", progressive: bool = False,
                all_layouts: bool = False, all_scans: bool = False, scan_substreams=False,
                segment_bytes: Optional[int] = None) -> List[torch.Tensor]:
    """JPEG files (bytes-like or paths) -> uint8 [H_i, W_i, C] GPU tensors, views into one packed buffer.  OSError names the
    first file the device rejects (Pillow raises OSError for such files too); ValueError for what is not decoded at all.
    ``substreams``: see :func:`plan`.  ``progressive=True`` also decodes progressive files, alone or among baseline files
    (:class:`JpegFiles`); without it such a file raises ValueError.  ``all_layouts=True`` also decodes CMYK / YCCK files,
    RGB-coded files and every sampling layout libjpeg decodes; without it such a file raises ValueError.  ``all_scans=True``
    implies both and also decodes progressive files of those layouts and sequential files of several scans: the one switch
    for a folder somebody else made.  ``scan_substreams``, ``segment_bytes``: see :func:`plan`; pixels do not depend on them."""
    views, status = JpegFiles(files, mode, order, device=device, substreams=substreams, segment_bytes=segment_bytes, progressive=progressive,
                              all_layouts=all_layouts, all_scans=all_scans, scan_substreams=scan_substreams).run()
    raise_first_broken(status, STATUS_NAMES, "jpeg")
    return views


def read_jpeg(paths, mode: str = "RGB", order: str = "rgb", device=None, substreams="auto", progressive: bool = False,
              all_layouts: bool = False, all_scans: bool = False, scan_substreams=False,
              segment_bytes: Optional[int] = None) -> List[torch.Tensor]:
    """:func:`decode_jpeg` of the files at ``paths``."""
    return decode_jpeg([os.fspath(p) for p in paths], mode, order, device, substreams, progressive, all_layouts, all_scans, scan_substreams,
                       segment_bytes)


# ---- encoding ---------------------------------------------------------------------------------------------------------------
SUBSAMPLINGS = tuple(_lib.JPEGENC_SUBSAMPLING_IDS)
JPEGENC_UNIT_MCUS = _lib.JPEGENC_UNIT_MCUS              # MCUs one entropy unit (one workgroup) codes at most
JPEGENC_MAX_DIM = _lib.JPEGENC_MAX_DIM                  # W and H at most
_ENC_IMAGE_DTYPE = np.dtype(_lib.JpegEncImage)


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _enc_per_image(value, B: int, what: str, ok):
    vals = list(value) if isinstance(value, (list, tuple)) else [value] * B
    if len(vals) != B or not all(ok(v) for v in vals):
        raise ValueError(f"jpeg: {what}: one valid value or one per image expected, got {value!r}")
    return vals


class JpegBatch(ImageBatch):
    """One batch of differently sized uint8 images on the GPU, planned for ``attwarp_jpegenc_encode``: list of [H,W,3] /
    [H,W] / [H,W,1] tensors or one [B,H,W,C] tensor.  The images are referenced, not copied (any byte address, any row
    pitch): keep them alive; their CONTENT is read at every :meth:`run`, so a captured run re-encodes what they hold then.

    ``quality`` 1 .. 100, ``subsampling`` "4:4:4" / "4:2:2" / "4:2:0" (or Pillow's 0 / 1 / 2),
    ``restart_rows`` (MCU rows per restart interval, 0: no restart markers), ``order`` "rgb" / "bgr": one value or one per
    image.  The defaults are Pillow's, so a bare call gives the file of ``Image.save``; ``restart_rows=1`` costs two bytes
    per MCU row and is what this project's own reader (:func:`decode_jpeg`) decodes fastest.  ``out``: a uint8 device buffer
    of at least :attr:`bound` bytes.  ``optimize`` (one value or one per image, default False): the image's own Huffman
    tables, built on the GPU from its symbol counts the way libjpeg builds them, so that the file is byte for byte that of
    ``Image.save(..., optimize=True)``: the same pixels in fewer bytes, for three more launches.  Images
    with and without it share a batch; without it in any image the call is what it was before the keyword existed.
    ``progressive`` (one value or one per image, default False): the file of ``Image.save(..., progressive=True)``, byte for
    byte: SOF2, libjpeg's ten scans (six for grey), each behind the DHT of its own optimal table; it implies optimised
    tables whatever ``optimize`` says, as libjpeg does, and with ``restart_rows`` every scan restarts at its own rows, which
    is the kind of progressive file :func:`decode_jpeg` reads fast.  Plain, optimised and progressive
    images share a batch; with the keyword absent or all False the call is what it was before the keyword existed.
    CMYK, EXIF / ICC / dpi, custom tables and custom scan scripts do not exist here.  Limits raise ValueError before any launch.

    A grey image ignores ``subsampling`` and is always the file of a bare ``Image.save`` of an "L" image, factors 1 x 1.
    Pillow, GIVEN the keyword for an "L" image, writes its factors into the component's SOF0 entry (one byte: 0x21 or 0x22
    in place of 0x11) and the same scan data, so for grey images ``encode_jpeg(..., subsampling=s)`` differs in that one
    byte from ``Image.save(..., subsampling=s)`` unless s is "4:4:4".

    :meth:`run` takes seven launches, three more with an optimised image and eight more with a progressive one (the lists at
    the top of csrc/jpegenc.hip)."""

    _who, _prefix, _dtype_error, _entry, _max_side = "JpegBatch", "jpeg", ValueError, "attwarp_jpegenc_encode", JPEGENC_MAX_DIM

    @staticmethod
    def _too_large(H: int, W: int, C: int) -> str:
        return f"jpeg: {W} x {H} exceeds JPEGENC_MAX_DIM = {JPEGENC_MAX_DIM}"

    def __init__(self, images, quality=75, subsampling="4:2:0", restart_rows=0, order="rgb", out: Optional[torch.Tensor] = None,
                 optimize=False, progressive=False):
        images = self._views(images)
        if not images:
            raise ValueError("JpegBatch: empty batch")
        B = len(images)
        ids = {**_lib.JPEGENC_SUBSAMPLING_IDS, **{v: v for v in _lib.JPEGENC_SUBSAMPLING_IDS.values()}}
        qualities = _enc_per_image(quality, B, "quality (1 .. 100)", lambda v: _is_int(v) and 1 <= v <= 100)
        subs = _enc_per_image(subsampling, B, f"subsampling ({', '.join(SUBSAMPLINGS)})", lambda v: (isinstance(v, str) or _is_int(v)) and v in ids)
        rows = _enc_per_image(restart_rows, B, "restart_rows (0 or more)", lambda v: _is_int(v) and 0 <= v < 1 << 16)
        orders = _enc_per_image(order, B, "order ('rgb' / 'bgr')", lambda v: v in _ORDERS)
        self.optimize = [bool(v) for v in _enc_per_image(optimize, B, "optimize (True / False)", lambda v: isinstance(v, (bool, np.bool_)))]
        self.progressive = [bool(v) for v in _enc_per_image(progressive, B, "progressive (True / False)", lambda v: isinstance(v, (bool, np.bool_)))]
        rec = self._records(images, _ENC_IMAGE_DTYPE, [_ORDERS[o] for o in orders])
        rec["quality"] = [int(q) for q in qualities]
        rec["subsampling"] = [int(ids[s]) for s in subs]
        rec["restart_rows"] = [int(r) for r in rows]
        rp = ctypes.c_void_p(rec.ctypes.data)
        flags = np.asarray(self.optimize, np.int32)
        fp = ctypes.c_void_p(flags.ctypes.data) if flags.any() else None        # NULL: the plain planner's table
        pflags = np.asarray(self.progressive, np.int32)
        if pflags.any():                                                        # (none: the optimised planner's table, as before)
            pp = ctypes.c_void_p(pflags.ctypes.data)
            planners = ("attwarp_jpegenc_table_bytes_prog", rp, B, fp, pp), ("attwarp_jpegenc_plan_prog", rp, B, fp, pp, TABLE)
        else:
            planners = ("attwarp_jpegenc_table_bytes_ex", rp, B, fp), ("attwarp_jpegenc_plan_ex", rp, B, fp, TABLE)
        self._to_device(*planned_table(*planners, _lib.JpegEncHeader, ValueError, "JpegBatch: "), out)

    @property
    def units(self) -> int:
        return int(self.header.nunits)


def encode_jpeg(images, quality=75, subsampling="4:2:0", restart_rows=0, order="rgb", optimize=False, progressive=False) -> List[bytes]:
    """uint8 GPU images (list of [H,W,3] / [H,W] of any sizes, or [B,H,W,C]) -> the bytes of one JPEG file each, what
    ``Image.fromarray(a).save(f, "JPEG", quality=..., subsampling=..., restart_marker_rows=..., optimize=..., progressive=...)`` writes.  Raw pixels never
    leave the device.  See :class:`JpegBatch` for the keywords."""
    return download(*JpegBatch(images, quality, subsampling, restart_rows, order, optimize=optimize, progressive=progressive).run())


def write_jpeg(paths, images, quality=75, subsampling="4:2:0", restart_rows=0, order="rgb", optimize=False, progressive=False) -> None:
    """:func:`encode_jpeg`, each file written to its path."""
    n = images.shape[0] if isinstance(images, torch.Tensor) else len(images)
    write_files("write_jpeg", paths, n, lambda: encode_jpeg(images, quality, subsampling, restart_rows, order, optimize, progressive))
