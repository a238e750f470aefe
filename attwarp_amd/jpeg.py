"""Baseline JPEG files of a whole ragged batch, decoded on the GPU (csrc/jpegdec.hip): what the reference
does per file with ``Image.open(path).convert('RGB')`` (main_batched.py:95-98, main.py:148-152, functions.py:36,
MN/dataloader.py:216,368).  Only compressed bytes cross to the device; the pixels are Pillow's, bit for bit.
SOF0 / SOF1, 8 bits, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, any restart interval.
With ``progressive=True`` (off by default) also SOF2: the host walks every scan of the file, the device runs one entropy
launch per dependency level of the scans; baseline and progressive files may share a list.
"""
from __future__ import annotations

import ctypes
import os
import struct
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

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


def scan_levels(scans) -> List[int]:
    """The dependency level of every scan of one file: 0 if no earlier scan shares a component with it and overlaps its band,
    else 1 + the largest level among those.  Scans of one level write disjoint coefficients."""
    lv = []
    for i, a in enumerate(scans):
        deps = [lv[j] for j, e in enumerate(scans[:i]) if set(a["comps"]) & set(e["comps"]) and e["ss"] <= a["se"] and a["ss"] <= e["se"]]
        lv.append(1 + max(deps) if deps else 0)
    return lv


def parse_jpeg(data, index: int = 0, progressive: bool = False) -> dict:
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
    or at the file's end).  A file that ends INSIDE a scan is not refused: the device gives it a status."""
    mv = memoryview(data).cast("B")
    n = len(mv)
    sof, scans, sent, latched, markers, cut = 0, [], None, {}, None, False

    def bad(what):
        return ValueError(f"jpeg: file {index}: {what}")

    def need(upto):
        if upto > n:
            raise OSError(f"jpeg: file {index}: the file ends inside its headers")

    need(2)
    if mv[0] != 0xFF or mv[1] != 0xD8:
        raise bad("bad signature")
    pos = 2
    qts, dcs, acs = {}, {}, {}
    frame, ri, jfif, adobe = None, 0, False, None
    while True:
        if scans and pos + 1 >= n:
            break                                         # the file ends behind a scan: complete or not, below
        need(pos + 1)
        if mv[pos] != 0xFF:
            raise bad("a marker was expected")
        while mv[pos] == 0xFF:                            # fill bytes
            pos += 1
            if scans and pos >= n:
                break
            need(pos + 1)
        if scans and pos >= n:
            break
        m = mv[pos]
        pos += 1
        if scans and m == 0xD9:
            break
        if m in _UNSUPPORTED_FRAMES and not (m == 0xC2 and progressive):
            raise bad(f"{_UNSUPPORTED_FRAMES[m]} frame (sequential Huffman only)")
        if m == 0xCC:
            raise bad("arithmetic conditioning")
        if m in (0x00, 0x01, 0xD8, 0xD9) or 0xD0 <= m <= 0xD7:
            raise bad(f"marker {m:02x} in the headers")
        if scans and (pos + 2 > n or pos + (mv[pos] << 8 | mv[pos + 1]) > n):
            break                                         # the file ends inside a segment behind a scan
        need(pos + 2)
        L = mv[pos] << 8 | mv[pos + 1]
        if L < 2:
            raise bad("segment length below 2")
        need(pos + L)
        seg = bytes(mv[pos + 2:pos + L])
        pos += L
        if m in (0xC0, 0xC1, 0xC2):
            sof = m & 3
            if frame is not None:
                raise bad("a second frame (hierarchical)")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise bad("bad frame header")
            prec, H, W, nf = struct.unpack(">BHHB", seg[:6])
            if prec != 8:
                raise bad(f"precision {prec} (8 only)")
            if H == 0 or W == 0:
                raise bad(f"size {W} x {H}")
            if nf not in (1, 3):
                raise bad(f"{nf} components (1 or 3)")
            frame = (W, H, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)])
        elif m == 0xC4:
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
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq == 1:
                    raise bad("16-bit quantisation table")
                if pq > 1 or tq > 3 or q + 65 > len(seg):
                    raise bad("bad DQT")
                t = [0] * 64
                for k in range(64):
                    t[_ZIGZAG[k]] = seg[q + 1 + k]
                qts[tq] = t
                q += 65
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
            if sof != 2:
                break
            if frame is None:
                raise bad("SOS before the frame header")
            if sent is None:
                W, H, comps = frame
                nf = len(comps)
                hs = vs = 1
                if nf == 3:
                    if adobe == 0 or (adobe is None and not jfif and bytes(c[0] for c in comps) == b"RGB"):
                        raise bad("RGB-coded file (YCbCr only)")
                    samp = [(c[1], c[2]) for c in comps]
                    if samp[1] != (1, 1) or samp[2] != (1, 1) or samp[0] not in ((1, 1), (2, 1), (2, 2)):
                        raise bad(f"sampling layout {samp} (4:4:4, 4:2:2, 4:2:0)")
                    hs, vs = samp[0]
                sent = [[None] * 64 for _ in range(nf)]     # per coefficient: the Al it was last sent with
                markers = _marker_positions(mv)
                data_off = pos
            if len(scans) >= JPEGDEC_MAX_SCANS:
                raise bad(f"more than {JPEGDEC_MAX_SCANS} scans")
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0] or not 1 <= seg[0] <= nf:
                raise bad("bad scan header")
            ns = seg[0]
            ids = [c[0] for c in comps]
            if any(seg[1 + 2 * i] not in ids for i in range(ns)):
                raise bad("the scan names a component the frame does not have")
            ci = [ids.index(seg[1 + 2 * i]) for i in range(ns)]
            if any(b <= a for a, b in zip(ci, ci[1:])):
                raise bad("the scan's components are not in frame order")
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            if ss > se or se > 63 or (ss == 0 and se != 0) or (ss > 0 and ns > 1) or al > 13 or (ah != 0 and al != ah - 1):
                raise bad(f"bad progression: Ss={ss} Se={se} Ah={ah} Al={al} in a scan of {ns} component(s)")
            tables = []
            for i, c in enumerate(ci):
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if ss > 0 and sent[c][0] is None:
                    raise bad(f"an AC scan of component {c} before its DC was sent")
                for k in range(ss, se + 1):
                    if ah == 0 and sent[c][k] is not None:
                        raise bad(f"a first pass over coefficient {k} of component {c}, which was already sent")
                    if ah != 0 and sent[c][k] != ah:
                        raise bad(f"a refinement Ah={ah} of coefficient {k} of component {c}, whose precision is {sent[c][k]}")
                    sent[c][k] = al
                if c not in latched:                        # libjpeg latches a component's table at its first scan
                    if comps[c][3] not in qts:
                        raise bad("the scan names a table never defined")
                    latched[c] = qts[comps[c][3]]
                if ss == 0 and ah == 0:
                    if td not in dcs:
                        raise bad("the scan names a table never defined")
                    tables.append(dcs[td])
                elif ss > 0:
                    if ta not in acs:
                        raise bad("the scan names a table never defined")
                    tables.append(acs[ta])
            geo = dict(W=W, H=H, hs=hs, vs=vs)
            nmcu = scan_geometry(geo, ci)[1]
            at = int(np.searchsorted(markers, pos))
            end = int(markers[at]) if at < markers.size else n
            scans.append(dict(comps=ci, ss=ss, se=se, ah=ah, al=al, ri=ri, tables=tables, off=pos, end=end,
                              units=-(-nmcu // ri) if ri else 1))
            cut = end + 1 >= n                              # nothing, or a lone FF, behind the data: the file ends inside the scan
            pos = end
    if sof == 2:
        if not scans:
            raise OSError(f"jpeg: file {index}: the file ends inside its headers")
        if not cut and any(a != 0 for row in sent for a in row):
            raise bad("incomplete progressive file: some coefficient was never sent or never reached Al = 0")
        units = sum(s["units"] for s in scans)
        blocks = -(-W // (8 * hs)) * -(-H // (8 * vs)) * (hs * vs + nf - 1)
        if units > JPEGDEC_MAX_UNITS or blocks >= JPEGDEC_MAX_BLOCKS or n - data_off >= 1 << 31:
            raise bad(f"size limit: {units} restart intervals over all scans (at most {JPEGDEC_MAX_UNITS}), {blocks} blocks (below {JPEGDEC_MAX_BLOCKS})")
        qt = [latched.get(c, qts.get(comps[c][3], [0] * 64)) for c in range(nf)]
        return dict(W=W, H=H, ncomp=nf, hs=hs, vs=vs, ri=0, qt=qt, dc=[], ac=[], data_off=data_off, units=units, progressive=True,
                    scans=scans, levels=scan_levels(scans))
    if frame is None:
        raise bad("SOS before the frame header")
    W, H, comps = frame
    nf = len(comps)
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        raise bad("bad scan header")
    if seg[0] != nf or [seg[1 + 2 * i] for i in range(nf)] != [c[0] for c in comps]:
        raise bad("the scan does not hold all components in frame order (more than one scan)")
    if tuple(seg[1 + 2 * nf:]) != (0, 63, 0):
        raise bad("spectral selection / successive approximation")
    hs = vs = 1
    if nf == 3:
        if adobe == 0 or (adobe is None and not jfif and bytes(c[0] for c in comps) == b"RGB"):
            raise bad("RGB-coded file (YCbCr only)")
        samp = [(c[1], c[2]) for c in comps]
        if samp[1] != (1, 1) or samp[2] != (1, 1) or samp[0] not in ((1, 1), (2, 1), (2, 2)):
            raise bad(f"sampling layout {samp} (4:4:4, 4:2:2, 4:2:0)")
        hs, vs = samp[0]
    qt, dc, ac = [], [], []
    for i, c in enumerate(comps):
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if c[3] not in qts or td not in dcs or ta not in acs:
            raise bad("the scan names a table never defined")
        qt.append(qts[c[3]]); dc.append(dcs[td]); ac.append(acs[ta])
    mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
    units = -(-mcus // ri) if ri else 1
    blocks = mcus * (hs * vs + nf - 1)
    if units > JPEGDEC_MAX_UNITS or blocks >= JPEGDEC_MAX_BLOCKS or n - pos >= 1 << 31:
        raise bad(f"size limit: {units} restart intervals (at most {JPEGDEC_MAX_UNITS}), {blocks} blocks (below {JPEGDEC_MAX_BLOCKS})")
    return dict(W=W, H=H, ncomp=nf, hs=hs, vs=vs, ri=ri, qt=qt, dc=dc, ac=ac, data_off=pos, units=units)


def _file_bytes(f):
    if isinstance(f, (str, os.PathLike)):
        with open(f, "rb") as fh:
            return fh.read()
    return f


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


def plan(files, mode: str = "RGB", order: str = "rgb", substreams="auto", segment_bytes: Optional[int] = None,
         max_rounds: Optional[int] = None, progressive: bool = False, levels: bool = True, _parsed=None):
    """Host only (no device is touched): files -> ``(parsed, table, header)``: :func:`parse_jpeg` of every file and the table
    ``attwarp_jpegdec_plan_ex`` writes for them, which depends on the headers and the files' lengths alone.  ``substreams``:
    "auto" / True cut every marker-less file of at least two segments into ``segment_bytes`` (a power of two in 32..512,
    default :data:`SEGMENT_BYTES`) decoded by one lane each, in at most ``max_rounds`` rounds (default :data:`MAX_ROUNDS`);
    False plans every file for the sequential decode, one wave per restart interval.  Each ``parsed[i]["segments"]`` holds
    the segments planned (0: sequential).

    ``progressive=True`` also plans a list of progressive files (all of the list: :class:`JpegFiles` splits a mixed one)
    through ``attwarp_jpegdec_plan_scans``: every scan of every file, one entropy launch per dependency level
    (``parsed[i]["levels"]``).  ``levels=False`` plans one launch per scan position in file order instead; pixels, statuses
    and coefficients do not depend on it (for tests).  Progressive files take no sub-streams."""
    if mode not in _lib.JPEGDEC_MODE_IDS or order not in _ORDERS:
        raise ValueError(f"jpeg: mode must be one of {sorted(_lib.JPEGDEC_MODE_IDS)}, order one of {sorted(_ORDERS)}")
    sb, mr = _substream_plan(substreams, segment_bytes, max_rounds)
    files = [_file_bytes(f) for f in files]
    parsed = _parsed if _parsed is not None else [parse_jpeg(f, i, progressive) for i, f in enumerate(files)]
    B = len(parsed)
    prog = [bool(p.get("progressive")) for p in parsed]
    if any(prog) and not all(prog):
        raise ValueError("jpeg: plan() takes baseline files or progressive files; JpegFiles splits a list that holds both")
    rec = np.zeros(B, dtype=_IMAGE_DTYPE)
    lens = [len(memoryview(f).cast("B")) - p["data_off"] for f, p in zip(files, parsed)]
    rec["stream_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    rec["stream_len"] = lens
    for key, name in (("H", "H"), ("W", "W"), ("ncomp", "ncomp"), ("hs", "hs"), ("vs", "vs"), ("restart_interval", "ri")):
        rec[key] = [p[name] for p in parsed]
    rec["mode"] = _lib.JPEGDEC_MODE_IDS[mode]; rec["order"] = _ORDERS[order]
    for b, p in enumerate(parsed):
        for c in range(p["ncomp"]):
            rec["qt"][b, c] = p["qt"][c]
            if p.get("progressive"):
                continue                                    # the tables belong to the scans
            for kind, tabs in (("dc", p["dc"]), ("ac", p["ac"])):
                counts, syms = tabs[c]
                rec[kind + "_counts"][b, c] = list(counts)
                rec[kind + "_symbols"][b, c, :len(syms)] = list(syms)
    lib = _lib.load()
    rp = ctypes.c_void_p(rec.ctypes.data)
    nbytes = lib.attwarp_jpegdec_table_bytes(rp, B)
    if nbytes == 0:
        raise ValueError("jpeg: " + lib.attwarp_last_error().decode("utf-8", "replace"))
    if any(prog):
        scans = [(b, s) for b, p in enumerate(parsed) for s in p["scans"]]
        srec = np.zeros(len(scans), dtype=np.dtype(_lib.JpegDecScan))
        srec["image"] = [b for b, _ in scans]
        srec["ncomp"] = [len(s["comps"]) for _, s in scans]
        srec["comp"] = [(s["comps"] + [0, 0])[:3] for _, s in scans]
        for key, name in (("ss", "ss"), ("se", "se"), ("ah", "ah"), ("al", "al"), ("restart_interval", "ri")):
            srec[key] = [s[name] for _, s in scans]
        srec["stream_off"] = [s["off"] - parsed[b]["data_off"] for b, s in scans]
        counts_all, symbols_all = srec["counts"], srec["symbols"]
        for i, (_, s) in enumerate(scans):
            for t, (counts, syms) in enumerate(s["tables"]):
                counts_all[i, t] = np.frombuffer(bytes(counts), dtype=np.uint8)
                symbols_all[i, t, :len(syms)] = np.frombuffer(bytes(syms), dtype=np.uint8)
        nbytes = lib.attwarp_jpegdec_scans_table_bytes(rp, B, len(scans))
        if nbytes == 0:
            raise ValueError("jpeg: " + lib.attwarp_last_error().decode("utf-8", "replace"))
        table = np.empty(nbytes, dtype=np.uint8)
        try:
            call("attwarp_jpegdec_plan_scans", rp, B, srec.ctypes.data, len(scans), table.ctypes.data, nbytes, 1 if levels else 0)
        except _lib.AttWarpError as e:
            raise ValueError(f"jpeg: {e}") from None
        for p in parsed:
            p["segments"] = 0
        return parsed, table, _lib.JpegDecHeader.from_address(table.ctypes.data)
    table = np.empty(nbytes, dtype=np.uint8)
    try:
        call("attwarp_jpegdec_plan_ex", rp, B, table.ctypes.data, nbytes, sb, mr)
    except _lib.AttWarpError as e:
        raise ValueError(f"jpeg: {e}") from None
    for p, n in zip(parsed, lens):
        nseg = -(-n // sb) if sb else 0
        p["segments"] = nseg if p["units"] == 1 and n >= 2 * sb and nseg <= MAX_SEGMENTS else 0
    return parsed, table, _lib.JpegDecHeader.from_address(table.ctypes.data)


class JpegFiles:
    """One batch of JPEG files planned for ``attwarp_jpegdec_decode``: ``files`` is a list of bytes / bytearray / memoryview /
    paths.  The host walks the marker segments (:func:`parse_jpeg`), packs everything behind every file's SOS header back
    to back and uploads it, with the table, in ONE transfer; the plan depends only on what the headers say.  ``mode``:
    "RGB" (what ``Image.open(f).convert("RGB")`` gives), "L" (``.convert("L")``) or "keep" (grey files one channel, colour
    files three); ``order="bgr"`` swaps a 3-channel result.  ``out``: a uint8 device buffer of at least :attr:`out_bytes`
    bytes.  ``substreams``, ``segment_bytes``, ``max_rounds``: see :func:`plan`; ``substreams=False`` decodes every file
    sequentially.  Pixels and statuses do not depend on them.  Unsupported files raise ValueError before any launch.

    ``progressive=True`` also takes progressive files, alone or mixed with baseline files.  A list of one
    kind is one plan and one output buffer.  A mixed list is two plans, one per kind, each with its own transfer and
    output buffer (``out`` must then be None); :meth:`views` and the status come back in input order, and the baseline files
    take exactly the path of a ``progressive=False`` call on them alone.  ``levels``: see :func:`plan`."""

    def __init__(self, files, mode: str = "RGB", order: str = "rgb", out: Optional[torch.Tensor] = None, device=None,
                 substreams="auto", segment_bytes: Optional[int] = None, max_rounds: Optional[int] = None,
                 progressive: bool = False, levels: bool = True):
        from .pipeline import _upload_filled
        files = [_file_bytes(f) for f in files]
        if not files:
            raise ValueError("JpegFiles: empty batch")
        self.parts, self.progressive = None, False
        pre = [parse_jpeg(f, i, True) for i, f in enumerate(files)] if progressive else None
        if progressive and any(p.get("progressive") for p in pre):
            which = [bool(p.get("progressive")) for p in pre]
            if not all(which):
                if out is not None:
                    raise ValueError("JpegFiles: a list of baseline and progressive files decodes into two buffers; out must be None")
                self._init_mixed(files, which, mode, order, device, substreams, segment_bytes, max_rounds, levels)
                return
            self.progressive = True
        parsed, self.table_host, self.header = plan(files, mode, order, substreams, segment_bytes, max_rounds, progressive, levels, pre)
        self.segment_bytes, self.max_rounds = _substream_plan(substreams, segment_bytes, max_rounds)      # (0, 0): off
        self._info_off = int(_lib.load().attwarp_jpegdec_info_offset(self.table_host.ctypes.data))
        B = len(files)
        dev = torch.device(device) if device is not None else (out.device if out is not None else _lib.default_device())
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.B, self._dev, self.mode, self.order = B, dev, mode, order
        self.parsed = parsed
        self.shapes = [(p["H"], p["W"], 1 if mode == "L" else 3 if mode == "RGB" else p["ncomp"]) for p in parsed]
        srcs = [np.frombuffer(f, dtype=np.uint8)[p["data_off"]:] for f, p in zip(files, parsed)]
        self.compressed_bytes = int(self.header.stream_bytes)
        nbytes = self.table_host.size
        with torch.cuda.device(dev):
            pad = -nbytes % 256
            total = nbytes + pad + max(self.compressed_bytes, 1)

            def fill(buf):
                buf[:nbytes] = self.table_host
                at = nbytes + pad
                for s in srcs:
                    buf[at:at + s.size] = s
                    at += s.size
            self._uploaded = torch.empty(total, device=dev, dtype=torch.uint8)
            _upload_filled(total, fill, self._uploaded)
            self.table_dev = self._uploaded[:nbytes]
            self.stream = self._uploaded[nbytes + pad:]
            self.scratch = torch.empty(int(self.header.scratch_bytes), device=dev, dtype=torch.uint8)
            if out is None:
                out = torch.empty(max(self.out_bytes, 1), device=dev, dtype=torch.uint8)
            elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != dev or out.numel() < self.out_bytes:
                raise ValueError(f"JpegFiles: out must be a dense uint8 buffer of at least {self.out_bytes} bytes on the device")
            self.buffer = out
            self.status = torch.empty(B, device=dev, dtype=torch.int32)

    def _init_mixed(self, files, which, mode, order, device, substreams, segment_bytes, max_rounds, levels):
        self.parts = []
        for kind in (False, True):
            idx = [i for i, w in enumerate(which) if w == kind]
            part = JpegFiles([files[i] for i in idx], mode, order, None, device, substreams, segment_bytes, max_rounds, kind, levels)
            self.parts.append((idx, part))
        first = self.parts[0][1]
        self.B, self._dev, self.mode, self.order = len(files), first._dev, mode, order
        self.segment_bytes, self.max_rounds = first.segment_bytes, first.max_rounds
        self.parsed, self.shapes = [None] * self.B, [None] * self.B
        for idx, part in self.parts:
            for j, i in enumerate(idx):
                self.parsed[i], self.shapes[i] = part.parsed[j], part.shapes[j]
        self.compressed_bytes = sum(part.compressed_bytes for _, part in self.parts)
        with torch.cuda.device(self._dev):
            self.status = torch.empty(self.B, device=self._dev, dtype=torch.int32)
            self._index = [torch.tensor(idx, device=self._dev, dtype=torch.int64) for idx, _ in self.parts]

    def _per_image(self, name):
        out = [None] * self.B
        for idx, part in self.parts:
            for i, v in zip(idx, getattr(part, name)()):
                out[i] = v
        return out

    @property
    def out_bytes(self) -> int:
        """Bytes of all decoded images, back to back: the capacity ``out`` needs."""
        if self.parts:
            return sum(part.out_bytes for _, part in self.parts)
        return int(self.header.out_bytes)

    def views(self) -> List[torch.Tensor]:
        """uint8 [H_i, W_i, C] views into the packed output buffer, in the convention of ``pipeline.upload_images``."""
        if self.parts:
            return self._per_image("views")
        out, off = [], 0
        for H, W, C in self.shapes:
            out.append(self.buffer[off:off + H * W * C].view(H, W, C))
            off += H * W * C
        return out

    def units(self) -> List[int]:
        """Decoding units (restart intervals) planned per image, from the headers alone: one wave each."""
        return [p["units"] for p in self.parsed]

    def levels(self) -> List[int]:
        """Dependency levels of each image's scans, from the headers alone (0 for a baseline file): the entropy launches of a
        progressive plan number the largest of them."""
        return [1 + max(p["levels"]) if p.get("progressive") else 0 for p in self.parsed]

    def coefficients(self) -> List[torch.Tensor]:
        """After a :meth:`run`: per image the int16 [blocks, 64] coefficients as they lie in scratch (views).  For tests."""
        if self.parts:
            return self._per_image("coefficients")
        ims = np.frombuffer(self.table_host, dtype=np.uint8)
        out = []
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

    def substream_info(self) -> List[tuple]:
        """After a :meth:`run` (synchronises): per image ``(segments, rounds, accepted)`` as the device left them: the
        segments planned, the rounds its workgroup ran, and 1 if the sub-streams decoded the image, 0 if the sequential
        decode did.  For measurements and tests."""
        if self.parts:
            return self._per_image("substream_info")
        raw = self.scratch[self._info_off:self._info_off + self.B * 16].cpu().numpy().view(np.uint32).reshape(self.B, 4)
        return [(int(r[0]), int(r[1]), int(r[2])) for r in raw]

    def restarts(self) -> List[int]:
        """After a :meth:`run` (synchronises): restart markers the device found in front of each image's data end; units - 1
        in a file that decodes (a progressive file: over all its scans).  For measurements and tests."""
        if self.parts:
            return self._per_image("restarts")
        st = self.scratch[:self.B * 16].cpu().numpy().view(np.uint32).reshape(self.B, 4)
        return [int(r[3]) for r in st]

    def run(self):
        """Five launches on the current stream -> ``(views, status)``: the images, and an int32 [B] device tensor (0: ok,
        else ``STATUS_NAMES[code]``; such an image's pixels are unspecified).  No host synchronisation and no host-dependent
        argument: capturable in a graph.  A progressive plan takes one clear, one restart scan, one entropy launch per
        dependency level, IDCT and colour; a mixed list runs its two plans one after the other."""
        if self.parts:
            with torch.cuda.device(self._dev):
                for (_, part), index in zip(self.parts, self._index):
                    self.status.index_copy_(0, index, part.run()[1])
            return self.views(), self.status
        with torch.cuda.device(self._dev):
            call("attwarp_jpegdec_decode_scans" if self.progressive else "attwarp_jpegdec_decode", self.table_host.ctypes.data, ptr(self.table_dev), ptr(self.stream), ptr(self.scratch),
                 ptr(self.buffer), self.buffer.numel(), ptr(self.status), stream_ptr(self._dev))
        return self.views(), self.status


def decode_jpeg(files, mode: str = "RGB", order: str = "rgb", device=None, substreams="auto", progressive: bool = False) -> List[torch.Tensor]:
    """JPEG files (bytes-like or paths) -> uint8 [H_i, W_i, C] GPU tensors, views into one packed buffer.  OSError names the
    first file the device rejects (Pillow raises OSError for such files too); ValueError for what is not decoded at all.
    ``substreams``: see :func:`plan`.  ``progressive=True`` also decodes progressive files, alone or among baseline files
    (:class:`JpegFiles`); without it such a file raises ValueError."""
    views, status = JpegFiles(files, mode, order, device=device, substreams=substreams, progressive=progressive).run()
    st = status.cpu().tolist()
    for i, s in enumerate(st):
        if s:
            name = STATUS_NAMES[s] if 0 <= s < len(STATUS_NAMES) else str(s)
            raise OSError(f"jpeg: file {i} of {len(st)} is broken: {name}")
    return views


def read_jpeg(paths, mode: str = "RGB", order: str = "rgb", device=None, substreams="auto", progressive: bool = False) -> List[torch.Tensor]:
    """:func:`decode_jpeg` of the files at ``paths``."""
    return decode_jpeg([os.fspath(p) for p in paths], mode, order, device, substreams, progressive)
