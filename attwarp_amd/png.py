"""PNG files of a whole ragged batch, encoded and decoded on the GPU.  Decoding (csrc/pngdec.hip) is the
reading half: what the reference does per file with ``Image.open(...).convert(...)`` (evaluate_accuracy.py:157-158,
MN/dataloader.py:171-382); only compressed bytes cross to the device.  8-bit grey, grey + alpha, RGB, RGBA, non-interlaced;
with ``all_formats=True`` every format of the specification: palette files, 1 / 2 / 4 / 16 bits, Adam7.

Encoding: PNG files of a whole ragged batch, encoded on the GPU (csrc/png.hip): what the reference's drivers
write per sample with ``cv2.imwrite`` (main_batched.py:243-303, new_method.py:405-506).  Only compressed bytes cross to
the host.  8-bit grey or RGB, non-interlaced; OpenCV's writer defaults (SUB filter, distance-1 matches) are the defaults
here.  The files decode to the source pixels; their bytes are this encoder's own (tests/png_ref.py restates them).
"""
from __future__ import annotations

import ctypes
import os
import struct
import zlib
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._batch import TABLE, FileBatch, ImageBatch, download, file_bytes, indexed_device, planned_table, raise_first_broken, write_files

PNG_SEG_BYTES = _lib.PNG_SEG_BYTES              # filtered bytes one workgroup encodes at most
PNG_MAX_ROW_BYTES = _lib.PNG_MAX_ROW_BYTES      # 1 + W * C at most: W <= 8191 for RGB, 24575 for grey
PNG_SEG_MAX_ROWS = _lib.PNG_SEG_MAX_ROWS
PNG_FILE_OVERHEAD = _lib.PNG_FILE_OVERHEAD
FILTERS = tuple(_lib.PNG_FILTER_IDS)
_ORDERS = {"rgb": _lib.RGB, "bgr": _lib.BGR}
_PNG_IMAGE_DTYPE = np.dtype(_lib.PngImage)


def _per_image(value, names, B: int, what: str):
    vals = [value] * B if isinstance(value, str) else list(value)
    if len(vals) != B or any(v not in names for v in vals):
        raise ValueError(f"png: {what} must be one of {sorted(names)}, or one of them per image")
    return vals


class PngBatch(ImageBatch):
    """One batch of differently sized uint8 images on the GPU, planned for ``attwarp_png_encode``: list of [H,W,C] / [H,W]
    tensors or one [B,H,W,C] tensor, C 1 or 3.  The images are referenced, not copied (any byte address, any row pitch):
    keep them alive; their CONTENT is read at every :meth:`run`, so a captured run re-encodes whatever they hold then.

    ``filter``: "none" / "sub" / "up" / "average" / "paeth" / "adaptive", ``order``: "rgb" / "bgr", ``match``: "rle" / "lz"
    -- one value or one per image.  ``out``: a uint8 device buffer of at least :attr:`bound` bytes (every segment stored).
    Limits raise ValueError before any launch.

    ``match="lz"`` (the default "rle" is OpenCV's Z_RLE) also looks for repeated content inside each segment
    and keeps, per segment, the shortest of the two token streams and the stored form: pages of text, up-sampled masks and
    panels come out much smaller, photographs the same bytes as with "rle", never longer; the encode launch takes longer.
    tests/pnglz_ref.py restates the bytes; :meth:`routes` says what each segment chose.

    :meth:`run` takes three launches (four when the batch mixes ``match="rle"`` and ``"lz"`` images: one encode launch per
    route)."""
    _who, _prefix, _dtype_error, _entry, _max_row_bytes = "PngBatch", "png", TypeError, "attwarp_png_encode", PNG_MAX_ROW_BYTES

    @staticmethod
    def _too_large(H: int, W: int, C: int) -> str:
        return f"png: a row of 1 + {W} x {C} bytes exceeds PNG_MAX_ROW_BYTES = {PNG_MAX_ROW_BYTES}"

    def __init__(self, images, filter: Union[str, Sequence[str]] = "sub", order: Union[str, Sequence[str]] = "rgb",
                 out: Optional[torch.Tensor] = None, match: Union[str, Sequence[str]] = "rle"):
        images = self._views(images, "png")
        if not images:
            raise ValueError("PngBatch: empty batch")
        B = len(images)
        filters = _per_image(filter, _lib.PNG_FILTER_IDS, B, "filter")
        orders = _per_image(order, _ORDERS, B, "order")
        matches = np.array([_lib.PNG_MATCH_IDS[m] for m in _per_image(match, _lib.PNG_MATCH_IDS, B, "match")], np.int32)
        rec = self._records(images, _PNG_IMAGE_DTYPE, [_ORDERS[o] for o in orders])
        rec["filter"] = [_lib.PNG_FILTER_IDS[f] for f in filters]
        rp = ctypes.c_void_p(rec.ctypes.data)
        mp = ctypes.c_void_p(matches.ctypes.data) if matches.any() else None      # (NULL: the plain planners' table)
        self._to_device(*planned_table(("attwarp_png_table_bytes_ex", rp, B, mp), ("attwarp_png_plan_ex", rp, B, mp, TABLE),
                                       _lib.PngHeader, ValueError, "PngBatch: "), out)

    @property
    def segments(self) -> int:
        return int(self.header.nseg)

    def routes(self) -> List[int]:
        """After a :meth:`run` (synchronises): what every segment was written as, in file order -- 0 the distance-1 block,
        1 the ``match="lz"`` block, 2 stored.  From the segment records at the head of the scratch buffer; for measurements
        and tests."""
        rec = self.scratch[:self.segments * 24].cpu().numpy().view(np.uint32).reshape(self.segments, 6)
        return [int(r) for r in rec[:, 5]]


def encode_png(images, filter="sub", order="rgb", match="rle") -> List[bytes]:
    """uint8 GPU images (list of [H,W,C] / [H,W] of any sizes, or [B,H,W,C]) -> the bytes of one PNG file each.  The outputs
    of ``warp_from_masks_ragged``, ``heatmap_overlay[_ragged]``, ``RaggedBatch.mota_of`` and ``upload_images`` are taken as
    they are.  Raw pixels never leave the device.  ``match``: :class:`PngBatch`."""
    return download(*PngBatch(images, filter, order, match=match).run())


def write_png(paths, images, filter="sub", order="rgb", match="rle") -> None:
    """:func:`encode_png`, each file written to its path."""
    paths, images = list(paths), PngBatch._views(images, "png")
    write_files("write_png", paths, len(images), lambda: encode_png(images, filter, order, match))


# ---- decoding ---------------------------------------------------------------------------------------------------------------
PNGDEC_MAX_UNITS = _lib.PNGDEC_MAX_UNITS                # decoding units (sync points) kept per image
PNGDEC_MAX_ROW_BYTES = _lib.PNGDEC_MAX_ROW_BYTES        # 1 + W * channels at most
STATUS_NAMES = _lib.PNGDEC_STATUS_NAMES
WAVE_SEGMENT_BYTES = 64                                 # inflate="wave": stream bytes per lane (DESIGN.md 3.22 has the rounds table)
WAVE_MAX_ROUNDS = 64                                    # rounds per window of 64 segments: 64 always suffice
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
_PNGDEC_IMAGE_DTYPE = np.dtype(_lib.PngDecImage)
_PNGDEC_CHUNK_DTYPE = np.dtype(_lib.PngDecChunk)
_PNGDEC_FORMAT_DTYPE = np.dtype(_lib.PngDecFormat)
_FORMAT_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}       # all_formats: the palette's index is one channel
_FORMAT_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
_ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def filtered_bytes(W: int, H: int, channels: int, depth: int, interlace: int) -> int:
    """Bytes behind inflate: rows of 1 + ceil(w * channels * depth / 8), summed over the seven Adam7 passes of an
    interlaced file (w = ceil((W - x0) / dx), h = ceil((H - y0) / dy); an empty pass has none)."""
    total = 0
    for x0, y0, dx, dy in (_ADAM7 if interlace else ((0, 0, 1, 1),)):
        w, h = max(0, -(-(W - x0) // dx)), max(0, -(-(H - y0) // dy))
        if w and h:
            total += h * (1 + (w * channels * depth + 7) // 8)
    return total


def parse_png(data, index: int = 0, all_formats: bool = False):
    """The host's whole part of decoding one file: the chunk walk.  bytes-like -> ``(W, H, colour type, [(offset, length,
    stated CRC-32) of every IDAT payload])``.  Signature, IHDR first (its CRC and IEND's are checked here: tens of bytes),
    consecutive IDATs, IEND; ancillary chunks are skipped.  No compressed byte is looked at.  ValueError names the field.

    ``all_formats=True`` accepts every depth / colour-type pair of the specification (grey 1 / 2 / 4 / 8 / 16, palette
    1 / 2 / 4 / 8, RGB, grey + alpha and RGBA 8 / 16) with interlace method 0 or 1, and returns ``(W, H, colour type, spans,
    bit depth, interlace, palette bytes)``; the palette bytes are empty unless the colour type is 3.  It refuses, by these
    words: *bit depth* (a pair outside the list), *interlace* (a method above 1), *PLTE* (a palette file without a PLTE
    before its first IDAT, with one whose length is 0, no multiple of 3 or above 768, with a second one, or with a wrong PLTE
    CRC -- Pillow is more lenient there, this walk follows the specification), *size limit* (a full-width row above
    PNGDEC_MAX_ROW_BYTES, filtered bytes over all passes or a stream of 2 GiB or more).  tRNS is skipped."""
    mv = memoryview(data).cast("B")
    n = len(mv)

    def bad(what):
        return ValueError(f"png: file {index}: {what}")

    if n < 8 or bytes(mv[:8]) != _SIGNATURE:
        raise bad("bad signature")
    pos, ihdr, spans, idat_done, iend = 8, None, [], False, False
    plte = None                                               # (all_formats, colour type 3: the PLTE payload)
    while pos < n:
        if pos + 12 > n:
            raise bad("truncated chunk")
        ln, kind = struct.unpack_from(">I4s", mv, pos)
        if pos + 12 + ln > n:
            raise bad(f"truncated {kind!r} chunk")
        crc = struct.unpack_from(">I", mv, pos + 8 + ln)[0]
        if ihdr is None and kind != b"IHDR":
            raise bad(f"IHDR is not the first chunk ({kind!r} is)")
        if kind == b"IHDR":
            if ihdr is not None or ln != 13:
                raise bad("misplaced IHDR")
            if zlib.crc32(mv[pos + 4:pos + 8 + ln]) != crc:
                raise bad("IHDR CRC")
            ihdr = struct.unpack_from(">IIBBBBB", mv, pos + 8)
        elif kind == b"IDAT":
            if idat_done:
                raise bad("IDAT chunks are not consecutive")
            spans.append((pos + 8, ln, crc))
        elif kind == b"IEND":
            if not spans:
                raise bad("IDAT missing before IEND")
            if ln != 0 or zlib.crc32(b"IEND") != crc:
                raise bad("IEND CRC")
            iend = True
            break
        else:
            idat_done = bool(spans)
            if not (kind[0] & 32) and kind != b"PLTE":        # (a suggested palette is legal in colour files)
                raise bad(f"unknown critical chunk {kind!r}")
            if all_formats and kind == b"PLTE" and ihdr[3] == 3:
                if plte is not None:
                    raise bad("a second PLTE")
                if spans:
                    raise bad("PLTE behind the first IDAT")
                if ln == 0 or ln % 3 or ln > 768:
                    raise bad(f"PLTE of {ln} bytes (3 to 768, a multiple of 3)")
                if zlib.crc32(mv[pos + 4:pos + 8 + ln]) != crc:
                    raise bad("PLTE CRC")
                plte = bytes(mv[pos + 8:pos + 8 + ln])
        pos += 12 + ln
    if ihdr is None:
        raise bad("IHDR missing")
    if not iend:
        raise bad("IEND missing")
    W, H, depth, ctype, comp, filt, lace = ihdr
    if all_formats:
        if ctype not in _FORMAT_DEPTHS:
            raise bad(f"colour type {ctype} (0, 2, 3, 4 or 6)")
        if depth not in _FORMAT_DEPTHS[ctype]:
            raise bad(f"bit depth {depth} with colour type {ctype} ({_FORMAT_DEPTHS[ctype]} only)")
        if comp != 0 or filt != 0:
            raise bad("unknown compression / filter method")
        if lace > 1:
            raise bad(f"interlace method {lace} (0 or 1)")
        if W == 0 or H == 0:
            raise bad(f"size {W} x {H}")
        if ctype == 3 and plte is None:
            raise bad("PLTE missing before the first IDAT of a palette file")
        ch = _FORMAT_CHANNELS[ctype]
        if (1 + (W * ch * depth + 7) // 8 > PNGDEC_MAX_ROW_BYTES or filtered_bytes(W, H, ch, depth, lace) >= 1 << 31
                or sum(s[1] for s in spans) >= 1 << 31):
            raise bad(f"size limit: {W} x {H} x {ch} at {depth} bits (rows of at most {PNGDEC_MAX_ROW_BYTES} bytes, images and "
                      "streams below 2 GiB)")
        return W, H, ctype, spans, depth, lace, plte or b""
    if depth != 8:
        raise bad(f"bit depth {depth} (8 only)")
    if ctype not in _CHANNELS:
        raise bad(f"colour type {ctype} (0, 2, 4 or 6; palette files are not decoded)")
    if comp != 0 or filt != 0:
        raise bad("unknown compression / filter method")
    if lace != 0:
        raise bad("interlace (non-interlaced files only)")
    if W == 0 or H == 0:
        raise bad(f"size {W} x {H}")
    rb = 1 + W * _CHANNELS[ctype]
    if rb > PNGDEC_MAX_ROW_BYTES or H * rb >= 1 << 31 or sum(s[1] for s in spans) >= 1 << 31:
        raise bad(f"size limit: {W} x {H} x {_CHANNELS[ctype]} (rows of at most {PNGDEC_MAX_ROW_BYTES} bytes, images and streams below 2 GiB)")
    return W, H, ctype, spans


class PngFiles(FileBatch):
    """One batch of PNG files planned for ``attwarp_pngdec_decode``: ``files`` is a list of bytes / bytearray / memoryview /
    paths.  The host walks the chunks (:func:`parse_png`), packs every IDAT payload of every file back to back and uploads
    them in ONE transfer; the plan depends only on what IHDR and the chunk lengths say.  ``mode``: "RGB" (what
    ``Image.open(f).convert("RGB")`` gives), "L" (``.convert("L")``) or "keep" (the file's channels without alpha);
    ``order="bgr"`` swaps a 3-channel result.  ``out``: a uint8 device buffer of at least :attr:`out_bytes` bytes.
    Unsupported files raise ValueError before any launch.  :meth:`run` is seven launches.

    ``all_formats=True`` also takes palette, 1- / 2- / 4- / 16-bit and Adam7 files (:func:`parse_png`), with Pillow's pixels:
    samples below 8 bits MSB first, grey ones scaled by 255 / 85 / 17; 16-bit grey SATURATES (``min(v, 255)``, as Pillow's
    ``I;16`` does), every other 16-bit sample gives its high byte; a palette index gives its PLTE entry ("L": the entry's
    luma), one past the entries black; tRNS and alpha are dropped.  "keep" is the file's channels without alpha at 8 bits, a
    palette file its palette's three; "bgr" swaps palette colours too.  A call whose files are all 8-bit and non-interlaced
    plans the same table and launches as without the keyword; otherwise every file of the call goes through the formats
    kernel and :meth:`run` is nine launches.

    ``inflate="wave"`` (the default is "lane") adds one launch: every image of the serial route -- no sync
    point, a dependent unit or more than 256 units, so every one-stream file of another encoder -- is inflated by one whole
    wave, 64 segments of ``segment_bytes`` (16, 32, 64, 128 or 256, default :data:`WAVE_SEGMENT_BYTES`) stream bytes at a
    time in at most ``max_rounds`` (1 .. 64, the default: no well-formed stream needs more) rounds per window.  An image that
    does not check out there is decoded by the serial route as ever, so pixels and statuses do not depend on the keyword;
    :meth:`wave_info` says what happened.  It composes with every other keyword."""
    _entry = "attwarp_pngdec_decode"

    def __init__(self, files, mode: str = "RGB", order: str = "rgb", check_crc: bool = True, out: Optional[torch.Tensor] = None,
                 device=None, all_formats: bool = False, inflate: str = "lane", segment_bytes: Optional[int] = None,
                 max_rounds: Optional[int] = None):
        files = [file_bytes(f) for f in files]
        if not files:
            raise ValueError("PngFiles: empty batch")
        if inflate not in ("lane", "wave"):
            raise ValueError(f"PngFiles: inflate={inflate!r} must be 'lane' or 'wave'")
        sb = WAVE_SEGMENT_BYTES if segment_bytes is None else int(segment_bytes)
        mr = WAVE_MAX_ROUNDS if max_rounds is None else int(max_rounds)
        if sb not in (16, 32, 64, 128, 256) or not 1 <= mr <= 64:
            raise ValueError(f"PngFiles: segment_bytes={sb} must be 16, 32, 64, 128 or 256, max_rounds={mr} in 1..64")
        self.inflate, self.segment_bytes, self.max_rounds = inflate, sb, mr
        if mode not in _lib.PNGDEC_MODE_IDS or order not in _ORDERS:
            raise ValueError(f"PngFiles: mode must be one of {sorted(_lib.PNGDEC_MODE_IDS)}, order one of {sorted(_ORDERS)}")
        parsed = [parse_png(f, i, True) if all_formats else parse_png(f, i) + (8, 0, b"") for i, f in enumerate(files)]
        B = len(files)
        nchunks = sum(len(p[3]) for p in parsed)
        rec = np.zeros(B, dtype=_PNGDEC_IMAGE_DTYPE)
        chunks = np.zeros(max(nchunks, 1), dtype=_PNGDEC_CHUNK_DTYPE)
        lens = [sum(s[1] for s in p[3]) for p in parsed]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        spans_of = []                     # per file: (source bytes, [(offset in the file, offset in the packed buffer, length)])
        c = 0
        for b, (f, (W, H, ctype, spans, *_)) in enumerate(zip(files, parsed)):
            at = int(offs[b])
            moves = []
            for off, ln, crc in spans:
                moves.append((off, at, ln))
                chunks[c] = (at, ln, crc, b, 0)
                at += ln
                c += 1
            spans_of.append((np.frombuffer(f, dtype=np.uint8), moves))
        rec["stream_off"] = offs[:-1]; rec["stream_len"] = lens
        rec["W"] = [p[0] for p in parsed]; rec["H"] = [p[1] for p in parsed]; rec["color_type"] = [p[2] for p in parsed]
        rec["mode"] = _lib.PNGDEC_MODE_IDS[mode]; rec["order"] = _ORDERS[order]
        dev = indexed_device(device, out)
        rp, cp = ctypes.c_void_p(rec.ctypes.data), ctypes.c_void_p(chunks.ctypes.data)
        fp = None
        if all_formats:
            fmt = np.zeros(B, dtype=_PNGDEC_FORMAT_DTYPE)
            fmt["depth"] = [p[4] for p in parsed]; fmt["interlace"] = [p[5] for p in parsed]
            fmt["palette_entries"] = [len(p[6]) // 3 for p in parsed]
            for b, p in enumerate(parsed):
                fmt["palette"][b, :len(p[6])] = np.frombuffer(p[6], np.uint8)
            fp = ctypes.c_void_p(fmt.ctypes.data)
            size = ("attwarp_pngdec_table_bytes_formats", rp, fp, B, cp, nchunks)
            plan = ("attwarp_pngdec_plan_formats", rp, fp, B, cp, nchunks, int(bool(check_crc)), TABLE)
        else:
            size = ("attwarp_pngdec_table_bytes", rp, B, nchunks)
            plan = ("attwarp_pngdec_plan", rp, B, cp, nchunks, int(bool(check_crc)), TABLE)
        if inflate == "wave":             # (formats: the array or NULL; the table is the other planners' plus the mark)
            size = ("attwarp_pngdec_table_bytes_wave", rp, fp, B, cp, nchunks)
            plan = ("attwarp_pngdec_plan_wave", rp, fp, B, cp, nchunks, int(bool(check_crc)), sb, mr, TABLE)
        self.table_host, self.header = planned_table(size, plan, _lib.PngDecHeader, ValueError, "PngFiles: ", wrap_plan=True)
        self.B, self._dev, self.mode, self.order = B, dev, mode, order
        self.shapes = [(p[1], p[0], 1 if mode == "L" else 3 if mode == "RGB" else (1 if p[2] in (0, 4) else 3)) for p in parsed]
        self.compressed_bytes = int(offs[-1])

        def fill(body):                   # every IDAT payload, gathered straight into the pinned slot
            for src, moves in spans_of:
                for off, at, ln in moves:
                    body[at:at + ln] = src[off:off + ln]
        self._to_device(fill, out)

    def routes(self):
        """After a :meth:`run` (synchronises): per image ``(route, units on the chain, sync points kept)``; route 0 is the
        unit route, 1 the serial one, 2 none (the zlib header failed).  For measurements and tests."""
        st = self.scratch[:self.B * 32].cpu().numpy().view(np.uint32).reshape(self.B, 8)
        return [(int(r[1]), int(r[7]), int(r[0])) for r in st]

    def kept(self):
        """After a :meth:`run` (synchronises): per image the byte positions the marker scan kept, the stream's start first
        (empty when the zlib header failed).  For measurements and tests."""
        B, U = self.B, PNGDEC_MAX_UNITS
        nunits = self.scratch[:B * 32].cpu().numpy().view(np.uint32).reshape(B, 8)[:, 0]
        off = -(-B * 32 // 16) * 16 + B * U * 32                 # behind the states and the unit records (pd_kept_off)
        pos = self.scratch[off:off + B * U * 4].cpu().numpy().view(np.uint32).reshape(B, U)
        return [pos[b, :int(nunits[b])].tolist() for b in range(B)]

    def wave_info(self, resolution: bool = False):
        """After a :meth:`run` with ``inflate="wave"`` (synchronises): per image ``(windows, rounds, accepted)`` as the
        device left them -- windows of 64 segments decoded, rounds over all of them, 1 if the wave route's bytes stand (0: the
        image took another route, or fell back to the serial one).  ``resolution=True`` adds the match-resolution rounds as
        a fourth number.  For measurements and tests."""
        if self.inflate != "wave":
            raise ValueError("PngFiles.wave_info: planned with inflate='lane'")
        n = int(self.header.scratch_bytes)
        rec = self.scratch[n - self.B * 16:n].cpu().numpy().view(np.uint32).reshape(self.B, 4)
        return [tuple(int(x) for x in (r if resolution else r[:3])) for r in rec]


def decode_png(files, mode: str = "RGB", order: str = "rgb", device=None, all_formats: bool = False,
               inflate: str = "lane") -> List[torch.Tensor]:
    """PNG files (bytes-like or paths) -> uint8 [H_i, W_i, C] GPU tensors, views into one packed buffer.  OSError names the
    first file the device rejects (Pillow raises OSError for such files too); ValueError for what is not decoded at all.
    ``all_formats=True`` also takes palette, 1- / 2- / 4- / 16-bit and interlaced files (:class:`PngFiles`); without it they
    raise ValueError.  ``inflate="wave"`` inflates every one-stream file with a whole wave (:class:`PngFiles`); the result does
    not depend on it."""
    views, status = PngFiles(files, mode, order, device=device, all_formats=all_formats, inflate=inflate).run()
    raise_first_broken(status, STATUS_NAMES, "png")
    return views


def read_png(paths, mode: str = "RGB", order: str = "rgb", device=None, all_formats: bool = False,
             inflate: str = "lane") -> List[torch.Tensor]:
    """:func:`decode_png` of the files at ``paths`` (``inflate``: see there)."""
    return decode_png([os.fspath(p) for p in paths], mode, order, device, all_formats, inflate)
