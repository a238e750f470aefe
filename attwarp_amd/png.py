"""PNG files of a whole ragged batch, encoded on the GPU (csrc/png.hip): what the reference's drivers
write per sample with ``cv2.imwrite`` (main_batched.py:243-303, new_method.py:405-506).  Only compressed bytes cross to
the host.  8-bit grey or RGB, non-interlaced; OpenCV's writer defaults (SUB filter, distance-1 matches) are the defaults
here.  The files decode to the source pixels; their bytes are this encoder's own (tests/png_ref.py restates them).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

PNG_SEG_BYTES = _lib.PNG_SEG_BYTES              # filtered bytes one workgroup encodes at most
PNG_MAX_ROW_BYTES = _lib.PNG_MAX_ROW_BYTES      # 1 + W * C at most: W <= 8191 for RGB, 24575 for grey
PNG_SEG_MAX_ROWS = _lib.PNG_SEG_MAX_ROWS
PNG_FILE_OVERHEAD = _lib.PNG_FILE_OVERHEAD
FILTERS = tuple(_lib.PNG_FILTER_IDS)
_ORDERS = {"rgb": _lib.RGB, "bgr": _lib.BGR}
_PNG_IMAGE_DTYPE = np.dtype(_lib.PngImage)


def _views(images) -> List[torch.Tensor]:
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise ValueError("png: a tensor batch is [B,H,W,C]; pass differently sized images as a list")
        return [images[b] for b in range(images.shape[0])]
    return list(images)


def _per_image(value, names, B: int, what: str):
    vals = [value] * B if isinstance(value, str) else list(value)
    if len(vals) != B or any(v not in names for v in vals):
        raise ValueError(f"png: {what} must be one of {sorted(names)}, or one of them per image")
    return vals


def _geometry(t: torch.Tensor):
    """(H, W, C, pitch) of a uint8 [H,W,C] / [H,W] view whose pixels are dense along a row."""
    if t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise TypeError(f"png: uint8 [H,W,C] / [H,W] tensors expected, got {t.dtype} {tuple(t.shape)}")
    H, W = int(t.shape[0]), int(t.shape[1])
    C = int(t.shape[2]) if t.dim() == 3 else 1
    if H < 1 or W < 1:
        raise ValueError(f"png: empty image {tuple(t.shape)}")
    if C not in (1, 3):
        raise ValueError(f"png: {C} channels (grey [H,W] / [H,W,1] or RGB [H,W,3] only)")
    if 1 + W * C > PNG_MAX_ROW_BYTES:
        raise ValueError(f"png: a row of 1 + {W} x {C} bytes exceeds PNG_MAX_ROW_BYTES = {PNG_MAX_ROW_BYTES}")
    st = t.stride()
    if (t.dim() == 3 and C > 1 and st[2] != 1) or (W > 1 and st[1] != C):
        raise ValueError(f"png: unsupported strides {st} for shape {tuple(t.shape)}: the pixels of a row must be dense")
    pitch = int(st[0]) if H > 1 else W * C
    if pitch < W * C or pitch >= 1 << 31:
        raise ValueError(f"png: unsupported row stride {st[0]} for rows of {W * C} bytes")
    return H, W, C, pitch


class PngBatch:
    """One batch of differently sized uint8 images on the GPU, planned for ``attwarp_png_encode``: list of [H,W,C] / [H,W]
    tensors or one [B,H,W,C] tensor, C 1 or 3.  The images are referenced, not copied (any byte address, any row pitch):
    keep them alive; their CONTENT is read at every :meth:`run`, so a captured run re-encodes whatever they hold then.

    ``filter``: "none" / "sub" / "up" / "average" / "paeth" / "adaptive", ``order``: "rgb" / "bgr" -- one value or one per
    image.  ``out``: a uint8 device buffer of at least :attr:`bound` bytes.  Limits raise ValueError before any launch."""

    def __init__(self, images, filter: Union[str, Sequence[str]] = "sub", order: Union[str, Sequence[str]] = "rgb",
                 out: Optional[torch.Tensor] = None):
        from .pipeline import _upload
        images = _views(images)
        if not images:
            raise ValueError("PngBatch: empty batch")
        B = len(images)
        filters = _per_image(filter, _lib.PNG_FILTER_IDS, B, "filter")
        orders = _per_image(order, _ORDERS, B, "order")
        geo = [_geometry(t) for t in images]
        dev = _lib.require_gpu(*images)
        self.images, self.B, self._dev = images, B, dev
        rec = np.zeros(B, dtype=_PNG_IMAGE_DTYPE)
        rec["src"] = [t.data_ptr() for t in images]
        rec["H"] = [g[0] for g in geo]; rec["W"] = [g[1] for g in geo]; rec["C"] = [g[2] for g in geo]
        rec["pitch"] = [g[3] for g in geo]
        rec["order"] = [_ORDERS[o] for o in orders]
        rec["filter"] = [_lib.PNG_FILTER_IDS[f] for f in filters]
        lib = _lib.load()
        rp = ctypes.c_void_p(rec.ctypes.data)
        nbytes = lib.attwarp_png_table_bytes(rp, B)
        if nbytes == 0:
            raise ValueError("PngBatch: " + lib.attwarp_last_error().decode("utf-8", "replace"))
        self.table_host = np.empty(nbytes, dtype=np.uint8)
        call("attwarp_png_plan", rp, B, self.table_host.ctypes.data, nbytes)
        self.header = _lib.PngHeader.from_address(self.table_host.ctypes.data)
        self._pixels = sum(g[0] * g[1] * g[2] for g in geo)
        with torch.cuda.device(dev):
            self.table_dev = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            _upload(self.table_host, self.table_dev)
            self.scratch = torch.empty(int(self.header.scratch_bytes), device=dev, dtype=torch.uint8)
            if out is None:
                out = torch.empty(self.bound, device=dev, dtype=torch.uint8)
            elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != dev or out.numel() < self.bound:
                raise ValueError(f"PngBatch: out must be a dense uint8 buffer of at least {self.bound} bytes on the images' device")
            self.buffer = out
            self.offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)

    @property
    def bound(self) -> int:
        """Bytes the files of this batch take at most (every segment stored): the capacity ``out`` needs."""
        return int(self.header.out_bytes)

    @property
    def segments(self) -> int:
        return int(self.header.nseg)

    def algorithmic_bytes(self) -> int:
        """Pixel bytes the encoder has to read (the compressed bytes written depend on the content)."""
        return self._pixels

    def run(self):
        """Three launches on the current stream -> ``(buffer, offsets)``: file b is ``buffer[offsets[b]:offsets[b+1]]``
        (uint8 and int64 [B+1], both on the device).  No host-dependent argument: capturable in a graph."""
        with torch.cuda.device(self._dev):
            call("attwarp_png_encode", self.table_host.ctypes.data, ptr(self.table_dev), ptr(self.scratch), ptr(self.buffer),
                 self.buffer.numel(), ptr(self.offsets), stream_ptr(self._dev))
        return self.buffer, self.offsets


def download(buffer: torch.Tensor, offsets: torch.Tensor) -> List[bytes]:
    """The files of a :meth:`PngBatch.run`: one device-to-host copy of the offsets, one of the used bytes."""
    offs = offsets.cpu().tolist()
    data = buffer[:offs[-1]].cpu().numpy().tobytes()
    return [data[a:b] for a, b in zip(offs[:-1], offs[1:])]


def encode_png(images, filter="sub", order="rgb") -> List[bytes]:
    """uint8 GPU images (list of [H,W,C] / [H,W] of any sizes, or [B,H,W,C]) -> the bytes of one PNG file each.  The outputs
    of ``warp_from_masks_ragged``, ``heatmap_overlay[_ragged]``, ``RaggedBatch.mota_of`` and ``upload_images`` are taken as
    they are.  Raw pixels never leave the device."""
    return download(*PngBatch(images, filter, order).run())


def write_png(paths, images, filter="sub", order="rgb") -> None:
    """:func:`encode_png`, each file written to its path."""
    paths, images = list(paths), _views(images)
    if len(paths) != len(images):
        raise ValueError(f"write_png: {len(paths)} paths for {len(images)} images")
    files = encode_png(images, filter, order)
    for p, f in zip(paths, files):
        with open(p, "wb") as fh:
            fh.write(f)
