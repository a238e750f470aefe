"""What the planned batch classes share (pipeline.RaggedBatch / ClipBatch, dataloader.PreparedImages, png.PngBatch /
PngFiles, jpeg.JpegBatch / JpegFiles): the pinned staging pool every host-to-device table goes through, the planned-table
idiom of the library's ``*_table_bytes`` / ``*_plan`` pairs, the base classes of a planned batch of FILES to decode and of
IMAGES to encode, and the helper that decodes a list of several kinds group by group.  Internal: nothing here is part of
the package's interface.
"""
from __future__ import annotations

import os
import threading
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

_STAGING: dict = {}                   # device index -> pinned staging buffers: [tensor, event of the last copy out of it, free]
_STAGING_LOCK = threading.Lock()     # (host threads on their own streams share the pool)


def _upload(host: "np.ndarray", dst: torch.Tensor):
    """host bytes -> dst (device uint8), asynchronously on the current stream of dst's device through a pooled pinned buffer
    (one pool per device: a slot's event is recorded on, and queried against, the stream that carries its copy).
    Refuses to run inside a stream capture: the copy would become a graph node and be re-executed on every replay from a
    staging buffer that has long been reused."""
    def fill(buf):
        buf[:] = host
    _upload_filled(host.size, fill, dst)


def _upload_filled(n: int, fill, dst: torch.Tensor):
    """:func:`_upload` for bytes that are assembled in place: ``fill(buf)`` writes the n bytes straight into the pinned
    staging slot (a uint8 numpy view), so data gathered from many sources crosses host memory once."""
    dev = dst.device
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("attwarp_amd: a host-to-device table upload inside a stream capture (build the batch objects / call "
                           "upload_images before capturing; a captured copy would replay from a reused staging buffer)")
    with torch.cuda.device(dev):
        with _STAGING_LOCK:
            pool = _STAGING.setdefault(dev.index, [])
            slot = None
            for s in pool:
                if s[0].numel() >= n and s[2] and s[1].query():
                    slot = s
                    break
            if slot is None:
                if len(pool) >= 64:               # (only if nothing ever completes: keep the pool bounded)
                    torch.cuda.synchronize(dev)
                    del pool[1:]
                slot = [torch.empty(max(n, 1 << 16), dtype=torch.uint8).pin_memory(), torch.cuda.Event(), True]
                pool.append(slot)
            slot[2] = False                       # taken: nobody else may pick it until its copy has been enqueued and recorded
        try:
            fill(slot[0][:n].numpy())
            dst.copy_(slot[0][:n], non_blocking=True)
            slot[1].record(torch.cuda.current_stream(dev))
        finally:
            slot[2] = True


def uploaded(host: "np.ndarray", dev: torch.device) -> torch.Tensor:
    """A new uint8 tensor on ``dev`` that holds the bytes of ``host`` (records, a table): :func:`_upload` into it."""
    dst = torch.empty(host.nbytes, device=dev, dtype=torch.uint8)
    _upload(host.view(np.uint8).reshape(-1), dst)
    return dst


def packed_views(flat: torch.Tensor, shapes) -> List[torch.Tensor]:
    """Views of the given shapes into a flat buffer that holds them back to back."""
    out, off = [], 0
    for shape in shapes:
        n = int(np.prod(shape))
        out.append(flat[off:off + n].view(*shape))
        off += n
    return out


TABLE = object()                      # in the planner's arguments of planned_table: where (table address, table bytes) go


def planned_table(size, plan, header, exc, prefix: str, wrap_plan: bool = False):
    """The planned-table idiom: ``size = (name of the *_table_bytes entry point, its arguments...)`` gives the bytes (0: ``exc``
    with ``prefix`` and the library's last error), ``plan = (name of the planner, its arguments...)`` fills a host buffer of
    that size, :data:`TABLE` standing where the planner takes the buffer and its size -> ``(table, header)``, the header a
    ``header`` structure over the buffer's first bytes.  ``wrap_plan``: the planner's AttWarpError becomes ``exc`` too."""
    lib = _lib.load()
    nbytes = getattr(lib, size[0])(*size[1:])
    if nbytes == 0:
        raise exc(prefix + lib.attwarp_last_error().decode("utf-8", "replace"))
    table = np.empty(nbytes, dtype=np.uint8)
    args = []
    for a in plan[1:]:
        args += [table.ctypes.data, nbytes] if a is TABLE else [a]
    try:
        call(plan[0], *args)
    except _lib.AttWarpError as e:
        if not wrap_plan:
            raise
        raise exc(f"{prefix}{e}") from None
    return table, header.from_address(table.ctypes.data)


def file_bytes(f):
    """A file given as a path -> its bytes; bytes-like objects are taken as they are."""
    if isinstance(f, (str, os.PathLike)):
        with open(f, "rb") as fh:
            return fh.read()
    return f


def indexed_device(device=None, out=None) -> torch.device:
    """``device``, else the device of ``out``, else the default one, with its index filled in."""
    dev = torch.device(device) if device is not None else (out.device if out is not None else _lib.default_device())
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def raise_first_broken(status: torch.Tensor, names, what: str):
    """OSError for the first file whose status is not 0 (synchronises): ``what`` is "png" / "jpeg"."""
    st = status.cpu().tolist()
    for i, s in enumerate(st):
        if s:
            name = names[s] if 0 <= s < len(names) else str(s)
            raise OSError(f"{what}: file {i} of {len(st)} is broken: {name}")


def split_indices(keys, order) -> list:
    """``[(key, indices of the items with that key)]`` for every key of ``order`` that occurs, in that order."""
    return [(k, idx) for k in order for idx in [[i for i, x in enumerate(keys) if x == k]] if idx]


def scattered(n: int, groups) -> list:
    """``groups``: (indices, one value per index) -> the n values in input order."""
    out = [None] * n
    for idx, values in groups:
        for i, v in zip(idx, values):
            out[i] = v
    return out


def per_kind(items, keys, order, run) -> list:
    """Split ``items`` by their ``keys``, call ``run(key, items of that key)`` once per kind that occurs (in ``order``), each
    giving one result per item, and put the results back in input order."""
    return scattered(len(items), ((idx, run(k, [items[i] for i in idx])) for k, idx in split_indices(keys, order)))


class FileBatch:
    """A planned batch of image files (png.PngFiles, jpeg.JpegFiles).  The subclass parses and plans -- it sets ``B``,
    ``shapes`` ([(H, W, C)]), ``table_host``, ``header`` (with out_bytes and scratch_bytes), ``compressed_bytes``, ``_dev``
    and ``_entry`` (the decode entry point) -- and calls :meth:`_to_device`, which makes the ONE transfer of the table and,
    256-byte aligned behind it, the compressed bytes, and allocates what a run writes."""

    def _to_device(self, fill_stream, out):
        """``fill_stream(body)`` gathers the compressed bytes straight into the pinned slot (a uint8 view that starts at the
        stream's first byte); ``out``: the caller's buffer or None."""
        who, dev, nbytes = type(self).__name__, self._dev, self.table_host.size
        with torch.cuda.device(dev):
            pad = -nbytes % 256
            total = nbytes + pad + max(self.compressed_bytes, 1)

            def fill(buf):
                buf[:nbytes] = self.table_host
                fill_stream(buf[nbytes + pad:])
            self._uploaded = torch.empty(total, device=dev, dtype=torch.uint8)
            _upload_filled(total, fill, self._uploaded)
            self.table_dev = self._uploaded[:nbytes]
            self.stream = self._uploaded[nbytes + pad:]
            self.scratch = torch.empty(int(self.header.scratch_bytes), device=dev, dtype=torch.uint8)
            if out is None:
                out = torch.empty(max(self.out_bytes, 1), device=dev, dtype=torch.uint8)
            elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != dev or out.numel() < self.out_bytes:
                raise ValueError(f"{who}: out must be a dense uint8 buffer of at least {self.out_bytes} bytes on the device")
            self.buffer = out
            self.status = torch.empty(self.B, device=dev, dtype=torch.int32)

    @property
    def out_bytes(self) -> int:
        """Bytes of all decoded images, back to back: the capacity ``out`` needs."""
        return int(self.header.out_bytes)

    def views(self) -> List[torch.Tensor]:
        """uint8 [H_i, W_i, C] views into the packed output buffer, in the convention of ``pipeline.upload_images``."""
        return packed_views(self.buffer, self.shapes)

    def run(self):
        """The launches of the subclass's entry point on the current stream -> ``(views, status)``: the images, and an int32
        [B] device tensor (0: ok, else the module's ``STATUS_NAMES[code]``; such an image's pixels are unspecified).  No host
        synchronisation and no host-dependent argument: capturable in a graph."""
        with torch.cuda.device(self._dev):
            call(self._entry, self.table_host.ctypes.data, ptr(self.table_dev), ptr(self.stream), ptr(self.scratch),
                 ptr(self.buffer), self.buffer.numel(), ptr(self.status), stream_ptr(self._dev))
        return self.views(), self.status


class ImageBatch:
    """A planned batch of uint8 images to be encoded into files (png.PngBatch, jpeg.JpegBatch), the counterpart of
    :class:`FileBatch`.  The subclass names itself in its messages -- ``_who`` (the class), ``_prefix`` (the module),
    ``_dtype_error`` (what a wrong dtype raises) --, its encode entry point ``_entry`` and its size limit (``_max_side``: H and
    W at most, ``_max_row_bytes``: 1 + W * C at most, ``_too_large``: the message), parses its keywords, and calls
    :meth:`_views`, :meth:`_records` and, with its planned table, :meth:`_to_device`."""
    _max_side = _max_row_bytes = 1 << 62

    @classmethod
    def _views(cls, images, who: Optional[str] = None) -> List[torch.Tensor]:
        """A [B,H,W,C] tensor -> its B images; anything else: the list it is."""
        if isinstance(images, torch.Tensor):
            if images.dim() != 4:
                raise ValueError(f"{who or cls._who}: a tensor batch is [B,H,W,C]; pass differently sized images as a list")
            return [images[b] for b in range(images.shape[0])]
        return list(images)

    @classmethod
    def _geometry(cls, images) -> list:
        """[(H, W, C, pitch)] of uint8 [H,W,C] / [H,W] views whose pixels are dense along a row."""
        pre, max_side, max_row = cls._prefix, cls._max_side, cls._max_row_bytes
        out = []
        for t in images:
            if t.dtype != torch.uint8 or t.dim() not in (2, 3):
                raise cls._dtype_error(f"{pre}: uint8 [H,W,C] / [H,W] tensors expected, got {t.dtype} {tuple(t.shape)}")
            H, W = int(t.shape[0]), int(t.shape[1])
            C = int(t.shape[2]) if t.dim() == 3 else 1
            if H < 1 or W < 1:
                raise ValueError(f"{pre}: empty image {tuple(t.shape)}")
            if C not in (1, 3):
                raise ValueError(f"{pre}: {C} channels (grey [H,W] / [H,W,1] or RGB [H,W,3] only)")
            if H > max_side or W > max_side or 1 + W * C > max_row:
                raise ValueError(cls._too_large(H, W, C))
            st = t.stride()
            if (t.dim() == 3 and C > 1 and st[2] != 1) or (W > 1 and st[1] != C):
                raise ValueError(f"{pre}: unsupported strides {st} for shape {tuple(t.shape)}: the pixels of a row must be dense")
            pitch = int(st[0]) if H > 1 else W * C
            if pitch < W * C or pitch >= 1 << 31:
                raise ValueError(f"{pre}: unsupported row stride {st[0]} for rows of {W * C} bytes")
            out.append((H, W, C, pitch))
        return out

    def _records(self, images, dtype, orders) -> "np.ndarray":
        """Checks every image and fills what the two record types share: src, H, W, C, pitch, order (ids).  Sets ``images``,
        ``B`` and the device; the images must live on one GPU."""
        geo = self._geometry(images)
        self.images, self.B, self._dev = images, len(images), _lib.require_gpu(*images)
        self._pixels = sum(g[0] * g[1] * g[2] for g in geo)
        rec = np.zeros(self.B, dtype=dtype)
        rec["src"] = [t.data_ptr() for t in images]
        rec["H"] = [g[0] for g in geo]; rec["W"] = [g[1] for g in geo]; rec["C"] = [g[2] for g in geo]
        rec["pitch"] = [g[3] for g in geo]
        rec["order"] = orders
        return rec

    def _to_device(self, table_host, header, out):
        """The upload of the table the subclass planned (:func:`planned_table`), and what a run writes (``out``: the caller's
        buffer or None)."""
        who, dev = self._who, self._dev
        self.table_host, self.header = table_host, header
        with torch.cuda.device(dev):
            self.table_dev = uploaded(self.table_host, dev)
            self.scratch = torch.empty(int(self.header.scratch_bytes), device=dev, dtype=torch.uint8)
            if out is None:
                out = torch.empty(self.bound, device=dev, dtype=torch.uint8)
            elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != dev or out.numel() < self.bound:
                raise ValueError(f"{who}: out must be a dense uint8 buffer of at least {self.bound} bytes on the images' device")
            self.buffer = out
            self.offsets = torch.empty(self.B + 1, device=dev, dtype=torch.int64)

    @property
    def bound(self) -> int:
        """Bytes the files of this batch take at most (the planner's sum over the images): the capacity ``out`` needs."""
        return int(self.header.out_bytes)

    def algorithmic_bytes(self) -> int:
        """Pixel bytes the encoder has to read (the compressed bytes written depend on the content)."""
        return self._pixels

    def run(self):
        """The launches of the subclass's entry point on the current stream -> ``(buffer, offsets)``: file b is
        ``buffer[offsets[b]:offsets[b+1]]`` (uint8 and int64 [B+1], both on the device).  No host-dependent argument:
        capturable in a graph."""
        with torch.cuda.device(self._dev):
            call(self._entry, self.table_host.ctypes.data, ptr(self.table_dev), ptr(self.scratch), ptr(self.buffer),
                 self.buffer.numel(), ptr(self.offsets), stream_ptr(self._dev))
        return self.buffer, self.offsets


def download(buffer: torch.Tensor, offsets: torch.Tensor) -> List[bytes]:
    """The files of an :meth:`ImageBatch.run`: one device-to-host copy of the offsets, one of the used bytes."""
    offs = offsets.cpu().tolist()
    data = buffer[:offs[-1]].cpu().numpy().tobytes()
    return [data[a:b] for a, b in zip(offs[:-1], offs[1:])]


def write_files(who: str, paths, n: int, encode) -> None:
    """``encode()``'s n files, each written to its path; ``who``: the caller's name in the error."""
    paths = list(paths)
    if len(paths) != n:
        raise ValueError(f"{who}: {len(paths)} paths for {n} images")
    for p, f in zip(paths, encode()):
        with open(p, "wb") as fh:
            fh.write(f)
