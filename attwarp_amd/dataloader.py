"""The MarginalNet trainer's batches, prepared on the GPU from decoded samples of different sizes.

The reference prepares every sample on the CPU (MN/dataloader.py: ``FullDataset.__getitem__`` :204-273,
``_load_attention_map_from_artifact`` :160-189, the transforms :123-137 and :325-332) and stacks them (MN/data.py
``collate_str``): a PIL image goes through ``T.Resize((S, S))`` + ``T.ToTensor()``, a float attention array is normalised,
quantised to 8 bits, NEAREST-resized to S x S and passed through ``ToTensor``.  Here the decoded samples go to the GPU as
they are (one transfer per batch) and two entry points of the HIP library produce ``batch["image"]`` (B,3,S,S) and
``batch["attention_map"]`` (B,1,S,S), bit for bit what Pillow + ToTensor compute.  File I/O, decoding, the
dataset classes and ``image_size=None`` batches (samples of different sizes cannot be stacked) stay with the caller.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, _tables, pipeline
from ._batch import TABLE, packed_views, planned_table, uploaded
from ._lib import call, ptr, require_gpu, stream_ptr

_PREP_IMAGE_DTYPE = np.dtype([("image", "<u8"), ("bounds_x", "<u8"), ("kk_x", "<u8"), ("bounds_y", "<u8"), ("kk_y", "<u8"),
                              ("H", "<i4"), ("W", "<i4"), ("ksize_x", "<i4"), ("ksize_y", "<i4"),
                              ("vertical_first", "<i4"), ("reserved", "<i4")])          # attwarp_prep_image
# the per-image record inside a planned table (dataprep.hip: PrepImageDev): the caller's record + the launcher's choices
_PREP_RECORD_DTYPE = np.dtype(_PREP_IMAGE_DTYPE.descr + [("tmp_off", "<i8"), ("fused", "<i4"), ("ny", "<i4"), ("rb", "<i4"),
                                                         ("nr_cap", "<i4")])
_PREP_ATTENTION_DTYPE = np.dtype([("map", "<u8"), ("idx_x", "<u8"), ("idx_y", "<u8"),
                                  ("h", "<i4"), ("w", "<i4"), ("normalize", "<i4"), ("reserved", "<i4")])   # attwarp_prep_attention


def _size(image_size):
    if image_size is None:
        raise ValueError("attwarp_amd.dataloader: image_size=None keeps every sample at its native size; such samples cannot "
                         "be stacked into a batch")
    sh, sw = (int(image_size), int(image_size)) if isinstance(image_size, int) else (int(image_size[0]), int(image_size[1]))
    if sh < 1 or sw < 1:
        raise ValueError(f"attwarp_amd.dataloader: image_size must be positive (got {image_size})")
    return sh, sw


def _bilinear_tables(n_in: int, n_out: int, device: torch.device):
    """Pillow's 8-bit BILINEAR tables n_in -> n_out on the device, at their own tap count (the kernels here take any):
    (bounds int32 [n_out,2], kk int32 [n_out,ksize], ksize)."""
    key = ("prep_bilinear", n_in, n_out, str(device))
    t = _tables._DEV_CACHE.get(key)
    if t is None:
        bounds, kk, ksize = _tables._lanczos_tables_host(n_in, n_out, "bilinear")
        kk = np.ascontiguousarray(kk[:, :ksize])
        t = _tables._cache_put(key, (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize))
    return t


def _nearest_table(n_in: int, n_out: int, device: torch.device) -> torch.Tensor:
    """Pillow's NEAREST source indices n_in -> n_out (attwarp_pil_nearest_index) on the device: int32 [n_out]."""
    key = ("prep_nearest", n_in, n_out, str(device))
    t = _tables._DEV_CACHE.get(key)
    if t is None:
        idx = np.empty(n_out, dtype=np.int32)
        call("attwarp_pil_nearest_index", int(n_in), int(n_out), idx.ctypes.data)
        t = _tables._cache_put(key, torch.from_numpy(idx).to(device))
    return t


def _uploads_done(device: torch.device) -> torch.cuda.Event:
    """An event behind every upload enqueued so far on the constructing stream (tables, records)."""
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    return ev


def _wait_uploads(ev: torch.cuda.Event, device: torch.device):
    """run() may be called on another stream than the one the batch was planned on: order it behind the uploads.  Inside a
    stream capture no outside event can be waited for; the capture has to start after the planning stream's work, as
    ``pipeline.capture_step`` arranges with its ``wait_stream``."""
    if not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream(device).wait_event(ev)


class PreparedImages:
    """One batch of uint8 [H_i,W_i,C] GPU images planned for ``attwarp_prep_images_u8``: the coefficient tables, the
    record table (host and device copy), the uint8 intermediate of the images that take the two-launch route and the
    output (B,C,S_h,S_w).  ``run()`` enqueues the launch(es) on the current stream -- any stream: it first waits for the
    event recorded behind the table uploads of the constructor -- and may be captured in a graph; a capture cannot wait for
    that event, so it must begin after the constructing stream's work (``pipeline.capture_step`` does that).  The images are
    referenced, not copied: keep them alive and unchanged until the launch has run, and let the stream that wrote them be
    ordered before the one ``run()`` is called on."""

    def __init__(self, images: Sequence[torch.Tensor], image_size=512, out: Optional[torch.Tensor] = None):
        sh, sw = _size(image_size)
        images = list(images)
        if not images:
            raise ValueError("prepare_images: empty batch")
        for im in images:
            if not isinstance(im, torch.Tensor):
                raise TypeError("PreparedImages: uint8 [H,W,C] GPU tensors expected (prepare_images uploads host images)")
        dev = require_gpu(*images)
        for im in images:
            if im.dtype != torch.uint8:
                raise TypeError(f"prepare_images: images must be uint8 (got {im.dtype})")
            if im.dim() != 3:
                raise ValueError(f"prepare_images: images must be [H,W,C] (got {tuple(im.shape)})")
        C = int(images[0].shape[2])
        if C not in (1, 3) or any(int(im.shape[2]) != C for im in images):
            raise ValueError("prepare_images: every image must have the same channel count, 1 or 3")
        if any(im.numel() == 0 for im in images):
            raise ValueError("prepare_images: empty image")
        self.images = [im if im.is_contiguous() else im.contiguous() for im in images]
        self.B, self.C, self.S_h, self.S_w, self._dev = len(images), C, sh, sw, dev
        rec = np.zeros(self.B, dtype=_PREP_IMAGE_DTYPE)
        hs = [int(im.shape[0]) for im in self.images]
        ws = [int(im.shape[1]) for im in self.images]
        tx = [_bilinear_tables(w, sw, dev) for w in ws]
        ty = [_bilinear_tables(h, sh, dev) for h in hs]
        rec["image"] = [im.data_ptr() for im in self.images]
        rec["H"], rec["W"] = hs, ws
        rec["bounds_x"] = [t[0].data_ptr() for t in tx]; rec["kk_x"] = [t[1].data_ptr() for t in tx]
        rec["bounds_y"] = [t[0].data_ptr() for t in ty]; rec["kk_y"] = [t[1].data_ptr() for t in ty]
        rec["ksize_x"] = [t[2] for t in tx]; rec["ksize_y"] = [t[2] for t in ty]
        # PIL.Image.resize runs the vertical pass first on a source more than 100 times as high as wide that it shrinks
        # vertically (two calls of the resampler); the intermediate is uint8 either way, so the order shows in the bytes
        rec["vertical_first"] = [int(h > 100 * w and sh < h) for h, w in zip(hs, ws)]
        self._keep = tx + ty
        rp = ctypes.c_void_p(rec.ctypes.data)
        self.table_host, self.header = planned_table(
            ("attwarp_prep_images_table_bytes", rp, self.B, C, sh, sw), ("attwarp_prep_images_plan", rp, self.B, C, sh, sw, TABLE),
            _lib.PrepHeader, _lib.AttWarpError, "attwarp_prep_images_table_bytes: ")
        self.table_dev = uploaded(self.table_host, dev)
        self.tmp = torch.empty(int(self.header.tmp_bytes), device=dev, dtype=torch.uint8) if self.header.tmp_bytes else None
        if out is None:
            out = torch.empty(self.B, C, sh, sw, device=dev, dtype=torch.float32)
        elif tuple(out.shape) != (self.B, C, sh, sw) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise ValueError("prepare_images: out must be a dense float32 (B,C,S_h,S_w) tensor on the images' device")
        self.out = out
        self._ready = _uploads_done(dev)

    @property
    def plan(self) -> np.ndarray:
        """What the launcher chose per image (structured array): ``fused`` (1: the one-launch kernel), its band height ``ny``,
        staged source rows per round ``rb`` and LDS rows ``nr_cap``; ``tmp_off`` on the two-launch route."""
        off = int(self.header.off_images)
        return self.table_host[off:off + self.B * _PREP_RECORD_DTYPE.itemsize].view(_PREP_RECORD_DTYPE)

    @property
    def algorithmic_bytes(self) -> int:
        """Sources read once, the float32 batch written once."""
        return sum(im.numel() for im in self.images) + self.out.numel() * 4

    def run(self) -> torch.Tensor:
        with torch.cuda.device(self._dev):
            _wait_uploads(self._ready, self._dev)
            call("attwarp_prep_images_u8", self.table_host.ctypes.data, ptr(self.table_dev), ptr(self.tmp), ptr(self.out),
                 stream_ptr(self._dev))
        return self.out


class PreparedAttention:
    """One batch of float32 [h_i,w_i] GPU attention maps planned for ``attwarp_prep_attention_f32`` (see PreparedImages)."""

    def __init__(self, maps: Sequence[torch.Tensor], image_size=512, normalize: bool = True, out: Optional[torch.Tensor] = None):
        sh, sw = _size(image_size)
        maps = list(maps)
        if not maps:
            raise ValueError("prepare_attention_maps: empty batch")
        for m in maps:
            if not isinstance(m, torch.Tensor):
                raise TypeError("PreparedAttention: float32 [h,w] GPU tensors expected (prepare_attention_maps uploads arrays)")
        dev = require_gpu(*maps)
        for m in maps:
            if m.dtype != torch.float32:
                raise TypeError(f"prepare_attention_maps: maps must be float32 (got {m.dtype})")
            if m.dim() != 2:
                raise ValueError(f"prepare_attention_maps: maps must be [h,w] (got {tuple(m.shape)}; average a third axis first)")
            if m.numel() == 0:
                raise ValueError("prepare_attention_maps: empty map")
        self.maps = [m if m.is_contiguous() else m.contiguous() for m in maps]
        self.B, self.S_h, self.S_w, self._dev = len(maps), sh, sw, dev
        rec = np.zeros(self.B, dtype=_PREP_ATTENTION_DTYPE)
        ix = [_nearest_table(int(m.shape[1]), sw, dev) for m in self.maps]
        iy = [_nearest_table(int(m.shape[0]), sh, dev) for m in self.maps]
        rec["map"] = [m.data_ptr() for m in self.maps]
        rec["idx_x"] = [t.data_ptr() for t in ix]; rec["idx_y"] = [t.data_ptr() for t in iy]
        rec["h"] = [int(m.shape[0]) for m in self.maps]; rec["w"] = [int(m.shape[1]) for m in self.maps]
        rec["normalize"] = int(bool(normalize))
        self._keep = ix + iy
        self.records = uploaded(rec, dev)
        self.ws = torch.empty(int(_lib.load().attwarp_prep_attention_workspace_bytes(self.B)), device=dev, dtype=torch.uint8)
        if out is None:
            out = torch.empty(self.B, 1, sh, sw, device=dev, dtype=torch.float32)
        elif tuple(out.shape) != (self.B, 1, sh, sw) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise ValueError("prepare_attention_maps: out must be a dense float32 (B,1,S_h,S_w) tensor on the maps' device")
        self.out = out
        self._ready = _uploads_done(dev)

    @property
    def algorithmic_bytes(self) -> int:
        return sum(m.numel() for m in self.maps) * 4 + self.out.numel() * 4

    def run(self) -> torch.Tensor:
        with torch.cuda.device(self._dev):
            _wait_uploads(self._ready, self._dev)
            call("attwarp_prep_attention_f32", ptr(self.records), self.B, self.S_h, self.S_w, ptr(self.ws), ptr(self.out),
                 stream_ptr(self._dev))
        return self.out


def prepare_images(images, image_size=512) -> torch.Tensor:
    """``T.Resize(image_size)`` + ``T.ToTensor()`` of every image, stacked: (B,C,S_h,S_w) float32 on the GPU.

    ``images``: uint8 [H_i,W_i,3] (or, all of them, [H_i,W_i,1]) GPU tensors -- for instance the views
    ``pipeline.upload_images`` returns -- or, all of them, host images, which go through ``upload_images`` (one transfer):
    numpy arrays [H_i,W_i,C] keep their channel count, PIL images are always taken as RGB (an "L" image arrives with three
    equal channels, as ``im.convert("RGB")`` in the reference's loader, so it cannot be mixed with [H,W,1] arrays).
    ``image_size``: an int or (H, W)."""
    _size(image_size)
    images = list(images)
    if not images:
        raise ValueError("prepare_images: empty batch")
    if not any(isinstance(im, torch.Tensor) for im in images):
        for im in images:
            if hasattr(im, "convert"):          # a PIL image: upload_images takes it as RGB
                continue
            a = np.asarray(im)
            if a.dtype != np.uint8:
                raise TypeError(f"prepare_images: images must be uint8 (got {a.dtype})")
            if a.ndim != 3:
                raise ValueError(f"prepare_images: images must be [H,W,C] (got {a.shape})")
        images = pipeline.upload_images(images)
    return PreparedImages(images, image_size).run()


def prepare_attention_maps(maps, image_size=512, normalize: bool = True) -> torch.Tensor:
    """The attention tensors of the same samples: (B,1,S_h,S_w) float32 on the GPU.

    ``maps``: float32 [h_i,w_i] GPU tensors or numpy arrays (uploaded in one transfer).  ``normalize=True`` is the
    npy / raw branch of ``_load_attention_map_from_artifact`` (division by a maximum above 1); ``normalize=False`` the
    overlay branch, whose values gray / 255 are taken as they are.  NaN and +-inf become 0 and values are clipped to
    [0, 1] either way (identities on the overlay branch)."""
    _size(image_size)
    maps = list(maps)
    if not maps:
        raise ValueError("prepare_attention_maps: empty batch")
    if not any(isinstance(m, torch.Tensor) for m in maps):
        arrs = [np.asarray(m) for m in maps]
        for a in arrs:
            if a.dtype != np.float32:
                raise TypeError(f"prepare_attention_maps: maps must be float32 (got {a.dtype})")
            if a.ndim != 2:
                raise ValueError(f"prepare_attention_maps: maps must be [h,w] (got {a.shape}; average a third axis first)")
            if a.size == 0:
                raise ValueError("prepare_attention_maps: empty map")
        dev = _lib.default_device()
        host = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in arrs])
        maps = packed_views(uploaded(host, dev).view(torch.float32), [a.shape for a in arrs])
    return PreparedAttention(maps, image_size, normalize).run()


def transform_for_sample(dataset_name: Any, bucket: Any, mapping: Dict[str, str]) -> str:
    """The transform name of one sample, by the rule of MN/data.py:32-47: only GQA samples (any dataset name that holds
    "gqa", whatever its case) have per-bucket transforms, looked up under ``str(bucket)`` in the caller's ``mapping`` with
    "sqrt" for a bucket it does not list; every other sample, one without a dataset name included, gets "iden"."""
    name = "" if dataset_name is None else str(dataset_name).lower()
    if "gqa" not in name:
        return "iden"
    return mapping.get(None if bucket is None else str(bucket), "sqrt")


def transforms_for_batch(datasets, buckets, mapping: Dict[str, str]) -> List[str]:
    datasets, buckets = list(datasets), list(buckets)
    if len(datasets) != len(buckets):
        raise ValueError(f"transforms_for_batch: {len(datasets)} dataset names for {len(buckets)} buckets")
    return [transform_for_sample(d, b, mapping) for d, b in zip(datasets, buckets)]


def collate(images, attention_maps, questions, answers, datasets, buckets, image_size=512, normalize: bool = True) -> dict:
    """``collate_str`` (MN/data.py:10-24) on decoded samples: the same keys, ``image`` and ``attention_map`` on the GPU."""
    cols = [list(c) for c in (images, attention_maps, questions, answers, datasets, buckets)]
    if len({len(c) for c in cols}) != 1:
        raise ValueError("collate: images, attention_maps, questions, answers, datasets and buckets must have one length "
                         f"(got {[len(c) for c in cols]})")
    return {"image": prepare_images(cols[0], image_size),
            "attention_map": prepare_attention_maps(cols[1], image_size, normalize),
            "q_str": cols[2], "answer": cols[3], "dataset": cols[4], "bucket": cols[5]}


def prepare_trainer_batch(images, attention_maps, questions, answers, datasets, buckets, mapping: Dict[str, str],
                          image_size=512, grid=(pipeline.GRID, pipeline.GRID), normalize: bool = True) -> dict:
    """``collate`` followed by the trainer's attention targets (``pipeline.trainer_attention_targets``, MN/trainer.py:173-236)
    with the per-sample transforms of ``transforms_for_batch``: the collated batch plus ``transforms``, ``A`` (B,1,gh,gw),
    ``px_gt`` (B,gw) and ``py_gt`` (B,gh)."""
    batch = collate(images, attention_maps, questions, answers, datasets, buckets, image_size, normalize)
    batch["transforms"] = transforms_for_batch(batch["dataset"], batch["bucket"], mapping)
    batch["A"], batch["px_gt"], batch["py_gt"] = pipeline.trainer_attention_targets(batch["attention_map"], batch["transforms"], grid)
    return batch
