"""Measure the Jet heat-map overlay (attwarp_heatmap_overlay: per-block min / max, then colour + blend) on the GPU.

    python tools/overlay_bench.py [--out FILE]

Cases (blend_mask style, uint8 up-sampled masks, the chain's layout: images packed back to back as upload_images packs
them, masks packed like a RaggedBatch's ``mota``):
  * the TextVQA-like size mix of the chain benchmarks (bench.py TEXTVQA_LIKE_WH, cycled) at B = 32 and B = 256;
  * B = 256 images of 1024 x 1024;
  * B = 256 images of 1024 x 683 (rows of 2049 bytes, every image at an odd byte address) against 1024 x 684;
  * the B = 32 mix with float32 maps (save_warped style), for reference;
  * the whole pipeline.heatmap_overlay_ragged call at B = 32 (records uploaded + workspace allocated per call).
Bytes: the floor of the algorithm -- the map read twice (min / max pass, then the colour pass), the image read once,
the output written once: 8 bytes per pixel for a uint8 map (14 for float32).  Fraction of peak = bytes / time / 8 TB/s.
Every case cycles through a ring of independent batches of >= 1 GiB (the 256 MiB Infinity Cache holds none of them
between two uses).  Times: CUDA events around n back-to-back calls (launches of both kernels included), median of 5."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXTVQA_LIKE_WH = [(1024, 768), (683, 1024), (1024, 1024), (500, 375), (333, 500), (640, 427)]      # as bench.py


def make_batch(sizes_hw, dev, dtype=torch.uint8, shift=1, seed=0):
    """Images packed back to back from byte `shift` of one buffer, maps packed the same way, outputs packed too."""
    g = torch.Generator(device=dev).manual_seed(seed)
    npx = [h * w for h, w in sizes_hw]
    ibuf = torch.randint(0, 256, (shift + 3 * sum(npx),), device=dev, dtype=torch.uint8, generator=g)
    esz = torch.empty((), dtype=dtype).element_size()
    mbuf = torch.empty(sum(npx) + 16, device=dev, dtype=dtype)
    obuf = torch.empty(3 * sum(npx) + 16, device=dev, dtype=torch.uint8)
    imgs, maps, outs, io, mo = [], [], [], shift, 0
    for (h, w), n in zip(sizes_hw, npx):
        imgs.append(ibuf[io:io + 3 * n].view(h, w, 3))
        small = torch.rand(1, 1, 24, 24, device=dev, generator=g) ** 3
        up = torch.nn.functional.interpolate(small, size=(h, w), mode="bilinear", align_corners=False)[0, 0]
        m = (up * 255).to(torch.uint8) if dtype == torch.uint8 else up.to(dtype)
        mbuf[mo:mo + n].copy_(m.reshape(-1))
        maps.append(mbuf[mo:mo + n].view(h, w))
        outs.append(obuf[io - shift:io - shift + 3 * n].view(h, w, 3))
        io += 3 * n
        mo += n
    return imgs, maps, outs, esz


class Prepared:
    """One batch's records on the device and its workspace: the timed loop is the library call alone."""

    def __init__(self, imgs, maps, outs, style, alpha=0.5):
        from attwarp_amd import _lib, pipeline
        self.lib, self.B = _lib.load(), len(imgs)
        rec = np.zeros(self.B, dtype=pipeline._OVERLAY_IMAGE_DTYPE)
        rec["image"] = [t.data_ptr() for t in imgs]; rec["map"] = [t.data_ptr() for t in maps]
        rec["out"] = [t.data_ptr() for t in outs]
        rec["H"] = [t.shape[0] for t in imgs]; rec["W"] = [t.shape[1] for t in imgs]
        self.rec = rec
        self.rec_dev = torch.from_numpy(rec.view(np.uint8).copy()).to(imgs[0].device)
        self.ws = torch.empty(self.lib.attwarp_overlay_workspace_bytes(self.B), device=imgs[0].device, dtype=torch.uint8)
        self.args = (rec.ctypes.data, _lib.ptr(self.rec_dev), self.B, _lib.dtype_id(maps[0]), pipeline.OVERLAY_STYLES[style],
                     float(alpha), _lib.RGB, _lib.RGB, _lib.ptr(self.ws))
        self.keep = (imgs, maps, outs)

    def __call__(self):
        from attwarp_amd import _lib
        _lib.call("attwarp_heatmap_overlay", *self.args, _lib.stream_ptr(self.ws.device))


def time_calls(fns, n, reps=5):
    for f in fns[:3] if len(fns) >= 3 else fns * 2:
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n):
            fns[i % len(fns)]()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / n)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def case(name, sizes_hw, dev, ring_bytes=1 << 30, dtype=torch.uint8, style="blend_mask", shift=1, n=None):
    px = sum(h * w for h, w in sizes_hw)
    esz = torch.empty((), dtype=dtype).element_size()
    per_px = 2 * esz + 6
    nbytes = px * per_px
    ring = max(2, -(-ring_bytes // (px * (6 + esz))))
    preps = []
    for r in range(ring):
        imgs, maps, outs, _ = make_batch(sizes_hw, dev, dtype, shift, seed=r)
        preps.append(Prepared(imgs, maps, outs, style))
    n = n or max(4 * ring, min(200, int(2e9 // nbytes)))
    med, lo, hi = time_calls(preps, n)
    res = {"case": name, "B": len(sizes_hw), "pixels": px, "map_dtype": str(dtype).replace("torch.", ""), "style": style,
           "bytes": nbytes, "bytes_per_px": per_px, "us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2),
           "TBps": round(nbytes / med / 1e6, 3), "frac_of_8TBps": round(nbytes / med / 1e6 / 8.0, 3), "ring": ring, "calls": n}
    del preps
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "overlay_bench measures on a GPU"
    dev = torch.device("cuda:0")
    mix = lambda B: [(h, w) for (w, h) in (TEXTVQA_LIKE_WH[b % len(TEXTVQA_LIKE_WH)] for b in range(B))]
    rows = [case("textvqa_mix", mix(32), dev), case("textvqa_mix", mix(256), dev),
            case("square_1024", [(1024, 1024)] * 256, dev, shift=0),
            case("w684_aligned", [(1024, 684)] * 256, dev, shift=0), case("w683_odd_address", [(1024, 683)] * 256, dev, shift=1),
            case("textvqa_mix_f32", mix(32), dev, dtype=torch.float32, style="save_warped", shift=1)]
    # the whole Python call on a ragged batch (records + workspace per call) next to the chain step of the same batch
    from attwarp_amd import pipeline
    sizes = mix(32)
    g = torch.Generator(device=dev).manual_seed(9)
    host = [np.random.default_rng(b).integers(0, 256, (h, w, 3), dtype=np.uint8) for b, (h, w) in enumerate(sizes)]
    imgs = pipeline.upload_images(host, dev)
    a24 = torch.rand(32, 24, 24, device=dev, generator=g) ** 3
    _, rb = pipeline.warp_from_masks_ragged(imgs, a24, (500, 500), return_batch=True)
    med, lo, hi = time_calls([lambda: pipeline.heatmap_overlay_ragged(rb)], 50)
    px = sum(h * w for h, w in sizes)
    rows.append({"case": "heatmap_overlay_ragged_call", "B": 32, "pixels": px, "us": round(med, 2), "us_min": round(lo, 2),
                 "us_max": round(hi, 2), "note": "python call incl. record upload + workspace; same batch every call (cache-warm)"})
    r683 = next(r for r in rows if r["case"] == "w683_odd_address")["us"]
    r684 = next(r for r in rows if r["case"] == "w684_aligned")["us"]
    mix32 = rows[0]["us"]
    summary = {"w683_over_w684": round(r683 / r684, 3), "mix32_overlay_us": mix32,
               "mix32_overlay_over_51us_chain_step": round(mix32 / 51.0, 3),
               "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    lines = []
    for r in rows:
        lines.append(json.dumps(r))
    lines.append(json.dumps(summary))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
