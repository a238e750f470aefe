"""Measure the GPU PNG encoder (attwarp_amd.png) on what the driver loop saves.

    python tools/png_bench.py [--out profiles/png_bench.json]

Cases: the 500 x 500 x 3 warped outputs of the TextVQA-like size mix (tests/test_gpu_parity.py) at B = 32 and B = 256
(photo-like synthetic sources through warp_from_masks_ragged), and 256 images of 1024 x 1024 x 3.  Per case, one process:
  * PngBatch.run on a planned batch (HIP events around the three launches), SUB filter;
  * a plain streaming launch (csrc/calib.hip, tuning flavour) that reads the same pixel bytes once and writes as many
    bytes as the files take: the ruler; fractions of the 8 TB/s peak are on the pixel bytes read for both;
  * sizes on the first 16 images: this encoder's zlib stream against zlib's own Z_RLE level 1 on the same filtered bytes,
    Pillow's files at compress_level = 1 and at its default, and the raw pixels;
  * the host route this replaces: download of the raw pixels + Pillow ``save`` per image on 16 threads, against
    ``encode_png`` (plan, three launches, download of the compressed bytes), both wall clock around a synchronise.
None of these numbers is a pass mark.  Times: HIP events around n back-to-back calls after a warm-up, median of 5 groups."""
import argparse
import ctypes
import io
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXTVQA_LIKE_WH = [(1024, 768), (683, 1024), (1024, 1024), (500, 375), (333, 500), (640, 427)]      # as tests/test_gpu_parity.py
HBM_PEAK = 8.0e12
SAMPLE = 16


def timed(fn, n=10, groups=5, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / n)
    return {"us_median": float(np.median(per)), "us_min": float(min(per)), "us_max": float(max(per)), "calls_per_group": n,
            "groups": groups, "timer": "HIP events"}


def wall(fn, n=3):
    fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e6)
    return {"us_median": float(np.median(per)), "us_min": float(min(per)), "us_max": float(max(per)), "calls": n,
            "timer": "wall clock incl. host"}


def rate(entry, nbytes):
    entry["pixel_bytes"] = int(nbytes)
    entry["bytes_per_s"] = nbytes / (entry["us_median"] * 1e-6)
    entry["fraction_of_8TBs_peak"] = entry["bytes_per_s"] / HBM_PEAK
    return entry


def photo_like(h, w, dev, gen, k):
    """Smooth colour gradients, a few hard edges and sensor-like noise: uint8 [h,w,3] on the device."""
    yy = torch.arange(h, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(w, device=dev, dtype=torch.float32)[None, :]
    ch = []
    for c in range(3):
        v = 120 + 70 * torch.sin(xx / (23.0 + 5 * c + k % 7)) * torch.cos(yy / (31.0 + 3 * c + k % 5)) + 0.05 * (xx + yy)
        v = v + 40 * ((xx // 64 + yy // 48) % 2) * (c == k % 3)
        ch.append(v + torch.randn(h, w, device=dev, generator=gen) * 2.5)
    return torch.stack(ch, -1).clamp(0, 255).to(torch.uint8)


def case(dev, name, images):
    from PIL import Image
    from attwarp_amd import _lib, png
    B = int(images.shape[0])
    res = {"case": name, "B": B, "image": list(images.shape[1:]), "filter": "sub"}
    batch = png.PngBatch(images)
    nbytes = batch.algorithmic_bytes()
    res["segments"] = batch.segments
    res["bound_bytes"] = batch.bound
    res["encode"] = rate(timed(batch.run), nbytes)
    files = png.download(*batch.run())
    total = sum(len(f) for f in files)
    res["file_bytes"] = total
    res["files_over_pixels"] = total / nbytes
    first = np.asarray(Image.open(io.BytesIO(files[0])))
    res["pillow_decodes_to_source"] = bool(np.array_equal(first, images[0].cpu().numpy()))

    tl = _lib.load_tuning()
    read, write = nbytes // 16 * 16, total // 16 * 16
    dst = torch.empty(write, device=dev, dtype=torch.uint8)
    flat = images.reshape(-1)
    st = _lib.stream_ptr(dev)

    def copy():
        rc = tl.attwarp_debug_stream_copy(ctypes.c_void_p(flat.data_ptr()), read, ctypes.c_void_p(dst.data_ptr()), write, st)
        assert rc == 0
    res["stream_copy_same_bytes"] = rate(timed(copy), nbytes)
    res["encode_over_copy"] = res["encode"]["us_median"] / res["stream_copy_same_bytes"]["us_median"]
    del dst

    host = images[:SAMPLE].cpu().numpy()
    sizes = {"images": int(host.shape[0]), "pixels": int(host.size), "zlib_stream": 0, "zlib_rle_level1": 0, "file": 0,
             "pillow_level1_file": 0, "pillow_default_file": 0}
    for im, f in zip(host, files):
        z = f[41:41 + int.from_bytes(f[33:37], 'big')]          # signature 8, IHDR 25, IDAT length + type 8
        raw = zlib.decompress(z)
        c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        sizes["zlib_stream"] += len(z)
        sizes["zlib_rle_level1"] += len(c.compress(raw) + c.flush())
        sizes["file"] += len(f)
        for key, kw in (("pillow_level1_file", {"compress_level": 1}), ("pillow_default_file", {})):
            bio = io.BytesIO()
            Image.fromarray(im).save(bio, "PNG", **kw)
            sizes[key] += bio.tell()
    sizes["stream_over_zlib_rle"] = sizes["zlib_stream"] / sizes["zlib_rle_level1"]
    sizes["file_over_pillow_level1"] = sizes["file"] / sizes["pillow_level1_file"]
    sizes["file_over_pillow_default"] = sizes["file"] / sizes["pillow_default_file"]
    res["sizes_first_images"] = sizes

    def save(a):
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, "PNG")
        return bio.tell()

    with ThreadPoolExecutor(16) as pool:
        def host_path():
            return sum(pool.map(save, images.cpu().numpy()))
        res["host_download_pillow_16_threads"] = wall(host_path)
    res["encode_png_incl_plan_and_download"] = wall(lambda: png.encode_png(images))
    res["host_over_encode_png"] = res["host_download_pillow_16_threads"]["us_median"] / res["encode_png_incl_plan_and_download"]["us_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "png_bench needs a GPU"
    from attwarp_amd import pipeline
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    gen = torch.Generator(device=dev).manual_seed(7)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "cases": []}
    protos = [photo_like(h, w, dev, gen, k) for k, (w, h) in enumerate(TEXTVQA_LIKE_WH)]
    for B in (32, 256):
        srcs = [protos[b % len(protos)] for b in range(B)]
        masks = torch.rand(B, 24, 24, device=dev, generator=gen) ** 3
        out = pipeline.warp_from_masks_ragged(srcs, masks, (500, 500))
        res["cases"].append(case(dev, f"textvqa_mix_B{B}_warped_500x500", out))
        print(json.dumps(res["cases"][-1]), flush=True)
        del out
        torch.cuda.empty_cache()
    big = torch.stack([torch.roll(protos[2], shifts=(17 * b, 29 * b), dims=(0, 1)) for b in range(256)])
    res["cases"].append(case(dev, "1024x1024_B256", big))
    print(json.dumps(res["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
