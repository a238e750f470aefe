"""Measure the GPU JPEG encoder (attwarp_amd.jpeg.JpegBatch) on what the driver loop saves.

    python tools/jpegenc_bench.py [--out profiles/jpegenc_bench.json]
    python tools/jpegenc_bench.py --one-run 500x500_B256      # one JpegBatch.run of a case, for a kernel trace of its own

Cases: B = 32 and 256 images of 500 x 500 x 3 and 256 of 1024 x 1024 x 3, the synthetic photo-like content of
tools/png_bench.py, quality 75, 4:2:0, restart_rows 0 and 1.  Per case, one process:
  * JpegBatch.run on a planned batch (HIP events around the seven launches);
  * a plain streaming launch (csrc/calib.hip, tuning flavour) that reads the same pixel bytes once and writes as many bytes as
    the files take: the ruler;
  * PngBatch.run on the same images;
  * file bytes against the PNG files and against the pixels;
  * end to end: ``encode_jpeg`` (plan, launches, download of the compressed bytes) against the host route it replaces, download
    of the raw pixels + ``Image.save`` per image on 16 threads, both wall clock around a synchronise.
None of these numbers is a pass mark.  Times: HIP events around n back-to-back calls after a warm-up, median of 5 groups."""
import argparse
import ctypes
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from png_bench import photo_like, rate, timed, wall  # noqa: E402

CASES = {"500x500_B32": (32, 500), "500x500_B256": (256, 500), "1024x1024_B256": (256, 1024)}


def images_of(dev, B, size):
    gen = torch.Generator(device=dev).manual_seed(7)
    protos = [photo_like(size, size, dev, gen, k) for k in range(6)]
    return torch.stack([torch.roll(protos[b % 6], shifts=(17 * b, 29 * b), dims=(0, 1)) for b in range(B)])


def case(dev, name, images, restart_rows):
    from PIL import Image
    from attwarp_amd import _lib, jpeg, png
    B = int(images.shape[0])
    res = {"case": name, "B": B, "image": list(images.shape[1:]), "quality": 75, "subsampling": "4:2:0", "restart_rows": restart_rows}
    batch = jpeg.JpegBatch(images, restart_rows=restart_rows)
    nbytes = batch.algorithmic_bytes()
    res["units"] = batch.units
    res["bound_bytes"] = batch.bound
    res["scratch_bytes"] = int(batch.scratch.numel())
    res["encode"] = rate(timed(batch.run), nbytes)
    files = png.download(*batch.run())
    total = sum(len(f) for f in files)
    res["file_bytes"] = total
    res["files_over_pixels"] = total / nbytes
    bio = io.BytesIO()
    Image.fromarray(images[0].cpu().numpy()).save(bio, "JPEG", restart_marker_rows=restart_rows)
    res["first_file_equals_pillow"] = bool(bio.getvalue() == files[0])

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
    del dst, batch

    pb = png.PngBatch(images)
    res["png_encode"] = rate(timed(pb.run), nbytes)
    png_total = int(pb.run()[1][-1])
    res["png_file_bytes"] = png_total
    res["jpeg_over_png_bytes"] = total / png_total
    res["jpeg_over_png_time"] = res["encode"]["us_median"] / res["png_encode"]["us_median"]
    del pb

    def save(a):
        b = io.BytesIO()
        Image.fromarray(a).save(b, "JPEG", restart_marker_rows=restart_rows)
        return b.tell()

    with ThreadPoolExecutor(16) as pool:
        def host_path():
            return sum(pool.map(save, images.cpu().numpy()))
        res["host_download_pillow_16_threads"] = wall(host_path)
    res["encode_jpeg_incl_plan_and_download"] = wall(lambda: jpeg.encode_jpeg(images, restart_rows=restart_rows))
    res["host_over_encode_jpeg"] = res["host_download_pillow_16_threads"]["us_median"] / res["encode_jpeg_incl_plan_and_download"]["us_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegenc_bench.json"))
    ap.add_argument("--one-run", choices=sorted(CASES), help="one JpegBatch.run of this case (restart_rows 0, then 1) and nothing else")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpegenc_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    if args.one_run:
        from attwarp_amd import jpeg
        images = images_of(dev, *CASES[args.one_run])
        for rr in (0, 1):
            jpeg.JpegBatch(images, restart_rows=rr).run()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": "one run", "cases": []}
    for name, (B, size) in CASES.items():
        images = images_of(dev, B, size)
        for rr in (0, 1):
            res["cases"].append(case(dev, name, images, rr))
            print(json.dumps(res["cases"][-1]), flush=True)
        del images
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
