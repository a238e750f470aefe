"""Measure the GPU decode of PROGRESSIVE JPEG files (attwarp_amd.jpeg.JpegFiles with progressive=True).

    python tools/jpegprog_bench.py [--out profiles/jpegprog_bench.json] [--cases mix_B32,mix_B256,1024x1024_B256]

The size mix, the 1024 x 1024 case and the pictures of tools/jpegdec_bench.py, written by Pillow at quality 75, 4:2:0,
progressive=True: "plain" (no restart markers: ONE lane per scan, as many in flight as the scan's level holds; sub-streams
for progressive scans do not exist yet) and "rows" (restart_marker_rows=1: one wave per MCU row of every scan).
Per case and kind, one process, ONE run:
  * JpegFiles.run with the level plan and with levels=False (one entropy launch per scan position), HIP events;
  * decode_jpeg(progressive=True) on the host clock (marker walk over all scans, one upload, the launches, the status);
  * (a) the host route: Image.open(...).convert("RGB") on 16 threads + pipeline.upload_images for the same files;
  * (b) the BASELINE encoding of the same pictures (same quality, sampling and restart option) through today's path,
    JpegFiles.run and decode_jpeg, in the same process.
None of these numbers is a pass mark."""
import argparse
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import jpegdec_bench as JB  # noqa: E402


def make_files(kind, imgs, progressive):
    from PIL import Image

    def one(a):
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, "JPEG", quality=75, subsampling=2, progressive=progressive, **JB.KINDS[kind])
        return bio.getvalue()

    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(one, imgs))


def ms(t):
    return round(t["us_median"] / 1e3, 3)


def measure(dev, kind, imgs):
    from PIL import Image
    from attwarp_amd import jpeg, pipeline
    files, base = make_files(kind, imgs, True), make_files(kind, imgs, False)
    res = {"kind": kind, "file_bytes": int(sum(len(f) for f in files)), "baseline_file_bytes": int(sum(len(f) for f in base))}
    jf = jpeg.JpegFiles(files, device=dev, progressive=True)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    res["equals_pillow"] = bool(all(np.array_equal(v.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB")))
                                    for v, f in list(zip(views, files))[:6]))
    res["scans_per_image"] = len(jf.parsed[0]["scans"])
    res["levels"] = max(jf.levels())
    res["units_per_image_mean"] = float(np.mean(jf.units()))
    res["pixel_bytes"], res["scratch_bytes"] = jf.out_bytes, int(jf.scratch.numel())
    n = 1 if kind == "plain" else 3
    res["run_levels"] = JB.timed(jf.run, n=n, groups=3)
    first = jf.buffer.clone()
    del jf
    flat = jpeg.JpegFiles(files, device=dev, progressive=True, levels=False)
    res["run_one_launch_per_scan"] = JB.timed(flat.run, n=n, groups=3)
    res["one_launch_per_scan_equals_levels"] = bool(torch.equal(flat.buffer, first))
    del flat, first
    bf = jpeg.JpegFiles(base, device=dev)
    res["baseline_run"] = JB.timed(bf.run)
    del bf

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB")

    with ThreadPoolExecutor(16) as pool:
        res["host_pillow_16_threads_plus_upload"] = JB.wall(lambda: pipeline.upload_images(list(pool.map(one, files)), dev))
    res["decode_jpeg_progressive"] = JB.wall(lambda: jpeg.decode_jpeg(files, device=dev, progressive=True))
    res["baseline_decode_jpeg"] = JB.wall(lambda: jpeg.decode_jpeg(base, device=dev))
    res["ms"] = {"run_levels": ms(res["run_levels"]), "run_one_launch_per_scan": ms(res["run_one_launch_per_scan"]),
                 "baseline_run": ms(res["baseline_run"]), "decode_jpeg_progressive": ms(res["decode_jpeg_progressive"]),
                 "baseline_decode_jpeg": ms(res["baseline_decode_jpeg"]), "host_route": ms(res["host_pillow_16_threads_plus_upload"])}
    res["host_over_decode_jpeg_progressive"] = res["ms"]["host_route"] / res["ms"]["decode_jpeg_progressive"]
    res["progressive_over_baseline_run"] = res["ms"]["run_levels"] / res["ms"]["baseline_run"]
    res["one_launch_per_scan_over_levels"] = res["ms"]["run_one_launch_per_scan"] / res["ms"]["run_levels"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegprog_bench.json"))
    ap.add_argument("--cases", default=",".join(JB.CASES), help="comma-separated subset of " + ", ".join(JB.CASES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpegprog_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": 1,
           "files": "Pillow, quality 75, 4:2:0, progressive=True; baseline: the same pictures without it", "cases": []}
    for case in args.cases.split(","):
        B, sizes = JB.CASES[case]
        imgs = JB.images(B, sizes)
        entry = {"case": case, "B": B, "sizes_HW": [list(s) for s in sizes], "kinds": []}
        for kind in JB.KINDS:
            entry["kinds"].append(measure(dev, kind, imgs))
            print(json.dumps({"case": case, **entry["kinds"][-1]}), flush=True)
            torch.cuda.empty_cache()
        res["cases"].append(entry)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                        # after every case: a partial file survives a time limit
            json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
