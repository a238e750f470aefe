"""Measure what ``optimize=True`` costs and saves in the GPU JPEG encoder (attwarp_amd.jpeg.JpegBatch).

    python tools/jpegopt_bench.py [--out profiles/jpegopt_bench.json]
    python tools/jpegopt_bench.py --one-run 500x500_B256        # three runs of the optimised batch and nothing else, for
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/jpegopt_bench.py --one-run 500x500_B256
    python tools/jpegopt_bench.py --shares 500x500_B256=DIR/..._kernel_trace.csv [...]    # adds the shares to the file (no GPU)

The three rows of DESIGN.md 3.20's table (B = 32 and 256 images of 500 x 500 x 3, 256 of 1024 x 1024 x 3; the photo-like
content of tools/jpegenc_bench.py; quality 75, 4:2:0, no restart markers), the keyword off and on in ONE process:
  * JpegBatch.run on a planned batch (HIP events; seven launches off, ten on) and the ratio on / off;
  * ``encode_jpeg`` end to end (plan, launches, download of the compressed bytes), wall clock, and its ratio;
  * file bytes on / off, and the same ratio of Pillow's two files for the first six images (the distinct contents);
  * whether the first file of each route equals Pillow's.
Per-kernel shares come from a kernel trace in a process of its own (--one-run, then --shares).  No number here is a pass mark.
Times: HIP events around n back-to-back calls after a warm-up, median of 5 groups."""
import argparse
import io
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from jpegenc_bench import CASES, images_of  # noqa: E402
from png_bench import rate, timed, wall  # noqa: E402


def case(name, images):
    from PIL import Image
    from attwarp_amd import jpeg, png
    B = int(images.shape[0])
    res = {"case": name, "B": B, "image": list(images.shape[1:]), "quality": 75, "subsampling": "4:2:0", "restart_rows": 0}
    for key, opt in (("off", False), ("on", True)):
        batch = jpeg.JpegBatch(images, optimize=opt)
        r = {"bound_bytes": batch.bound, "scratch_bytes": int(batch.scratch.numel()), "run": rate(timed(batch.run), batch.algorithmic_bytes())}
        files = png.download(*batch.run())
        r["file_bytes"] = sum(len(f) for f in files)
        bio = io.BytesIO()
        Image.fromarray(images[0].cpu().numpy()).save(bio, "JPEG", optimize=opt)
        r["first_file_equals_pillow"] = bool(bio.getvalue() == files[0])
        del batch
        r["encode_jpeg_incl_plan_and_download"] = wall(lambda: jpeg.encode_jpeg(images, optimize=opt))
        res[key] = r
    res["run_on_over_off"] = res["on"]["run"]["us_median"] / res["off"]["run"]["us_median"]
    res["encode_jpeg_on_over_off"] = (res["on"]["encode_jpeg_incl_plan_and_download"]["us_median"] /
                                      res["off"]["encode_jpeg_incl_plan_and_download"]["us_median"])
    res["file_bytes_on_over_off"] = res["on"]["file_bytes"] / res["off"]["file_bytes"]
    sizes = [0, 0]
    for a in images[:6].cpu().numpy():
        for k, opt in enumerate((False, True)):
            bio = io.BytesIO()
            Image.fromarray(a).save(bio, "JPEG", optimize=opt)
            sizes[k] += bio.tell()
    res["pillow_bytes_on_over_off_first_6"] = sizes[1] / sizes[0]
    return res


def shares(specs, out):
    """Per-kernel time of the traced runs (rocprofv3 --kernel-trace --output-format csv), microseconds per run -> out["kernel_shares"]."""
    import csv
    import re
    res = {}
    for spec in specs:
        name, path = spec.split("=", 1)
        rows = [r for r in csv.DictReader(open(path)) if re.search(r"jpeg(enc|opt)_\w+_kernel", r["Kernel_Name"])]
        tot = {}
        for r in rows:
            k = re.search(r"(jpeg(?:enc|opt)_\w+?)_kernel", r["Kernel_Name"]).group(1)
            tot[k] = tot.get(k, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        runs = sum(bool(re.search(r"jpegopt_clear_kernel", r["Kernel_Name"])) for r in rows)
        total = sum(tot.values())
        res[name] = {"workload": name + ", optimize=True", "runs": runs, "kernel_us_per_run": {k: round(v / runs / 1e3, 1) for k, v in tot.items()},
                     "share_percent": {k: round(100 * v / total, 2) for k, v in tot.items()}, "sum_us_per_run": round(total / runs / 1e3, 1)}
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernel_shares"] = {"tool": "rocprofv3 --kernel-trace --output-format csv -- python tools/jpegopt_bench.py --one-run CASE",
                            "note": "a process of its own, separate from the timed runs; the first run of the process included", "traces": res}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegopt_bench.json"))
    ap.add_argument("--one-run", choices=sorted(CASES), help="three runs of this case's optimised batch and nothing else")
    ap.add_argument("--shares", nargs="+", default=None, help="CASE=kernel_trace.csv ...: add the per-kernel shares to the file and exit")
    args = ap.parse_args()
    if args.shares:
        shares(args.shares, args.out)
        return
    assert torch.cuda.is_available(), "jpegopt_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    if args.one_run:
        from attwarp_amd import jpeg
        batch = jpeg.JpegBatch(images_of(dev, *CASES[args.one_run]), optimize=True)
        for _ in range(3):
            batch.run()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": "one run", "cases": []}
    for name, (B, size) in CASES.items():
        images = images_of(dev, B, size)
        res["cases"].append(case(name, images))
        print(json.dumps(res["cases"][-1]), flush=True)
        del images
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
