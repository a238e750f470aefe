"""Measure what ``progressive=True`` costs and saves in the GPU JPEG encoder (attwarp_amd.jpeg.JpegBatch).

    python tools/jpegprogenc_bench.py [--out profiles/jpegprogenc_bench.json]
    python tools/jpegprogenc_bench.py --one-run 500x500_B256 [--restart-rows 1]     # three runs of the progressive batch and nothing else, for
        rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/jpegprogenc_bench.py --one-run 500x500_B256
    python tools/jpegprogenc_bench.py --shares 500x500_B256=DIR/..._kernel_trace.csv [...]    # writes profiles/jpegprogenc_kernel_shares.json (no GPU)

The three rows of DESIGN.md 3.20's table (B = 32 and 256 images of 500 x 500 x 3, 256 of 1024 x 1024 x 3; the photo-like
content of tools/jpegenc_bench.py; quality 75, 4:2:0), all routes in ONE process:
  * JpegBatch.run on a planned batch (HIP events) with ``optimize=True`` and with ``progressive=True``, without restart markers
    and with ``restart_rows=1``, and the ratios progressive / optimised;
  * ``encode_jpeg`` end to end (plan, launches, download of the compressed bytes), wall clock, and its ratio;
  * file bytes progressive / optimised / plain, beside Pillow's own three files for the first six images (the distinct contents);
  * whether the first file of each route equals Pillow's;
  * this project's ``decode_jpeg`` of the progressive files written with ``restart_rows=1`` against the baseline files of the
    same pictures (wall clock, parse and plan included).
Per-kernel shares come from a kernel trace in a process of its own (--one-run, then --shares).  No number here is a pass mark.
Times: HIP events around n back-to-back calls after a warm-up, median of 3 groups; n shrinks where one call takes long."""
import argparse
import io
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from jpegenc_bench import CASES, images_of  # noqa: E402
from png_bench import rate, timed, wall  # noqa: E402

ROUTES = {"plain": dict(), "optimize": dict(optimize=True), "progressive": dict(progressive=True)}


def calls_for(fn, budget_s=4.0):
    """Back-to-back calls per group so that the three groups stay within the budget."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-5)
    return max(1, min(10, int(budget_s / 3 / one)))


def pillow_file(a, restart_rows, route):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", restart_marker_rows=restart_rows, **ROUTES[route])
    return bio.getvalue()


def case(name, images):
    from attwarp_amd import jpeg, png
    B = int(images.shape[0])
    res = {"case": name, "B": B, "image": list(images.shape[1:]), "quality": 75, "subsampling": "4:2:0"}
    first = images[0].cpu().numpy()
    files = {}
    for rr in (0, 1):
        for route, kw in ROUTES.items():
            batch = jpeg.JpegBatch(images, restart_rows=rr, **kw)
            n = calls_for(batch.run)
            r = {"bound_bytes": batch.bound, "scratch_bytes": int(batch.scratch.numel()),
                 "run": rate(timed(batch.run, n=n, groups=3, warm=1), batch.algorithmic_bytes())}
            out = png.download(*batch.run())
            files[route, rr] = out
            r["file_bytes"] = sum(len(f) for f in out)
            r["first_file_equals_pillow"] = bool(pillow_file(first, rr, route) == out[0])
            del batch
            if route != "plain":
                r["encode_jpeg_incl_plan_and_download"] = wall(lambda: jpeg.encode_jpeg(images, restart_rows=rr, **kw), n=2)
            res[f"{route}_restart_rows_{rr}"] = r
        p, o = res[f"progressive_restart_rows_{rr}"], res[f"optimize_restart_rows_{rr}"]
        res[f"run_progressive_over_optimize_restart_rows_{rr}"] = p["run"]["us_median"] / o["run"]["us_median"]
        res[f"encode_jpeg_progressive_over_optimize_restart_rows_{rr}"] = (p["encode_jpeg_incl_plan_and_download"]["us_median"] /
                                                                           o["encode_jpeg_incl_plan_and_download"]["us_median"])
        res[f"file_bytes_progressive_over_optimize_restart_rows_{rr}"] = p["file_bytes"] / o["file_bytes"]
        res[f"file_bytes_progressive_over_plain_restart_rows_{rr}"] = p["file_bytes"] / res[f"plain_restart_rows_{rr}"]["file_bytes"]
    sizes = {route: 0 for route in ROUTES}
    for a in images[:6].cpu().numpy():
        for route in ROUTES:
            sizes[route] += len(pillow_file(a, 0, route))
    res["pillow_bytes_first_6"] = sizes
    res["pillow_progressive_over_optimize_first_6"] = sizes["progressive"] / sizes["optimize"]
    # this project's reader on the files with one restart interval per row of every scan
    dev = images.device
    prog, base = files["progressive", 1], files["plain", 1]
    res["decode_jpeg_progressive_restart_rows_1"] = wall(lambda: jpeg.decode_jpeg(prog, "RGB", device=dev, progressive=True), n=2)
    res["decode_jpeg_baseline_restart_rows_1"] = wall(lambda: jpeg.decode_jpeg(base, "RGB", device=dev), n=2)
    res["decode_progressive_over_baseline"] = (res["decode_jpeg_progressive_restart_rows_1"]["us_median"] /
                                               res["decode_jpeg_baseline_restart_rows_1"]["us_median"])
    return res


def shares(specs, out):
    """Per-kernel time of the traced runs (rocprofv3 --kernel-trace --output-format csv), microseconds per run."""
    import csv
    import re
    res = {}
    for spec in specs:
        name, path = spec.split("=", 1)
        rows = [r for r in csv.DictReader(open(path)) if re.search(r"jpeg(enc|opt|progenc)_\w+_kernel", r["Kernel_Name"])]
        tot = {}
        for r in rows:
            k = re.search(r"(jpeg(?:enc|opt|progenc)_\w+?)_kernel", r["Kernel_Name"]).group(1)
            tot[k] = tot.get(k, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        runs = sum(bool(re.search(r"jpegprogenc_clear_kernel", r["Kernel_Name"])) for r in rows)
        total = sum(tot.values())
        res[name] = {"workload": name + ", progressive=True", "runs": runs, "kernel_us_per_run": {k: round(v / runs / 1e3, 1) for k, v in tot.items()},
                     "share_percent": {k: round(100 * v / total, 2) for k, v in tot.items()}, "sum_us_per_run": round(total / runs / 1e3, 1)}
    doc = {"tool": "rocprofv3 --kernel-trace --output-format csv -- python tools/jpegprogenc_bench.py --one-run CASE [--restart-rows R]",
           "note": "one run; a process of its own, separate from the timed runs; the first run of the process included", "traces": res}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-run", choices=sorted(CASES), help="three runs of this case's progressive batch and nothing else")
    ap.add_argument("--restart-rows", type=int, default=0)
    ap.add_argument("--cases", nargs="+", default=sorted(CASES, key=list(CASES).index))
    ap.add_argument("--shares", nargs="+", default=None, help="NAME=kernel_trace.csv ...: write the per-kernel shares and exit")
    args = ap.parse_args()
    if args.shares:
        shares(args.shares, args.out or os.path.join(ROOT, "profiles", "jpegprogenc_kernel_shares.json"))
        return
    out = args.out or os.path.join(ROOT, "profiles", "jpegprogenc_bench.json")
    assert torch.cuda.is_available(), "jpegprogenc_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    if args.one_run:
        from attwarp_amd import jpeg
        batch = jpeg.JpegBatch(images_of(dev, *CASES[args.one_run]), restart_rows=args.restart_rows, progressive=True)
        for _ in range(3):
            batch.run()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": "one run", "cases": []}
    for name in args.cases:
        images = images_of(dev, *CASES[name])
        res["cases"].append(case(name, images))
        print(json.dumps(res["cases"][-1]), flush=True)
        del images
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:                             # after every case: a long case that is cut short loses only itself
            json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
