"""Measure what the PNG decoder's formats path costs (attwarp_amd.png.PngFiles(all_formats=True)).

    python tools/pngfmt_bench.py [--out profiles/pngfmt_bench.json] [--only KIND --loops N]

One case: B = 32 files of 500 x 500, the same photo-like pictures (tests/png_cases.photo, eight prototypes rolled to 32
different images) written five ways by the tests' hand writer (tests/pngfmt_cases.hand: SUB filter on every row, zlib level 6,
one IDAT), so that the kinds differ in format alone:
  plain     RGB at 8 bits, non-interlaced: the parent's seven launches (the table has no format flag);
  plain_mixed  the same 32 files and a 1 x 1 palette file behind them: every file through the formats kernel, which is how
            the new kernel compares with the old one on the same bytes;
  adam7     the same pixels, Adam7-interlaced;
  palette8  quantised to 256 colours by Pillow, colour type 3;
  grey1     thresholded luma, 1 bit;
  rgb16     every sample x 257, 16 bits.
Per kind, one process, ONE run:
  * PngFiles.run on a planned batch (HIP events around the launches; the compressed bytes are already on the device);
  * the route users take today: Image.open(...).convert("RGB") on 16 threads + pipeline.upload_images, against decode_png
    (chunk walk, ONE upload of the compressed bytes, the launches, the status read back), both on the host clock around a
    synchronise, both including their upload.
--only runs PngFiles.run of one kind N times and nothing else: the workload for a kernel trace, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pngfmt_bench.py --only adam7 --loops 3
--shares KIND=DIR/..._kernel_trace.csv [...] turns such traces into profiles/pngfmt_kernel_shares.json (no GPU needed).
None of these numbers is a pass mark.  Times: HIP events around n back-to-back calls after a warm-up, median of 5 groups."""
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

from pngdec_bench import images, timed, wall          # noqa: E402  (the same pictures and timers as the parent path's bench)

B, SIDE = 32, 500
KINDS = ("plain", "plain_mixed", "adam7", "palette8", "grey1", "rgb16")


def make_file(kind, a):
    from PIL import Image
    import pngfmt_cases as C
    sub = lambda p, r: 1
    if kind in ("plain", "adam7"):
        return C.hand(kind, a.astype(np.uint16), 2, 8, int(kind == "adam7"), sub).file
    if kind == "rgb16":
        return C.hand(kind, a.astype(np.uint16) * 257, 2, 16, 0, sub).file
    if kind == "grey1":
        g = np.asarray(Image.fromarray(a).convert("L"))
        return C.hand(kind, (g >= 128).astype(np.uint16)[:, :, None], 0, 1, 0, sub).file
    q = Image.fromarray(a).quantize(256)
    pal = bytes(q.getpalette()[:768])
    return C.hand(kind, np.asarray(q).astype(np.uint16)[:, :, None], 3, 8, 0, sub, pal).file


def make_files(kind, imgs):
    import pngfmt_cases as C
    with ThreadPoolExecutor(16) as pool:
        files = list(pool.map(lambda a: make_file("plain" if kind == "plain_mixed" else kind, a), imgs))
    if kind == "plain_mixed":
        files.append(C.hand("dot", np.zeros((1, 1, 1), np.uint16), 3, 8, 0, lambda p, r: 0, bytes(3)).file)
    return files


def measure(dev, kind, files):
    from PIL import Image
    from attwarp_amd import pipeline, png
    res = {"kind": kind, "file_bytes": int(sum(len(f) for f in files))}
    pf = png.PngFiles(files, device=dev, all_formats=True)
    views, status = pf.run()
    assert status.cpu().tolist() == [0] * len(files)

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB")

    res["equals_pillow"] = bool(all(np.array_equal(v.cpu().numpy(), np.asarray(one(f))) for v, f in list(zip(views, files))[:4]))
    res["format_flag"] = int(pf.header.formats)
    res["launches"] = 9 if pf.header.formats else 7
    routes = pf.routes()
    res["unit_route_images"] = sum(r[0] == 0 for r in routes)
    res["pixel_bytes"] = pf.out_bytes
    res["compressed_bytes"] = pf.compressed_bytes

    def filtered(f):
        W, H, ctype, _, depth, lace, _ = png.parse_png(f, 0, True)
        return png.filtered_bytes(W, H, {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype], depth, lace)

    res["filtered_bytes"] = int(sum(filtered(f) for f in files))
    res["run"] = timed(pf.run)
    res["run"]["pixel_bytes_per_s"] = pf.out_bytes / (res["run"]["us_median"] * 1e-6)
    del pf
    with ThreadPoolExecutor(16) as pool:
        res["host_pillow_16_threads_plus_upload"] = wall(lambda: pipeline.upload_images(list(pool.map(one, files)), dev))
    res["decode_png_incl_plan_and_upload"] = wall(lambda: png.decode_png(files, device=dev, all_formats=True))
    res["host_over_decode_png"] = res["host_pillow_16_threads_plus_upload"]["us_median"] / res["decode_png_incl_plan_and_upload"]["us_median"]
    return res


def shares(specs, out):
    import csv
    import re
    res = {}
    for spec in specs:
        kind, path = spec.split("=", 1)
        rows = [r for r in csv.DictReader(open(path)) if "pngdec_" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        tot, n_inflate = {}, 0
        for r in rows:
            name = re.search(r"pngdec_(\w+?)_kernel", r["Kernel_Name"]).group(1)
            if name == "inflate":
                name = "inflate_count" if n_inflate % 2 == 0 else "inflate_write"
                n_inflate += 1
            tot[name] = tot.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        runs, total = n_inflate // 2, sum(tot.values())
        res[kind] = {"workload": f"{kind}: B = {B} x {SIDE} x {SIDE}", "runs": runs,
                     "kernel_us_per_run": {k: round(v / runs / 1e3, 1) for k, v in tot.items()},
                     "share_percent": {k: round(100 * v / total, 2) for k, v in tot.items()}, "sum_us_per_run": round(total / runs / 1e3, 1)}
    with open(out, "w") as f:
        json.dump({"tool": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/pngfmt_bench.py --only KIND --loops 3",
                   "note": "runs of their own, separate from profiles/pngfmt_bench.json; the two launches of pngdec_inflate_kernel in a run "
                           "are split by dispatch order (first: count, second: write + serial route)", "traces": res}, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pngfmt_bench.json"))
    ap.add_argument("--only", default=None, help="KIND -- run PngFiles.run of that batch --loops times and exit (for a kernel trace)")
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--shares", nargs="+", default=None, help="KIND=kernel_trace.csv ...: write the per-kernel shares file and exit")
    args = ap.parse_args()
    if args.shares:
        shares(args.shares, args.out if args.out.endswith("shares.json") else os.path.join(ROOT, "profiles", "pngfmt_kernel_shares.json"))
        return
    assert torch.cuda.is_available(), "pngfmt_bench needs a GPU"
    from attwarp_amd import png
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    imgs = images(B, SIDE)
    if args.only:
        pf = png.PngFiles(make_files(args.only, imgs), device=dev, all_formats=True)
        for _ in range(args.loops):
            pf.run()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": 1, "B": B, "image": [SIDE, SIDE], "kinds": []}
    for kind in KINDS:
        res["kinds"].append(measure(dev, kind, make_files(kind, imgs)))
        print(json.dumps(res["kinds"][-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
