"""Measure the PNG decoder's wave route (inflate="wave") against its lane route on one-stream files.

    python tools/pngwave_bench.py [--out profiles/pngwave_bench.json] [--cases ...] [--only KIND:CASE[:lane|wave] --loops N]

Cases and kinds are those of tools/pngdec_bench.py (rle1: zlib Z_RLE level 1 on SUB rows, as cv2.imwrite writes; pillow:
Pillow's default save; B = 32 / 256 x 500 x 500 x 3 and 256 x 1024 x 1024 x 3) and, as case "fmt_500x500_B32", the RGB-8
("plain") and palette-8 rows of tools/pngfmt_bench.py with all_formats=True.  Per case and kind, in ONE process and run:
  * PngFiles.run with inflate="lane" and with inflate="wave" (HIP events; the compressed bytes are already on the device),
    what wave_info() says (images accepted, windows, rounds per window, resolution rounds) and whether both outputs are equal;
  * decode_png with either keyword and Image.open(...).convert("RGB") on 16 threads + pipeline.upload_images, on the host clock.
--only runs PngFiles.run of one kind and case N times and nothing else: the workload for a kernel trace, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pngwave_bench.py --only pillow:500x500_B256:wave --loops 3
--shares KIND=DIR/..._kernel_trace.csv [...] turns such traces into profiles/pngwave_kernel_shares.json (no GPU needed).
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

import pngdec_bench as PB                             # noqa: E402  (the same pictures, files and timers)
import pngfmt_bench as FB                             # noqa: E402

CASES = dict(PB.CASES, fmt_500x500_B32=(32, 500))
KINDS = {"500x500_B32": ("rle1", "pillow"), "500x500_B256": ("rle1", "pillow"), "1024x1024_B256": ("rle1", "pillow"),
         "fmt_500x500_B32": ("plain", "palette8")}


def files_of(case, kind, dev):
    B, side = CASES[case]
    imgs = PB.images(B, side)
    if case.startswith("fmt_"):
        return FB.make_files(kind, imgs), True
    return PB.make_files(kind, imgs, dev), False


def measure(dev, kind, files, all_formats):
    from PIL import Image
    from attwarp_amd import pipeline, png
    res = {"kind": kind, "file_bytes": int(sum(len(f) for f in files)), "all_formats": all_formats}
    outs = {}
    for inflate in ("lane", "wave"):
        pf = png.PngFiles(files, device=dev, all_formats=all_formats, inflate=inflate)
        _, status = pf.run()
        assert status.cpu().tolist() == [0] * len(files)
        outs[inflate] = pf.buffer.clone()
        res["pixel_bytes"], res["compressed_bytes"] = pf.out_bytes, pf.compressed_bytes
        res["serial_route_images"] = sum(r[0] == 1 for r in pf.routes())
        res[f"run_{inflate}"] = PB.timed(pf.run)
        if inflate == "wave":
            info = pf.wave_info(resolution=True)
            res["wave"] = {"segment_bytes": pf.segment_bytes, "max_rounds": pf.max_rounds, "accepted_images": sum(i[2] for i in info),
                           "windows_per_image_mean": float(np.mean([i[0] for i in info])),
                           "rounds_per_window_mean": float(sum(i[1] for i in info) / max(1, sum(i[0] for i in info))),
                           "resolution_rounds_per_image_mean": float(np.mean([i[3] for i in info]))}
        del pf
    res["outputs_equal"] = bool(torch.equal(outs["lane"], outs["wave"]))
    res["lane_over_wave"] = res["run_lane"]["us_median"] / res["run_wave"]["us_median"]
    del outs

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB")

    with ThreadPoolExecutor(16) as pool:
        res["host_pillow_16_threads_plus_upload"] = PB.wall(lambda: pipeline.upload_images(list(pool.map(one, files)), dev))
    for inflate in ("lane", "wave"):
        res[f"decode_png_{inflate}_incl_plan_and_upload"] = PB.wall(lambda: png.decode_png(files, device=dev, all_formats=all_formats, inflate=inflate))
        res[f"host_over_decode_png_{inflate}"] = (res["host_pillow_16_threads_plus_upload"]["us_median"] /
                                                  res[f"decode_png_{inflate}_incl_plan_and_upload"]["us_median"])
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
        res[kind] = {"workload": kind, "runs": runs, "kernel_us_per_run": {k: round(v / runs / 1e3, 1) for k, v in tot.items()},
                     "share_percent": {k: round(100 * v / total, 2) for k, v in tot.items()}, "sum_us_per_run": round(total / runs / 1e3, 1)}
    with open(out, "w") as f:
        json.dump({"tool": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/pngwave_bench.py --only KIND:CASE:wave --loops 3",
                   "note": "a run of its own, separate from profiles/pngwave_bench.json", "traces": res}, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pngwave_bench.json"))
    ap.add_argument("--only", default=None, help="KIND:CASE[:lane|wave] -- run PngFiles.run of that batch --loops times and exit")
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of " + ", ".join(CASES))
    ap.add_argument("--shares", nargs="+", default=None, help="KIND=kernel_trace.csv ...: write the per-kernel shares file and exit")
    args = ap.parse_args()
    if args.shares:
        shares(args.shares, args.out if args.out.endswith("shares.json") else os.path.join(ROOT, "profiles", "pngwave_kernel_shares.json"))
        return
    assert torch.cuda.is_available(), "pngwave_bench needs a GPU"
    from attwarp_amd import png
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    if args.only:
        kind, case, *rest = args.only.split(":")
        files, fmt = files_of(case, kind, dev)
        pf = png.PngFiles(files, device=dev, all_formats=fmt, inflate=rest[0] if rest else "wave")
        for _ in range(args.loops):
            pf.run()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": 1, "cases": []}
    for case in args.cases.split(","):
        B, side = CASES[case]
        entry = {"case": case, "B": B, "image": [side, side, 3], "kinds": []}
        for kind in KINDS[case]:
            files, fmt = files_of(case, kind, dev)
            entry["kinds"].append(measure(dev, kind, files, fmt))
            print(json.dumps({"case": case, **entry["kinds"][-1]}), flush=True)
            torch.cuda.empty_cache()
        res["cases"].append(entry)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
