"""Measure the GPU PNG decoder (attwarp_amd.png.PngFiles) on the files the pipeline reads back.

    python tools/pngdec_bench.py [--out profiles/pngdec_bench.json] [--only KIND:CASE --loops N]

Cases: B = 32 and B = 256 files of 500 x 500 x 3, and 256 files of 1024 x 1024 x 3, photo-like content
(tests/png_cases.photo, eight prototypes rolled to B different images).  File kinds:
  own      this project's encoder (attwarp_amd.png.encode_png, SUB): one sync point per 24 KiB segment;
  rle1     zlib Z_RLE level 1 on SUB-filtered rows, as cv2.imwrite writes: ONE stream, no sync point;
  pillow   Pillow's default save: one stream, adaptive filters.
Per case and kind, one process, ONE run:
  * PngFiles.run on a planned batch (HIP events around the seven launches; the compressed bytes are already on the device);
  * units per image as the chain kernel left them;
  * a plain streaming launch (csrc/calib.hip, tuning flavour) that reads and writes as many bytes as the decoded pixels: the ruler;
  * the route users take today: Image.open(...).convert("RGB") on 16 threads + pipeline.upload_images, against
    decode_png (chunk walk, ONE upload of the compressed bytes, seven launches, the status read back), both on the host clock
    around a synchronise, both including their upload.
--only runs PngFiles.run of one kind and case N times and nothing else: the workload for a kernel trace, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pngdec_bench.py --only own:500x500_B256 --loops 3
--shares KIND=DIR/..._kernel_trace.csv [...] turns such traces into profiles/pngdec_kernel_shares.json (no GPU needed): time per
run and share of every pngdec kernel, the two launches of pngdec_inflate_kernel split by dispatch order (count, then write).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"500x500_B32": (32, 500), "500x500_B256": (256, 500), "1024x1024_B256": (256, 1024)}
KINDS = ("own", "rle1", "pillow")


def timed(fn, n=5, groups=5, warm=2):
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


def images(B, side):
    import png_cases as PC
    protos = [PC.photo(side, side, 3, 40 + k) for k in range(8)]
    return [np.roll(protos[b % 8], (17 * b, 29 * b), (0, 1)) for b in range(B)]


def make_files(kind, imgs, dev):
    from PIL import Image
    import png_ref as R
    import pngdec_cases as C
    from attwarp_amd import png
    if kind == "own":
        out = []
        for i in range(0, len(imgs), 64):
            out += png.encode_png([torch.from_numpy(a).to(dev) for a in imgs[i:i + 64]])
        return out

    def rle1(a):
        H, W, ch = a.shape
        d = a.astype(np.int16)
        d[:, 1:] -= a[:, :-1]
        f = np.concatenate([np.ones((H, 1), np.uint8), (d & 255).astype(np.uint8).reshape(H, W * ch)], 1).tobytes()
        c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        return C.make_png(W, H, ch, c.compress(f) + c.flush(), 8192)

    def pil(a):
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, "PNG")
        return bio.getvalue()

    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(rle1 if kind == "rle1" else pil, imgs))


def measure(dev, kind, files, imgs):
    from PIL import Image
    from attwarp_amd import _lib, pipeline, png
    res = {"kind": kind, "file_bytes": int(sum(len(f) for f in files))}
    pf = png.PngFiles(files, device=dev)
    views, status = pf.run()
    assert status.cpu().tolist() == [0] * len(files)
    res["decodes_to_source"] = bool(all(np.array_equal(v.cpu().numpy(), a) for v, a in list(zip(views, imgs))[:4]))
    routes = pf.routes()
    res["unit_route_images"] = sum(r[0] == 0 for r in routes)
    res["units_per_image_mean"] = float(np.mean([r[1] if r[0] == 0 else 1 for r in routes]))
    res["pixel_bytes"] = pf.out_bytes
    res["compressed_bytes"] = pf.compressed_bytes
    res["run"] = timed(pf.run)
    res["run"]["pixel_bytes_per_s"] = pf.out_bytes / (res["run"]["us_median"] * 1e-6)
    tl = _lib.load_tuning()
    nb = pf.out_bytes // 16 * 16
    src, dst = torch.empty(nb, device=dev, dtype=torch.uint8), torch.empty(nb, device=dev, dtype=torch.uint8)
    st = _lib.stream_ptr(dev)

    def copy():
        assert tl.attwarp_debug_stream_copy(ctypes.c_void_p(src.data_ptr()), nb, ctypes.c_void_p(dst.data_ptr()), nb, st) == 0
    res["stream_copy_same_bytes"] = timed(copy)
    res["run_over_copy"] = res["run"]["us_median"] / res["stream_copy_same_bytes"]["us_median"]
    del src, dst, pf

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB")

    with ThreadPoolExecutor(16) as pool:
        res["host_pillow_16_threads_plus_upload"] = wall(lambda: pipeline.upload_images(list(pool.map(one, files)), dev))
    res["decode_png_incl_plan_and_upload"] = wall(lambda: png.decode_png(files, device=dev))
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
        res[kind] = {"workload": f"{kind}:500x500_B256", "runs": runs,
                     "kernel_us_per_run": {k: round(v / runs / 1e3, 1) for k, v in tot.items()},
                     "share_percent": {k: round(100 * v / total, 2) for k, v in tot.items()}, "sum_us_per_run": round(total / runs / 1e3, 1)}
    with open(out, "w") as f:
        json.dump({"tool": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/pngdec_bench.py --only KIND:500x500_B256 --loops 3",
                   "note": "a run of its own, separate from profiles/pngdec_bench.json; the two launches of pngdec_inflate_kernel in a run are "
                           "split by dispatch order (first: count, second: write + serial route)", "traces": res}, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pngdec_bench.json"))
    ap.add_argument("--only", default=None, help="KIND:CASE -- run PngFiles.run of that batch --loops times and exit (for a kernel trace)")
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of " + ", ".join(CASES))
    ap.add_argument("--shares", nargs="+", default=None, help="KIND=kernel_trace.csv ...: write the per-kernel shares file and exit")
    args = ap.parse_args()
    if args.shares:
        shares(args.shares, args.out if args.out.endswith("shares.json") else os.path.join(ROOT, "profiles", "pngdec_kernel_shares.json"))
        return
    assert torch.cuda.is_available(), "pngdec_bench needs a GPU"
    from attwarp_amd import png
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    if args.only:
        kind, case = args.only.split(":")
        B, side = CASES[case]
        imgs = images(B, side)
        pf = png.PngFiles(make_files(kind, imgs, dev), device=dev)
        for _ in range(args.loops):
            pf.run()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": 1, "cases": []}
    for case in args.cases.split(","):
        B, side = CASES[case]
        imgs = images(B, side)
        entry = {"case": case, "B": B, "image": [side, side, 3], "kinds": []}
        for kind in KINDS:
            entry["kinds"].append(measure(dev, kind, make_files(kind, imgs, dev), imgs))
            print(json.dumps({"case": case, **entry["kinds"][-1]}), flush=True)
            torch.cuda.empty_cache()
        res["cases"].append(entry)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
