"""Measure the GPU JPEG decoder (attwarp_amd.jpeg.JpegFiles) on files like those the drivers open.

    python tools/jpegdec_bench.py [--out profiles/jpegdec_bench.json] [--only KIND:CASE --loops N]

Cases: B = 32 and B = 256 files of a TextVQA-like size mix (1024 x 768, 768 x 1024, 1024 x 683, 1024 x 1024, 800 x 600,
640 x 480, cycling), and 256 files of 1024 x 1024; photo-like content (tests/png_cases.photo, eight prototypes per size
rolled to B different images), written by Pillow at quality 75, 4:2:0.  File kinds:
  plain    Pillow's default: no restart markers, ONE decoding unit per file: self-synchronising sub-streams (one workgroup
           per file, one lane per segment), or with them off one wave, one lane per file;
  rows     restart_marker_rows=1: one unit per MCU row.
Per case and kind, one process, ONE run:
  * JpegFiles.run on a planned batch (HIP events around the five launches; the compressed bytes are already on the device);
    for plain files also with substreams=False ("run_substreams_off") and over --sweep segment sizes, with the rounds and
    accepted counts the device reports;
  * a plain streaming launch (csrc/calib.hip, tuning flavour) that reads and writes as many bytes as the decoded pixels: the ruler;
  * the route users take today: Image.open(...).convert("RGB") on 16 threads + pipeline.upload_images, against
    decode_jpeg (marker walk, ONE upload of the compressed bytes, five launches, the status read back), both on the host
    clock around a synchronise, both including their upload.
--only runs JpegFiles.run of one kind and case N times and nothing else: the workload for a kernel trace, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/jpegdec_bench.py --only plain:mix_B256 --loops 3
--shares KIND=DIR/..._kernel_trace.csv [...] turns such traces into profiles/jpegdec_kernel_shares.json (no GPU needed).
None of these numbers is a pass mark.  Times: HIP events around n back-to-back calls after a warm-up, median of 5 groups."""
import argparse
import ctypes
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MIX = ((768, 1024), (1024, 768), (683, 1024), (1024, 1024), (600, 800), (480, 640))        # (H, W)
CASES = {"mix_B32": (32, MIX), "mix_B256": (256, MIX), "1024x1024_B256": (256, ((1024, 1024),))}
KINDS = {"plain": {}, "rows": {"restart_marker_rows": 1}}


def timed(fn, n=3, groups=5, warm=1):
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


def images(B, sizes):
    import png_cases as PC
    protos = {s: [PC.photo(s[0], s[1], 3, 40 + k) for k in range(4)] for s in sizes}
    return [np.roll(protos[sizes[b % len(sizes)]][(b // len(sizes)) % 4], (17 * b, 29 * b), (0, 1)) for b in range(B)]


def make_files(kind, imgs):
    from PIL import Image

    def one(a):
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, "JPEG", quality=75, subsampling=2, **KINDS[kind])
        return bio.getvalue()

    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(one, imgs))


def substream_summary(jf):
    info = jf.substream_info()
    planned = [i for i in info if i[0]]
    return {"segment_bytes": jf.segment_bytes, "max_rounds": jf.max_rounds, "images_planned": len(planned),
            "images_accepted": int(sum(i[2] for i in planned)), "segments_mean": float(np.mean([i[0] for i in planned])) if planned else 0.0,
            "rounds_max": max([i[1] for i in planned], default=0), "rounds_mean": float(np.mean([i[1] for i in planned])) if planned else 0.0}


def measure(dev, kind, files, sweep=()):
    from PIL import Image
    from attwarp_amd import _lib, jpeg, pipeline
    res = {"kind": kind, "file_bytes": int(sum(len(f) for f in files))}
    if kind == "plain":
        off = jpeg.JpegFiles(files, device=dev, substreams=False)
        res["run_substreams_off"] = timed(off.run, n=1, groups=3)
        first = off.buffer.clone()
        del off
        res["sweep"] = []
        for sb in sweep:
            sw = jpeg.JpegFiles(files, device=dev, segment_bytes=sb)
            entry = timed(sw.run)
            entry.update(substream_summary(sw), equals_substreams_off=bool(torch.equal(sw.buffer, first)))
            res["sweep"].append(entry)
            del sw
        del first
    jf = jpeg.JpegFiles(files, device=dev)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    res["substreams"] = substream_summary(jf)
    res["equals_pillow"] = bool(all(np.array_equal(v.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB")))
                                    for v, f in list(zip(views, files))[:6]))
    res["units_per_image_mean"] = float(np.mean(jf.units()))
    res["pixel_bytes"] = jf.out_bytes
    res["compressed_bytes"] = jf.compressed_bytes
    res["scratch_bytes"] = int(jf.scratch.numel())
    res["run"] = timed(jf.run)
    res["run"]["pixel_bytes_per_s"] = jf.out_bytes / (res["run"]["us_median"] * 1e-6)
    res["run"]["compressed_bytes_per_s"] = jf.compressed_bytes / (res["run"]["us_median"] * 1e-6)
    tl = _lib.load_tuning()
    nb = jf.out_bytes // 16 * 16
    src, dst = torch.empty(nb, device=dev, dtype=torch.uint8), torch.empty(nb, device=dev, dtype=torch.uint8)
    st = _lib.stream_ptr(dev)

    def copy():
        assert tl.attwarp_debug_stream_copy(ctypes.c_void_p(src.data_ptr()), nb, ctypes.c_void_p(dst.data_ptr()), nb, st) == 0
    res["stream_copy_same_bytes"] = timed(copy)
    res["run_over_copy"] = res["run"]["us_median"] / res["stream_copy_same_bytes"]["us_median"]
    del src, dst, jf

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB")

    with ThreadPoolExecutor(16) as pool:
        res["host_pillow_16_threads_plus_upload"] = wall(lambda: pipeline.upload_images(list(pool.map(one, files)), dev))
    res["decode_jpeg_incl_plan_and_upload"] = wall(lambda: jpeg.decode_jpeg(files, device=dev))
    res["host_over_decode_jpeg"] = res["host_pillow_16_threads_plus_upload"]["us_median"] / res["decode_jpeg_incl_plan_and_upload"]["us_median"]
    return res


def shares(specs, out):
    import csv
    import re
    res = {}
    for spec in specs:
        kind, path = spec.split("=", 1)
        rows = [r for r in csv.DictReader(open(path)) if "jpegdec_" in r["Kernel_Name"]]
        tot = {}
        for r in rows:
            name = re.search(r"jpegdec_(\w+?)_kernel", r["Kernel_Name"]).group(1)
            tot[name] = tot.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        runs = sum("jpegdec_scan" in r["Kernel_Name"] for r in rows)
        total = sum(tot.values())
        res[kind] = {"workload": f"{kind}:mix_B256", "runs": runs,
                     "kernel_us_per_run": {k: round(v / runs / 1e3, 1) for k, v in tot.items()},
                     "share_percent": {k: round(100 * v / total, 2) for k, v in tot.items()}, "sum_us_per_run": round(total / runs / 1e3, 1)}
    with open(out, "w") as f:
        json.dump({"tool": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/jpegdec_bench.py --only KIND:mix_B256 --loops 3",
                   "note": "a run of its own, separate from profiles/jpegdec_bench.json", "traces": res}, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegdec_bench.json"))
    ap.add_argument("--only", default=None, help="KIND:CASE -- run JpegFiles.run of that batch --loops times and exit (for a kernel trace)")
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of " + ", ".join(CASES))
    ap.add_argument("--sweep", default="64,128,256", help="segment sizes the plain rows are also run with ('' for none)")
    ap.add_argument("--substreams", default="auto", choices=("auto", "off"), help="with --only: the plan of the traced run")
    ap.add_argument("--shares", nargs="+", default=None, help="KIND=kernel_trace.csv ...: write the per-kernel shares file and exit")
    args = ap.parse_args()
    if args.shares:
        shares(args.shares, args.out if args.out.endswith("shares.json") else os.path.join(ROOT, "profiles", "jpegdec_kernel_shares.json"))
        return
    assert torch.cuda.is_available(), "jpegdec_bench needs a GPU"
    from attwarp_amd import jpeg
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    if args.only:
        kind, case = args.only.split(":")
        B, sizes = CASES[case]
        jf = jpeg.JpegFiles(make_files(kind, images(B, sizes)), device=dev, substreams="auto" if args.substreams == "auto" else False)
        for _ in range(args.loops):
            jf.run()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": 1,
           "files": "Pillow, quality 75, 4:2:0", "cases": []}
    for case in args.cases.split(","):
        B, sizes = CASES[case]
        imgs = images(B, sizes)
        entry = {"case": case, "B": B, "sizes_HW": [list(s) for s in sizes], "kinds": []}
        for kind in KINDS:
            entry["kinds"].append(measure(dev, kind, make_files(kind, imgs), [int(s) for s in args.sweep.split(",") if s]))
            print(json.dumps({"case": case, **entry["kinds"][-1]}), flush=True)
            torch.cuda.empty_cache()
        res["cases"].append(entry)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
