"""Measure the GPU decode of the JPEG files only ``all_scans=True`` takes (attwarp_amd.jpeg.JpegFiles).

    python tools/jpegscan_bench.py [--out profiles/jpegscan_bench.json] [--cases 500x500_B32,500x500_B256]
    python tools/jpegscan_bench.py --only ENCODING:KIND:CASE --loops 3      (JpegFiles.run alone, for a kernel trace;
                                                                             ENCODING may also be ref_prog_420)
    python tools/jpegscan_bench.py --shares NAME=kernel_trace.csv ...       (-> profiles/jpegscan_kernel_shares.json)

B = 32 and B = 256 photo-like 500 x 500 pictures (those of tools/jpegdec_bench.py) at quality 75, three encodings of the new
kind, each without restart markers ("plain": ONE lane per scan) and with one restart interval per MCU row ("rows"):
  prog_cmyk   Pillow's progressive CMYK, four full-size components;
  prog_440    Pillow's progressive 4:2:2 with the SOF2 header rewritten to 4:4:0 (same entropy data and block counts as a
              real file of that layout, scrambled picture; Pillow decodes it);
  seq3_420    a 4:2:0 file re-written as three sequential scans, one per component, by the transcoder of tests/jpegscan_ref.py.
              That transcoder is plain Python, so at most 32 distinct pictures are transcoded and repeated over the batch.
Per encoding and kind, one process, ONE run: JpegFiles.run between HIP events (median of groups), decode_jpeg on the host
clock (marker walk over all scans, plan, one upload, the launches, the status read back), and the host route (Pillow on 16
threads + pipeline.upload_images).  References, measured in the same process and never the code under test: the
progressive 4:2:0 encoding of the same pictures through progressive=True, and the one-scan sequential
encoding of the same layout through all_layouts=True (3.19; the baseline path for 4:2:0).  None of these numbers is a pass
mark."""
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

CASES = {"500x500_B32": 32, "500x500_B256": 256}
S = 500
# encoding -> (Pillow's keywords, new luma factors or None, MCUs per row as decoded, coefficient blocks per image, the
# one-scan reference's JpegFiles keywords)
ENCODINGS = {"prog_cmyk": (dict(subsampling=0), None, 63, 63 * 63 * 4, dict(all_layouts=True)),
             "prog_440": (dict(subsampling=1), 0x12, 63, 63 * 32 * 4, dict(all_layouts=True)),
             "seq3_420": (dict(subsampling=2), None, 32, 32 * 32 * 6, dict())}
KINDS = ("plain", "rows")
BLOCKS_420 = 32 * 32 * 6


def sof_rewritten(f, luma):
    """The frame header's first component's factors rewritten in place (a square picture keeps its size)."""
    at = min(i for i in (f.find(b"\xff\xc0"), f.find(b"\xff\xc2")) if i >= 0) + 4
    b = bytearray(f)
    b[at + 7] = luma
    return bytes(b)


def pillow_files(imgs, kind, per_row, luma=None, cmyk=False, **kw):
    from PIL import Image

    def one(a):
        im = Image.fromarray(a)
        bio = io.BytesIO()
        (im.convert("CMYK") if cmyk else im).save(bio, "JPEG", quality=75, **kw, **({"restart_marker_blocks": per_row} if kind == "rows" else {}))
        return sof_rewritten(bio.getvalue(), luma) if luma else bio.getvalue()

    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(one, imgs))


def three_scans(files, kind):
    """At most 32 distinct one-scan 4:2:0 files transcoded to three sequential scans, repeated over the batch."""
    import jpegscan_ref as R
    out = []
    for f in files[:32]:
        frame, planes = R.source_planes(f)
        script = [[0], [1], [2]]
        ri = [R.scan_mcus(S, S, frame["samp"], c)[0] for c in script] if kind == "rows" else None
        out.append(R.transcode(frame, planes, script, sequential=True, ri=ri))
    return [out[b % len(out)] for b in range(len(files))]


def make_files(encoding, kind, imgs):
    """-> (files of the new kind, the one-scan sequential files of the same layout)."""
    kw, luma, per_row, _, _ = ENCODINGS[encoding]
    cmyk = encoding == "prog_cmyk"
    one_scan = pillow_files(imgs, kind, per_row, luma, cmyk, **kw)
    if encoding == "seq3_420":
        return three_scans(one_scan, kind), one_scan
    return pillow_files(imgs, kind, per_row, luma, cmyk, progressive=True, **kw), one_scan


def ms(t):
    return round(t["us_median"] / 1e3, 3)


def measure(dev, encoding, kind, imgs):
    from PIL import Image
    from attwarp_amd import jpeg, pipeline
    files, one_scan = make_files(encoding, kind, imgs)
    blocks, ref_kw = ENCODINGS[encoding][3], ENCODINGS[encoding][4]
    B = len(files)
    res = {"encoding": encoding, "kind": kind, "file_bytes": int(sum(len(f) for f in files)), "blocks_per_image": blocks}
    jf = jpeg.JpegFiles(files, device=dev, all_scans=True)
    assert jf.all_scans and jf.parts is None
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * B
    res["equals_pillow"] = bool(all(np.array_equal(v.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB")))
                                    for v, f in list(zip(views, files))[:4]))
    res["scans_per_image"], res["levels"] = len(jf.parsed[0]["scans"]), max(jf.levels())
    res["units_per_image_mean"] = float(np.mean(jf.units()))
    res["pixel_bytes"], res["scratch_bytes"] = jf.out_bytes, int(jf.scratch.numel())
    n = 1 if kind == "plain" else 3
    res["run"] = JB.timed(jf.run, n=n, groups=3)
    del jf, views
    # references of the same pictures, in the same process: progressive 4:2:0 through 3.17, the one-scan layout through 3.19
    p420 = pillow_files(imgs, kind, 32, subsampling=2, progressive=True)
    pf = jpeg.JpegFiles(p420, device=dev, progressive=True)
    assert pf.progressive
    res["ref_progressive_420"] = {"scans_per_image": len(pf.parsed[0]["scans"]), "levels": max(pf.levels()), "blocks_per_image": BLOCKS_420,
                                  "run": JB.timed(pf.run, n=n, groups=3)}
    del pf
    of = jpeg.JpegFiles(one_scan, device=dev, **ref_kw)
    res["ref_one_scan"] = {"run": JB.timed(of.run)}
    del of

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB")

    with ThreadPoolExecutor(16) as pool:
        res["host_pillow_16_threads_plus_upload"] = JB.wall(lambda: pipeline.upload_images(list(pool.map(one, files)), dev))
    res["decode_jpeg_all_scans"] = JB.wall(lambda: jpeg.decode_jpeg(files, device=dev, all_scans=True))
    run, ref = ms(res["run"]), ms(res["ref_progressive_420"]["run"])
    res["ms"] = {"run": run, "ref_progressive_420_run": ref, "ref_one_scan_run": ms(res["ref_one_scan"]["run"]),
                 "decode_jpeg_all_scans": ms(res["decode_jpeg_all_scans"]), "host_route": ms(res["host_pillow_16_threads_plus_upload"])}
    res["ns_per_block"] = {"run": 1e6 * run / (B * blocks), "ref_progressive_420_run": 1e6 * ref / (B * BLOCKS_420)}
    res["run_over_ref_progressive_420"] = run / ref
    res["blocks_over_ref_progressive_420"] = blocks / BLOCKS_420
    res["host_over_decode_jpeg"] = res["ms"]["host_route"] / res["ms"]["decode_jpeg_all_scans"]
    return res


def shares(specs, out):
    """Per-kernel time of the traced runs (rocprofv3 --kernel-trace --stats --output-format csv), microseconds per run."""
    import csv
    import re
    res = {}
    for spec in specs:
        name, path = spec.split("=", 1)
        rows = [r for r in csv.DictReader(open(path)) if re.search(r"jpeg(scan|prog|fmt|dec)_\w+_kernel", r["Kernel_Name"])]
        tot = {}
        for r in rows:
            k = re.search(r"(jpeg(?:scan|prog|fmt|dec)_\w+?)_kernel", r["Kernel_Name"]).group(1)
            tot[k] = tot.get(k, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        runs = sum(bool(re.search(r"jpeg(scan|prog)_clear_kernel", r["Kernel_Name"])) for r in rows)
        total = sum(tot.values())
        res[name] = {"workload": name, "runs": runs, "kernel_us_per_run": {k: round(v / runs / 1e3, 1) for k, v in tot.items()},
                     "share_percent": {k: round(100 * v / total, 2) for k, v in tot.items()}, "sum_us_per_run": round(total / runs / 1e3, 1)}
    with open(out, "w") as f:
        json.dump({"tool": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/jpegscan_bench.py --only ENCODING:KIND:CASE --loops 3",
                   "note": "runs of their own, separate from profiles/jpegscan_bench.json; the first run of a process included", "traces": res}, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegscan_bench.json"))
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of " + ", ".join(CASES))
    ap.add_argument("--only", default=None, help="ENCODING:KIND:CASE -- run JpegFiles.run of that batch --loops times and exit (for a kernel trace)")
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--shares", nargs="+", default=None, help="NAME=kernel_trace.csv ...: write the per-kernel shares file and exit")
    args = ap.parse_args()
    if args.shares:
        shares(args.shares, args.out if args.out.endswith("shares.json") else os.path.join(ROOT, "profiles", "jpegscan_kernel_shares.json"))
        return
    assert torch.cuda.is_available(), "jpegscan_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    if args.only:
        from attwarp_amd import jpeg
        encoding, kind, case = args.only.split(":")
        imgs = JB.images(CASES[case], ((S, S),))
        if encoding == "ref_prog_420":                        # the reference: progressive 4:2:0 of the same pictures through 3.17
            jf = jpeg.JpegFiles(pillow_files(imgs, kind, 32, subsampling=2, progressive=True), device=dev, progressive=True)
        else:
            jf = jpeg.JpegFiles(make_files(encoding, kind, imgs)[0], device=dev, all_scans=True)
        for _ in range(args.loops):
            jf.run()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": 1,
           "files": "quality 75, 500 x 500; see the module's docstring for the encodings and the references", "cases": []}
    for case in args.cases.split(","):
        imgs = JB.images(CASES[case], ((S, S),))
        entry = {"case": case, "B": CASES[case], "results": []}
        for encoding in ENCODINGS:
            for kind in KINDS:
                entry["results"].append(measure(dev, encoding, kind, imgs))
                print(json.dumps({"case": case, **{k: v for k, v in entry["results"][-1].items() if not isinstance(v, dict) or k in ("ms", "ns_per_block")}}), flush=True)
                torch.cuda.empty_cache()
        res["cases"].append(entry)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                        # after every case: a partial file survives a time limit
            json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
