"""Measure the GPU JPEG decoder on files of the layouts ``all_layouts=True`` adds (attwarp_amd.jpeg.JpegFiles).

    python tools/jpegfmt_bench.py [--out profiles/jpegfmt_bench.json] [--only ENCODING:KIND:CASE --loops N]

Cases: B = 32 and B = 256 photo-like pictures of 500 x 500 (tests/png_cases.photo rolled to B different images), quality 75.
Encodings of the same pictures:
  420      Pillow's 4:2:0, decoded WITHOUT the keyword: the parent's route, the reference point of every ratio below;
  cmyk     the picture converted to CMYK and written by Pillow with four full-size components;
  440      the 4:2:2 file with the luma factors rewritten to 1 x 2 (500 x 500 again: the same MCUs, 63 to a row);
  411      the 4:2:0 file with the luma factors rewritten to 4 x 1 and the size to 500 x 512 (the same 1024 MCUs, 16 to a row).
The rewritten files hold scrambled pictures (the MCUs land elsewhere) but the entropy data, block counts and every kernel's
work are a real file's; Pillow decodes them and is compared with.  Kinds: plain (no restart markers: sub-streams) and rows
(one restart interval per MCU row of the file as decoded).
Per case, encoding and kind, one process, ONE run:
  * JpegFiles.run on a planned batch (HIP events around the five launches), and its ratio to the 420 run of the same
    pictures and kind next to the ratio of their block counts; plain files also with substreams=False;
  * decode_jpeg (marker walk, one upload, five launches, the status read back) against the route users take today,
    Image.open(...).convert("RGB") on 16 threads + pipeline.upload_images, both on the host clock around a synchronise.
--only runs JpegFiles.run of one batch N times and nothing else: the workload for a kernel trace, in a run of its own.
None of these numbers is a pass mark.  Times: HIP events around n back-to-back calls after a warm-up, median of 5 groups."""
import argparse
import io
import json
import os
import struct
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from jpegdec_bench import images, substream_summary, timed, wall  # noqa: E402

CASES = {"500x500_B32": 32, "500x500_B256": 256}
S = 500
# encoding -> (Pillow's keywords, new luma factors or None, (W, H) as decoded, MCUs per row as decoded, blocks per MCU)
ENCODINGS = {"420": (dict(subsampling=2), None, (S, S), 32, 6), "cmyk": (dict(subsampling=0), None, (S, S), 63, 4),
             "440": (dict(subsampling=1), 0x12, (S, S), 63, 4), "411": (dict(subsampling=2), 0x41, (S, 512), 16, 6)}


def sof_rewritten(f, luma, size):
    """The SOF0 segment's size and first component's factors rewritten in place."""
    at = f.index(b"\xff\xc0") + 4
    b = bytearray(f)
    b[at + 1:at + 5] = struct.pack(">HH", size[1], size[0])
    b[at + 7] = luma
    return bytes(b)


def make_files(encoding, kind, imgs):
    from PIL import Image
    kw, luma, size, per_row, _ = ENCODINGS[encoding]

    def one(a):
        im = Image.fromarray(a)
        bio = io.BytesIO()
        (im.convert("CMYK") if encoding == "cmyk" else im).save(bio, "JPEG", quality=75, **kw, **({"restart_marker_blocks": per_row} if kind == "rows" else {}))
        return sof_rewritten(bio.getvalue(), luma, size) if luma else bio.getvalue()

    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(one, imgs))


def blocks(encoding):
    _, _, (W, H), per_row, per_mcu = ENCODINGS[encoding]
    mh = {"420": 16, "cmyk": 8, "440": 16, "411": 8}[encoding]
    return per_row * -(-H // mh) * per_mcu


def measure(dev, encoding, kind, files):
    from PIL import Image
    from attwarp_amd import jpeg, pipeline
    kw = {} if encoding == "420" else {"all_layouts": True}
    res = {"encoding": encoding, "kind": kind, "file_bytes": int(sum(len(f) for f in files)), "blocks_per_image": blocks(encoding)}
    jf = jpeg.JpegFiles(files, device=dev, **kw)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    assert jf.parts is None and jf.all_layouts == (encoding != "420")
    res["equals_pillow"] = bool(all(np.array_equal(v.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB")))
                                    for v, f in list(zip(views, files))[:4]))
    res["units_per_image_mean"] = float(np.mean(jf.units()))
    res["substreams"] = substream_summary(jf)
    res["pixel_bytes"], res["compressed_bytes"] = jf.out_bytes, jf.compressed_bytes
    res["run"] = timed(jf.run)
    del jf
    if kind == "plain":
        off = jpeg.JpegFiles(files, device=dev, substreams=False, **kw)
        res["run_substreams_off"] = timed(off.run, n=1, groups=3)
        del off

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB")

    with ThreadPoolExecutor(16) as pool:
        res["host_pillow_16_threads_plus_upload"] = wall(lambda: pipeline.upload_images(list(pool.map(one, files)), dev))
    res["decode_jpeg_incl_plan_and_upload"] = wall(lambda: jpeg.decode_jpeg(files, device=dev, **kw))
    res["host_over_decode_jpeg"] = res["host_pillow_16_threads_plus_upload"]["us_median"] / res["decode_jpeg_incl_plan_and_upload"]["us_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegfmt_bench.json"))
    ap.add_argument("--only", default=None, help="ENCODING:KIND:CASE -- run JpegFiles.run of that batch --loops times and exit (for a kernel trace)")
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of " + ", ".join(CASES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpegfmt_bench needs a GPU"
    from attwarp_amd import jpeg
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    if args.only:
        encoding, kind, case = args.only.split(":")
        jf = jpeg.JpegFiles(make_files(encoding, kind, images(CASES[case], ((S, S),))), device=dev, all_layouts=encoding != "420")
        for _ in range(args.loops):
            jf.run()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": 1, "files": "quality 75, 500 x 500 pictures", "cases": []}
    for case in args.cases.split(","):
        imgs = images(CASES[case], ((S, S),))
        entry = {"case": case, "B": CASES[case], "rows": []}
        base = {}
        for kind in ("plain", "rows"):
            for encoding in ENCODINGS:
                r = measure(dev, encoding, kind, make_files(encoding, kind, imgs))
                if encoding == "420":
                    base[kind] = r
                else:
                    r["run_over_420_run"] = r["run"]["us_median"] / base[kind]["run"]["us_median"]
                    r["blocks_over_420_blocks"] = r["blocks_per_image"] / base[kind]["blocks_per_image"]
                    r["slower_than_the_block_ratio"] = bool(r["run_over_420_run"] > r["blocks_over_420_blocks"])
                entry["rows"].append(r)
                print(json.dumps({"case": case, **r}), flush=True)
                torch.cuda.empty_cache()
        res["cases"].append(entry)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
