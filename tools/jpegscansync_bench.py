"""Measure marker-less progressive JPEG files of the OTHER layouts with their scans cut into segments
(attwarp_amd.jpeg.JpegFiles with all_scans=True, scan_substreams="auto" / True) against the same call without
the keyword, in one process.

    python tools/jpegscansync_bench.py [--out profiles/jpegscansync_bench.json] [--cases 500x500_B32,500x500_B256]
                                       [--encodings prog_cmyk,prog_440]

The marker-less ("plain") rows of tools/jpegscan_bench.py: Pillow's progressive CMYK and progressive 4:4:0 (a 4:2:2 file with
its frame header rewritten), B = 32 and B = 256 pictures of 500 x 500 at quality 75.  Per row, ONE run:
  * JpegFiles.run with the keyword off (the yardstick: one lane per scan), True (all four kinds of scan) and "auto"
    (jpeg.AUTO_LAYOUT_SCAN_KINDS), HIP events; the whole batch checked against Pillow each time;
  * per scan kind: scans cut, scans accepted, the most rounds a scan took, the 100 MHz ticks its workgroups spent in their
    three parts (JpegFiles.scan_substream_ticks), JpegFiles.run with ONLY that kind cut and with every kind BUT that one cut
    (scan_substreams=True under the tuning library's jpegprog_sync_kinds mask).  A level takes as long as its slowest scan,
    so what decides whether a kind belongs in "auto" is the second number: it does when the run with all four kinds is
    faster than the run without it;
  * decode_jpeg with the keyword off and "auto", and the host route (Image.open(...).convert("RGB") on 16 threads +
    pipeline.upload_images), on the host clock.
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
import jpegscan_bench as SB  # noqa: E402

KINDS = ("dc_first", "dc_refine", "ac_first", "ac_refine")   # (JP_DC_FIRST .. JP_AC_REFINE: route - 1, and the mask's bit)


def measure(dev, encoding, imgs):
    from PIL import Image
    from attwarp_amd import _lib, jpeg, pipeline
    files, _ = SB.make_files(encoding, "plain", imgs)
    B = len(files)
    res = {"encoding": encoding, "file_bytes": int(sum(len(f) for f in files))}

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB")

    with ThreadPoolExecutor(16) as pool:
        want = [np.asarray(a) for a in pool.map(one, files)]

    def run(key, n, **kw):
        jf = jpeg.JpegFiles(files, device=dev, all_scans=True, **kw)
        assert jf.all_scans and jf.parts is None
        views, status = jf.run()
        assert status.cpu().tolist() == [0] * B
        res[f"{key}_equals_pillow"] = bool(all(np.array_equal(v.cpu().numpy(), w) for v, w in zip(views, want)))
        res[f"run_{key}"] = JB.timed(jf.run, n=n, groups=3)
        return jf

    jf = run("off", 1)
    res["scans_per_image"], res["levels"] = len(jf.parsed[0]["scans"]), max(jf.levels())
    del jf
    torch.cuda.empty_cache()
    jf = run("on", 3, scan_substreams=True)
    res["segment_bytes"], res["max_rounds"] = jf.segment_bytes, jf.max_rounds
    kinds = {name: {"scans": 0, "cut": 0, "accepted": 0, "max_rounds": 0, "ticks_sum": [0, 0, 0], "ticks_max_scan": [0, 0, 0]} for name in KINDS}
    for p, info, ticks in zip(jf.parsed, jf.scan_substream_info(), jf.scan_substream_ticks()):
        for s, (route, nseg, rounds, acc), t in zip(p["scans"], info, ticks):
            k = kinds[jpeg.scan_kind(s)]
            k["scans"] += 1
            k["cut"] += int(route != 0)
            k["accepted"] += acc
            k["max_rounds"] = max(k["max_rounds"], rounds)
            k["ticks_sum"] = [a + b for a, b in zip(k["ticks_sum"], t)]
            if sum(t) > sum(k["ticks_max_scan"]):
                k["ticks_max_scan"] = list(t)
    for k in kinds.values():
        tot = max(sum(k["ticks_sum"]), 1)
        k["part_shares"] = [round(a / tot, 4) for a in k["ticks_sum"]]
        k["longest_scan_ms"] = round(sum(k["ticks_max_scan"]) / 1e5, 3)
    res["scan_kinds"] = kinds
    del jf
    torch.cuda.empty_cache()
    for bit, name in enumerate(KINDS):
        for field, mask in (("run_ms_only_this_kind_cut", 1 << bit), ("run_ms_all_but_this_kind_cut", 15 ^ (1 << bit))):
            with _lib.debug_override(jpegprog_sync_kinds=mask):
                jf = jpeg.JpegFiles(files, device=dev, all_scans=True, scan_substreams=True)
                _, status = jf.run()
                assert status.cpu().tolist() == [0] * B
                t = JB.timed(jf.run, n=1, groups=3)
                del jf
            torch.cuda.empty_cache()
            kinds[name][field] = SB.ms(t)
        k = kinds[name]
        k["ms_saved_alone_against_off"] = round(SB.ms(res["run_off"]) - k["run_ms_only_this_kind_cut"], 3)
        k["ms_saved_by_adding_it_last"] = round(k["run_ms_all_but_this_kind_cut"] - SB.ms(res["run_on"]), 3)
        k["pays"] = bool(k["ms_saved_by_adding_it_last"] > 0)
    jf = run("auto", 3, scan_substreams="auto")
    res["auto_kinds"] = list(jpeg.AUTO_LAYOUT_SCAN_KINDS)
    del jf
    torch.cuda.empty_cache()
    with ThreadPoolExecutor(16) as pool:
        res["host_pillow_16_threads_plus_upload"] = JB.wall(lambda: pipeline.upload_images(list(pool.map(one, files)), dev))
    res["decode_jpeg_off"] = JB.wall(lambda: jpeg.decode_jpeg(files, device=dev, all_scans=True))
    res["decode_jpeg_auto"] = JB.wall(lambda: jpeg.decode_jpeg(files, device=dev, all_scans=True, scan_substreams="auto"))
    res["ms"] = {k: SB.ms(res[k]) for k in ("run_off", "run_on", "run_auto", "decode_jpeg_off", "decode_jpeg_auto", "host_pillow_16_threads_plus_upload")}
    res["run_off_over_auto"] = res["ms"]["run_off"] / res["ms"]["run_auto"]
    res["run_off_over_on"] = res["ms"]["run_off"] / res["ms"]["run_on"]
    res["host_over_decode_jpeg_auto"] = res["ms"]["host_pillow_16_threads_plus_upload"] / res["ms"]["decode_jpeg_auto"]
    res["host_over_decode_jpeg_off"] = res["ms"]["host_pillow_16_threads_plus_upload"] / res["ms"]["decode_jpeg_off"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegscansync_bench.json"))
    ap.add_argument("--cases", default=",".join(SB.CASES), help="comma-separated subset of " + ", ".join(SB.CASES))
    ap.add_argument("--encodings", default="prog_cmyk,prog_440")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpegscansync_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": 1,
           "files": "Pillow, quality 75, 500 x 500, progressive=True, no restart markers: CMYK, and 4:2:2 rewritten to 4:4:0", "cases": []}
    for case in args.cases.split(","):
        imgs = JB.images(SB.CASES[case], ((SB.S, SB.S),))
        entry = {"case": case, "B": SB.CASES[case], "results": []}
        for encoding in args.encodings.split(","):
            entry["results"].append(measure(dev, encoding, imgs))
            r = entry["results"][-1]
            print(json.dumps({"case": case, "encoding": encoding, "ms": r["ms"],
                              "kinds": {k: [v["cut"], v["accepted"], v["max_rounds"], v["ms_saved_by_adding_it_last"]] for k, v in r["scan_kinds"].items()}}),
                  flush=True)
            torch.cuda.empty_cache()
        res["cases"].append(entry)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                        # after every case: a partial file survives a time limit
            json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
