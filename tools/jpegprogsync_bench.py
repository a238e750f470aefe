"""Measure marker-less PROGRESSIVE JPEG files with their scans cut into segments (attwarp_amd.jpeg.JpegFiles with
progressive=True, scan_substreams="auto") against the same call without the keyword, in one process.  run_on: scan_substreams=True (all four kinds of scan);
run_auto and decode_jpeg_on: "auto".

    python tools/jpegprogsync_bench.py [--out profiles/jpegprogsync_bench.json] [--cases mix_B32,mix_B256,1024x1024_B256]

The three "no markers" rows of tools/jpegprog_bench.py: the size mix at B = 32 and B = 256 and 256 x 1024 x 1024, written by
Pillow at quality 75, 4:2:0, progressive=True, no restart markers.  Per case, ONE run:
  * JpegFiles.run with the keyword off (the yardstick: one lane per scan) and on, HIP events; the whole batch checked
    against Pillow both times;
  * per scan kind: scans cut, scans accepted, the most rounds a scan took, the 100 MHz ticks its workgroups spent in their
    three parts (JpegFiles.scan_substream_ticks: for an AC refinement masks / skim / write), JpegFiles.run with ONLY that
    kind cut and with every kind BUT that one cut (scan_substreams=True under the tuning library's jpegprog_sync_kinds
    mask).  The scans of a level run side by side and the level takes as long as its slowest scan, so a kind alone can
    only gain where it is the slowest of its level; what decides whether a kind belongs in "auto" is the second number:
    it does when the run with all four kinds is faster than the run without it;
  * JpegFiles.run with scan_substreams="auto" (jpeg.AUTO_SCAN_KINDS);
  * decode_jpeg with the keyword off and on, and the host route (Image.open(...).convert("RGB") on 16 threads +
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
import jpegprog_bench as PB  # noqa: E402

ROUTES = {1: "dc_first", 2: "dc_refine", 3: "ac_first", 4: "ac_refine"}


def measure(dev, imgs):
    from PIL import Image
    from attwarp_amd import jpeg, pipeline
    files = PB.make_files("plain", imgs, True)
    res = {"file_bytes": int(sum(len(f) for f in files))}

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB")

    with ThreadPoolExecutor(16) as pool:
        want = [np.asarray(a) for a in pool.map(one, files)]
    for key, kw in (("off", {}), ("on", {"scan_substreams": True})):
        jf = jpeg.JpegFiles(files, device=dev, progressive=True, **kw)
        views, status = jf.run()
        assert status.cpu().tolist() == [0] * len(files)
        res[f"{key}_equals_pillow"] = bool(all(np.array_equal(v.cpu().numpy(), w) for v, w in zip(views, want)))
        res[f"run_{key}"] = JB.timed(jf.run, n=1 if key == "off" else 3, groups=3)
        if key == "on":
            res["segment_bytes"] = jf.segment_bytes
            kinds = {name: {"scans": 0, "cut": 0, "accepted": 0, "max_rounds": 0, "ticks_sum": [0, 0, 0], "ticks_max_scan": [0, 0, 0]}
                     for name in ROUTES.values()}
            for p, info, ticks in zip(jf.parsed, jf.scan_substream_info(), jf.scan_substream_ticks()):
                for s, (route, nseg, rounds, acc), t in zip(p["scans"], info, ticks):
                    k = kinds[ROUTES[1 + (2 if s["ss"] else 0) + (1 if s["ah"] else 0)]]
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
    from attwarp_amd import _lib
    for bit, name in enumerate(("dc_first", "dc_refine", "ac_first", "ac_refine")):     # (JP_DC_FIRST .. JP_AC_REFINE)
        for field, mask in (("run_ms_only_this_kind_cut", 1 << bit), ("run_ms_all_but_this_kind_cut", 15 ^ (1 << bit))):
            with _lib.debug_override(jpegprog_sync_kinds=mask):
                jf = jpeg.JpegFiles(files, device=dev, progressive=True, scan_substreams=True)
                _, status = jf.run()
                assert status.cpu().tolist() == [0] * len(files)
                t = JB.timed(jf.run, n=1, groups=3)
                del jf
            torch.cuda.empty_cache()
            res["scan_kinds"][name][field] = PB.ms(t)
        k = res["scan_kinds"][name]
        k["ms_saved_alone_against_off"] = round(PB.ms(res["run_off"]) - k["run_ms_only_this_kind_cut"], 3)
        k["ms_saved_by_adding_it_last"] = round(k["run_ms_all_but_this_kind_cut"] - PB.ms(res["run_on"]), 3)
        k["pays"] = bool(k["ms_saved_by_adding_it_last"] > 0)
    jf = jpeg.JpegFiles(files, device=dev, progressive=True, scan_substreams="auto")
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    res["auto_kinds"], res["auto_equals_pillow"] = list(jpeg.AUTO_SCAN_KINDS), bool(all(np.array_equal(v.cpu().numpy(), w) for v, w in zip(views, want)))
    res["run_auto"] = JB.timed(jf.run, n=3, groups=3)
    del jf
    torch.cuda.empty_cache()
    with ThreadPoolExecutor(16) as pool:
        res["host_pillow_16_threads_plus_upload"] = JB.wall(lambda: pipeline.upload_images(list(pool.map(one, files)), dev))
    res["decode_jpeg_off"] = JB.wall(lambda: jpeg.decode_jpeg(files, device=dev, progressive=True))
    res["decode_jpeg_on"] = JB.wall(lambda: jpeg.decode_jpeg(files, device=dev, progressive=True, scan_substreams="auto"))
    res["ms"] = {k: PB.ms(res[k]) for k in ("run_off", "run_on", "run_auto", "decode_jpeg_off", "decode_jpeg_on", "host_pillow_16_threads_plus_upload")}
    res["run_off_over_on"] = res["ms"]["run_off"] / res["ms"]["run_on"]
    res["host_over_decode_jpeg_on"] = res["ms"]["host_pillow_16_threads_plus_upload"] / res["ms"]["decode_jpeg_on"]
    res["host_over_decode_jpeg_off"] = res["ms"]["host_pillow_16_threads_plus_upload"] / res["ms"]["decode_jpeg_off"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegprogsync_bench.json"))
    ap.add_argument("--cases", default=",".join(JB.CASES), help="comma-separated subset of " + ", ".join(JB.CASES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpegprogsync_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": 1,
           "files": "Pillow, quality 75, 4:2:0, progressive=True, no restart markers", "cases": []}
    for case in args.cases.split(","):
        B, sizes = JB.CASES[case]
        entry = {"case": case, "B": B, "sizes_HW": [list(s) for s in sizes], **measure(dev, JB.images(B, sizes))}
        print(json.dumps(entry), flush=True)
        res["cases"].append(entry)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                        # after every case: a partial file survives a time limit
            json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
