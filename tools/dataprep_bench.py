"""Measure the trainer's data preparation (attwarp_amd.dataloader) on the GPU.

    python tools/dataprep_bench.py [--out profiles/dataprep_bench.json]

Cases: B = 128 and B = 32 of the TextVQA-like size mix of tests/test_gpu_parity.py -> 512 x 512, and B = 128 images of
1024 x 1024 -> 512 x 512 (cfg.image_size = 512, B = 128 are the trainer's defaults).  Per case, in one process:
  * prepare_images on a planned batch (tables and records prepared once; HIP events around the launches): the one-launch
    kernel, and the same batch forced down the two-launch route (tuning library, prep_variant = 1);
  * prepare_attention_maps for B maps of 24 x 24 and of 512 x 512 -> 512 x 512;
  * a plain streaming launch (csrc/calib.hip, tuning flavour) that reads the sources' bytes once and writes the float32
    batch's bytes once: the ruler; fractions of the 8 TB/s peak are on those algorithmic bytes for both;
  * the host path this replaces: Pillow's resize + the ToTensor arithmetic per image on 16 threads, torch.stack and the
    upload of the float batch (wall clock around a device synchronise).
None of these numbers is a pass mark.  Times: HIP events around n back-to-back calls after a warm-up, median of 5 groups."""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXTVQA_LIKE_WH = [(1024, 768), (683, 1024), (1024, 1024), (500, 375), (333, 500), (640, 427)]      # as tests/test_gpu_parity.py
HBM_PEAK = 8.0e12
S = 512


def timed(fn, n=10, groups=5, warm=3):
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


def rate(entry, nbytes):
    entry["algorithmic_bytes"] = int(nbytes)
    entry["bytes_per_s"] = nbytes / (entry["us_median"] * 1e-6)
    entry["fraction_of_8TBs_peak"] = entry["bytes_per_s"] / HBM_PEAK
    return entry


def case(dev, name, sizes_wh):
    from PIL import Image
    from attwarp_amd import _lib, dataloader as D
    B = len(sizes_wh)
    gen = torch.Generator(device=dev).manual_seed(B)
    images = [torch.randint(0, 256, (h, w, 3), device=dev, dtype=torch.uint8, generator=gen) for (w, h) in sizes_wh]
    res = {"case": name, "B": B, "target": [S, S]}
    P = D.PreparedImages(images, S)
    nbytes = P.algorithmic_bytes
    res["plan"] = {"fused_images": int(P.header.n_fused_images), "fused_items": int(P.header.n_fused_items),
                   "two_launch_images": int(P.header.n_split_images), "lds_bytes": int(P.header.lds_bytes),
                   "register_window_taps": int(P.header.ks),
                   "bands": sorted({(int(p["ny"]), int(p["rb"]), int(p["nr_cap"])) for p in P.plan})}
    res["images_one_launch"] = rate(timed(P.run), nbytes)
    with _lib.debug_override(prep_variant=1):
        P2 = D.PreparedImages(images, S)
        assert P2.header.n_fused_images == 0
        res["images_forced_two_launch"] = rate(timed(P2.run), nbytes)
        res["images_forced_two_launch"]["tmp_bytes"] = int(P2.header.tmp_bytes)
        same = bool(torch.equal(P2.run(), P.run()))
    res["two_launch_equals_one_launch"] = same
    del P2

    tl = _lib.load_tuning()
    read = sum(im.numel() for im in images) // 16 * 16
    src = torch.empty(read, device=dev, dtype=torch.uint8)
    st = _lib.stream_ptr(dev)

    def copy():
        rc = tl.attwarp_debug_stream_copy(ctypes.c_void_p(src.data_ptr()), read, ctypes.c_void_p(P.out.data_ptr()), P.out.numel() * 4, st)
        assert rc == 0
    res["stream_copy_same_bytes"] = rate(timed(copy), nbytes)
    res["one_launch_over_copy"] = res["images_one_launch"]["us_median"] / res["stream_copy_same_bytes"]["us_median"]
    del src

    for side in (24, 512):
        maps = [torch.rand(side, side, device=dev, generator=gen) * 3 for _ in range(B)]
        A = D.PreparedAttention(maps, S)
        res[f"attention_{side}x{side}"] = rate(timed(A.run), A.algorithmic_bytes)
        del A, maps

    host = [Image.fromarray(im.cpu().numpy()) for im in images]

    def one(img):
        a = np.asarray(img.resize((S, S), Image.BILINEAR))
        return torch.from_numpy(a).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    with ThreadPoolExecutor(16) as pool:
        def host_path():
            return torch.stack(list(pool.map(one, host))).to(dev)
        res["host_pillow_16_threads_plus_upload"] = wall(host_path)
        res["host_equals_gpu"] = bool(torch.equal(host_path(), P.run()))
    res["host_over_one_launch"] = res["host_pillow_16_threads_plus_upload"]["us_median"] / res["images_one_launch"]["us_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataprep_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dataprep_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "cases": []}
    for name, sizes in (("textvqa_mix_B128", [TEXTVQA_LIKE_WH[b % len(TEXTVQA_LIKE_WH)] for b in range(128)]),
                        ("textvqa_mix_B32", [TEXTVQA_LIKE_WH[b % len(TEXTVQA_LIKE_WH)] for b in range(32)]),
                        ("1024x1024_B128", [(1024, 1024)] * 128)):
        res["cases"].append(case(dev, name, sizes))
        print(json.dumps(res["cases"][-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
