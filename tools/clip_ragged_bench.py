"""Measure the ragged CLIP preprocess (pipeline.ClipBatch, csrc/clip_ragged.hip) on the GPU.

    python tools/clip_ragged_bench.py [--out profiles/clip_ragged_bench.json]

Cases: B = 32 and B = 256 of the TextVQA-like size mix (as tools/dataprep_bench.py takes it) and B = 256 images of
500 x 500, all padded to a square and resized to 336 x 336 float16 (LLaVA-1.5's image_aspect_ratio == "pad").  Per case,
in one process, after a warm-up:
  * the batch call on a planned ClipBatch: HIP events around replays of its captured graph, and around eager calls;
    the same batch forced down the two-launch route (tuning library, clip_ragged_variant = 1);
  * the only GPU route the package had for such a batch before: a Python loop of clip_preprocess(img[None],
    pad_to_square=True) over the images, HIP events around eager passes (it allocates and uploads a constant per call, so
    it cannot be captured); the batch call must beat it -- the tool exits non-zero otherwise;
  * the host path this replaces: Pillow's paste + BICUBIC resize + the numpy normalisation per image on 16 threads,
    torch.stack, the float16 cast and the upload (wall clock around a device synchronise);
  * a plain streaming launch (csrc/calib.hip, tuning flavour) that reads the sources' bytes once and writes the batch's
    bytes once: the ruler; fractions of the 8 TB/s peak are on those algorithmic bytes.
Apart from the comparison with the loop none of these numbers is a pass mark.  One run; medians of 5 groups."""
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

TEXTVQA_LIKE_WH = [(1024, 768), (683, 1024), (1024, 1024), (500, 375), (333, 500), (640, 427)]      # as tools/dataprep_bench.py
HBM_PEAK = 8.0e12
S = 336


def timed(fn, n=10, groups=5, warm=3, what="HIP events around eager calls"):
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
            "groups": groups, "timer": what}


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
    from attwarp_amd import _lib, pipeline as P
    B = len(sizes_wh)
    gen = torch.Generator(device=dev).manual_seed(B)
    images = [torch.randint(0, 256, (h, w, 3), device=dev, dtype=torch.uint8, generator=gen) for (w, h) in sizes_wh]
    res = {"case": name, "B": B, "target": [S, S], "dtype": "float16", "pad_to_square": True}
    cb = P.ClipBatch(images, S, torch.float16)
    nbytes = cb.algorithmic_bytes
    h = cb.header
    res["plan"] = {"fused_images": int(h.n_fused_images), "fused_items": int(h.n_fused_items), "wide_items": int(h.n_wide_items),
                   "two_launch_images": int(h.n_split_images), "lds_bytes": int(h.lds_bytes), "register_window_taps": int(h.ks),
                   "bands": sorted({(int(p["window"]), int(p["ny"]), int(p["rb"]), int(p["nr_cap"])) for p in cb.plan})}
    graph, _ = P.capture_step(cb.run)
    res["batch_graph_replay"] = rate(timed(graph.replay, what="HIP events around graph replays"), nbytes)
    res["batch_eager"] = rate(timed(cb.run), nbytes)
    with _lib.debug_override(clip_ragged_variant=1):
        cb2 = P.ClipBatch(images, S, torch.float16)
        assert cb2.header.n_fused_images == 0
        res["batch_forced_two_launch"] = rate(timed(cb2.run), nbytes)
        res["batch_forced_two_launch"]["tmp_bytes"] = int(cb2.header.tmp_bytes)
        same = bool(torch.equal(cb2.run(), cb.run()))
    res["two_launch_equals_one_launch"] = same
    res["two_launch_over_one_launch"] = res["batch_forced_two_launch"]["us_median"] / res["batch_eager"]["us_median"]
    del cb2

    def loop():
        return [P.clip_preprocess(im[None], S, torch.float16, pad_to_square=True) for im in images]
    res["per_image_loop_existing_entry_point"] = rate(timed(loop, n=2, groups=5, warm=1), nbytes)
    res["loop_equals_batch"] = bool(torch.equal(torch.cat(loop()), cb.run()))
    res["loop_over_batch_eager"] = res["per_image_loop_existing_entry_point"]["us_median"] / res["batch_eager"]["us_median"]
    res["batch_faster_than_loop"] = res["loop_over_batch_eager"] > 1.0

    tl = _lib.load_tuning()
    read = sum(im.numel() for im in images) // 16 * 16
    src = torch.empty(read, device=dev, dtype=torch.uint8)
    st = _lib.stream_ptr(dev)

    def copy():
        rc = tl.attwarp_debug_stream_copy(ctypes.c_void_p(src.data_ptr()), read, ctypes.c_void_p(cb.out.data_ptr()),
                                          cb.out.numel() * 2, st)
        assert rc == 0
    res["stream_copy_same_bytes"] = rate(timed(copy), nbytes)
    res["step_over_copy"] = res["batch_graph_replay"]["us_median"] / res["stream_copy_same_bytes"]["us_median"]
    del src
    want = cb.run().clone()

    host = [Image.fromarray(im.cpu().numpy()) for im in images]
    mean = np.array(P.OPENAI_CLIP_MEAN, dtype=np.float32)
    std = np.array(P.OPENAI_CLIP_STD, dtype=np.float32)
    bg = tuple(int(m * 255) for m in P.OPENAI_CLIP_MEAN)

    def one(img):
        w, hh = img.size
        if w != hh:
            n = max(w, hh)
            canvas = Image.new("RGB", (n, n), bg)
            canvas.paste(img, ((n - w) // 2, 0) if hh > w else (0, (n - hh) // 2))
            img = canvas
        a = np.asarray(img.resize((S, S), Image.BICUBIC))
        x = (a.astype(np.float64) * (1 / 255)).astype(np.float32)
        return torch.from_numpy(np.ascontiguousarray(((x - mean) / std).transpose(2, 0, 1)))

    with ThreadPoolExecutor(16) as pool:
        def host_path():
            return torch.stack(list(pool.map(one, host))).to(torch.float16).to(dev)
        res["host_pillow_16_threads_plus_upload"] = wall(host_path)
        res["host_equals_gpu"] = bool(torch.equal(host_path(), want))
    res["host_over_batch_eager"] = res["host_pillow_16_threads_plus_upload"]["us_median"] / res["batch_eager"]["us_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_ragged_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "clip_ragged_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "runs": 1, "cases": []}
    for name, sizes in (("textvqa_mix_B32", [TEXTVQA_LIKE_WH[b % len(TEXTVQA_LIKE_WH)] for b in range(32)]),
                        ("textvqa_mix_B256", [TEXTVQA_LIKE_WH[b % len(TEXTVQA_LIKE_WH)] for b in range(256)]),
                        ("500x500_B256", [(500, 500)] * 256)):
        res["cases"].append(case(dev, name, sizes))
        print(json.dumps(res["cases"][-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)
    slower = [c["case"] for c in res["cases"] if not c["batch_faster_than_loop"]]
    if slower:
        sys.exit(f"the batch call is not faster than the per-image loop on: {slower}")


if __name__ == "__main__":
    main()
