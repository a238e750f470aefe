"""Measure the Stable-Diffusion warp ablation (attwarp_amd.sd_warp) on the GPU.

    python tools/sdwarp_bench.py [--out profiles/sdwarp_bench.json] [--steps 10]

Workload of the reduce: the cross-attention one SD-2.1 UNet forward at 768 x 768 leaves behind (16 layers: 5 each at 96^2,
48^2 and 24^2 with 5, 10 and 20 heads, one at 12^2 with 20 heads; B = 2, 77 tokens, float16, random softmax rows: ~125 MB),
--steps step keys of it resident in one HBM buffer.  In one process:
  * the one-pass reduce: attwarp_xattn_reduce on every tensor (token sums of all, hw_tok of the last layer of every step),
    kernels only (records prepared once), and reduce_captured_maps end to end (records, launch, the one host copy);
  * the same two reductions as the reference's torch expressions on the same GPU tensors: attn.sum(dim=(0,1,2,3)) of every
    tensor and attn[..., idx].sum(0).sum(0).sum(-1) of the last layer of every step -- on the device alone, and with the
    reference's .cpu() after every tensor;
  * a plain streaming launch of the same bytes (csrc/calib.hip, tuning flavour), the ruler for "each tensor crosses HBM
    once": fractions of the 8 TB/s peak are reported for both.
  * iterative_warp at B = 32 of the TextVQA-like size mix, 3 iterations, 24 x 24 maps, 500 x 500 output, against the loop a
    user of new_method would write (per image and pass: map to the image size on the device, then the numpy-facing
    new_method.warp_image_by_attention).
Times: HIP events around n back-to-back calls after a warm-up, median of 5 groups; wall clock where the host takes part."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXTVQA_LIKE_WH = [(1024, 768), (683, 1024), (1024, 1024), (500, 375), (333, 500), (640, 427)]      # as bench.py
HBM_PEAK = 8.0e12
LAYERS = [(96, 5)] * 2 + [(48, 10)] * 2 + [(24, 20)] * 2 + [(12, 20)] + [(24, 20)] * 3 + [(48, 10)] * 3 + [(96, 5)] * 3
B, TOKENS, TOP_K = 2, 77, 20


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


def reduce_case(dev, steps):
    from attwarp_amd import _lib, sd_warp
    numels = [B * heads * side * side * TOKENS for (side, heads) in LAYERS]
    span = [(n + 7) // 8 * 8 for n in numels]
    per_step = sum(span)
    buf = torch.empty(per_step * steps, device=dev, dtype=torch.float16)
    gen = torch.Generator(device=dev).manual_seed(0)
    cap = {}
    o = 0
    for s in range(steps):
        cap[1000 - 100 * s] = {}
        for k, ((side, heads), n, sp) in enumerate(zip(LAYERS, numels, span)):
            v = buf[o:o + n].view(B, heads, side, side, TOKENS)
            v.copy_(torch.softmax(torch.randn(B, heads, side, side, TOKENS, device=dev, generator=gen) * 2, dim=-1))
            cap[1000 - 100 * s][k] = v
            o += sp
    tensors = [t for d in cap.values() for t in d.values()]
    last = [k == len(LAYERS) - 1 for d in cap.values() for k in d]
    nbytes = sum(t.numel() for t in tensors) * 2
    res = {"steps": steps, "tensors": len(tensors), "bytes_read": nbytes, "dtype": "float16", "tokens": TOKENS,
           "row_bytes": TOKENS * 2}

    # kernels only: the records of sd_warp.xattn_reduce, prepared once
    M = len(tensors)
    rec = np.zeros(M, dtype=sd_warp._XATTN_DTYPE)
    sums = torch.empty(M, TOKENS, device=dev, dtype=torch.float16)
    hw = [torch.empty(t.shape[2] * t.shape[3], TOKENS, device=dev, dtype=torch.float16) if w else None for t, w in zip(tensors, last)]
    rec["attn"] = [t.data_ptr() for t in tensors]
    rec["token_sums"] = sums.data_ptr() + 2 * TOKENS * np.arange(M, dtype=np.int64)
    rec["hw_tok"] = [h.data_ptr() if h is not None else 0 for h in hw]
    rec["B"], rec["heads"] = B, [t.shape[1] for t in tensors]
    rec["HW"] = [t.shape[2] * t.shape[3] for t in tensors]
    rec_dev = torch.from_numpy(rec.view(np.uint8)).to(dev)
    lib = _lib.load()
    ws = torch.empty(lib.attwarp_xattn_reduce_workspace_bytes(rec.ctypes.data, M, TOKENS), device=dev, dtype=torch.uint8)
    st = _lib.stream_ptr(dev)

    def one_pass():
        _lib.call("attwarp_xattn_reduce", rec.ctypes.data, rec_dev.data_ptr(), M, _lib.F16, TOKENS, ws.data_ptr(), st)
    res["one_pass_kernels"] = timed(one_pass)
    res["one_pass_kernels"]["workspace_bytes"] = ws.numel()
    res["one_pass_end_to_end"] = wall(lambda: sd_warp.reduce_captured_maps(cap, keep_hw_tok=1))

    imp = sd_warp.compute_token_importance(sd_warp.reduce_captured_maps(cap, keep_hw_tok=0))
    idx = torch.as_tensor(np.ascontiguousarray(np.argsort(imp)[-TOP_K:][::-1]), device=dev)

    def torch_device():
        for t in tensors:
            t.sum(dim=(0, 1, 2, 3))
        for t, w in zip(tensors, last):
            if w:
                t[..., idx].sum(dim=0).sum(dim=0).sum(dim=-1)

    def torch_reference():
        for t in tensors:
            t.sum(dim=(0, 1, 2, 3)).cpu().numpy()
        for t, w in zip(tensors, last):
            if w:
                t[..., idx].sum(dim=0).sum(dim=0).sum(dim=-1).cpu().numpy().astype(np.float32)
    res["torch_expressions_device_only"] = timed(torch_device)
    res["torch_expressions_with_host_copies"] = wall(torch_reference)

    tl = _lib.load_tuning()
    dst = torch.empty(1 << 20, device=dev, dtype=torch.uint8)
    read = nbytes // 16 * 16

    def copy():
        rc = tl.attwarp_debug_stream_copy(ctypes.c_void_p(buf.data_ptr()), read, ctypes.c_void_p(dst.data_ptr()), dst.numel(), st)
        assert rc == 0
    res["stream_copy_same_bytes"] = timed(copy)
    for k in ("one_pass_kernels", "torch_expressions_device_only", "stream_copy_same_bytes"):
        res[k]["bytes_per_s"] = nbytes / (res[k]["us_median"] * 1e-6)
        res[k]["fraction_of_8TBs_peak"] = res[k]["bytes_per_s"] / HBM_PEAK
    res["one_pass_over_copy"] = res["one_pass_kernels"]["us_median"] / res["stream_copy_same_bytes"]["us_median"]
    res["torch_over_one_pass"] = res["torch_expressions_device_only"]["us_median"] / res["one_pass_kernels"]["us_median"]
    return res


def warp_case(dev, nB=32, iterations=3):
    from attwarp_amd import new_method, sd_warp
    rng = np.random.default_rng(0)
    sizes = [TEXTVQA_LIKE_WH[b % len(TEXTVQA_LIKE_WH)] for b in range(nB)]
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for (W, H) in sizes]
    maps = [rng.random((24, 24)).astype(np.float32) for _ in sizes]
    timg = [torch.from_numpy(i).to(dev) for i in images]
    tmap = [torch.from_numpy(m).to(dev) for m in maps]
    res = {"B": nB, "iterations": iterations, "out": [500, 500], "transform": "exp"}
    res["iterative_warp"] = timed(lambda: sd_warp.iterative_warp(timg, tmap, iterations, (500, 500), "exp", 1.0, 1.0, False), n=3)

    def loop():
        cur = images
        for _ in range(iterations):
            nxt = []
            for im, m in zip(cur, tmap):
                full = sd_warp.minmax_normalize(sd_warp.resize_cubic([m], [(im.shape[1], im.shape[0])]), in_place=True)[0]
                nxt.append(new_method.warp_image_by_attention(im, full.cpu().numpy(), 500, 500, "exp", 1.0 / iterations, 1.0, False))
            cur = nxt
        return cur
    res["loop_over_new_method_calls"] = wall(loop)
    res["loop_over_iterative_warp"] = res["loop_over_new_method_calls"]["us_median"] / res["iterative_warp"]["us_median"]
    got = sd_warp.iterative_warp(timg, tmap, iterations, (500, 500), "exp", 1.0, 1.0, False)[-1].cpu().numpy()
    res["same_bytes_as_the_loop"] = bool(all(np.array_equal(a, b) for a, b in zip(got, loop())))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdwarp_bench.json"))
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sdwarp_bench needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__}
    res["reduce"] = reduce_case(dev, args.steps)
    print(json.dumps(res["reduce"]), flush=True)
    torch.cuda.empty_cache()
    res["warp"] = warp_case(dev)
    print(json.dumps(res["warp"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
