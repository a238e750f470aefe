"""Measure the layer sweep (attwarp_amd.grounding) on the GPU.

    python tools/grounding_bench.py [--out profiles/grounding_bench.json] [--probe-layers 4]

Cases:
  * the fused sweep (grid_box_metrics: LANCZOS4 value of every full-resolution pixel computed on the fly + top1 / am) and
    the 18 x 27 resize, 9 layers x 2 types, at B = 32 and B = 256 of the TextVQA-like size mix (bench.py TEXTVQA_LIKE_WH,
    cycled) -- us per batch, map-pixels per second and the share of the VALU ceiling: 8 multiplies + 7 adds per pixel
    (float32, unpacked) at the FP32 vector rate of 157.3 TFLOPS / 2 = 78.6 T instructions-lanes/s;
  * materialise-then-measure on the same batch (resize_lanczos4 to full size, then the dense box_metrics);
  * the numpy restatement (tests/grounding_ref.py) on the host for two images, labelled as a restatement: OpenCV is absent
    here, so the reference's own cv2 path cannot be timed;
  * the probe: one bf16 prefill of a random-weight decoder of LLaMA-7B shape (hidden 4096, 32 heads, head_dim 128,
    intermediate 11008) truncated to --probe-layers layers, sequence 640: SDPA with LayerSweepProbe on every layer against
    eager attention with output_attentions=True, at B = 1 and B = 32 -- ms per prefill and peak memory.
Times: HIP events around n back-to-back calls after a warm-up, median of 5 groups (>= 20 calls per case)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TEXTVQA_LIKE_WH = [(1024, 768), (683, 1024), (1024, 1024), (500, 375), (333, 500), (640, 427)]      # as bench.py
VALU_LANES_PER_S = 157.3e12 / 2
OPS_PER_PIXEL = 15


def timed(fn, n=20, groups=5, warm=3):
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
    return float(np.median(per)), float(min(per)), float(max(per))


def sweep_case(dev, B, nL=9):
    from attwarp_amd import grounding as G
    rng = np.random.default_rng(B)
    sizes = [TEXTVQA_LIKE_WH[b % len(TEXTVQA_LIKE_WH)] for b in range(B)]
    rows = torch.from_numpy(rng.random((2, nL, B, 576), dtype=np.float32) ** 4).to(dev).bfloat16()
    boxes = [(W // 4, H // 4, W // 3, H // 3) for (W, H) in sizes]
    px = 2 * nL * sum(W * H for (W, H) in sizes)
    a = rows[0].float()
    grids = torch.stack([a, a / (rows[1].float() + 1e-8)], dim=1).reshape(-1, 24, 24).contiguous()
    msizes = sizes * (2 * nL)
    mboxes = boxes * (2 * nL)
    G.layer_sweep(rows[0], rows[1], sizes, boxes)                       # tables uploaded once per distinct size
    t_sweep = timed(lambda: G.layer_sweep(rows[0], rows[1], sizes, boxes))
    t_fused = timed(lambda: G.grid_box_metrics(grids, msizes, mboxes))
    t_small = timed(lambda: G.resize_lanczos4(grids, (18, 27)))
    t_mat = timed(lambda: G.box_metrics(G.resize_lanczos4(grids, msizes), mboxes), n=5 if B > 64 else 20)
    f = G.grid_box_metrics(grids, msizes, mboxes)
    d = G.box_metrics(G.resize_lanczos4(grids, msizes), mboxes)
    same = bool(torch.equal(f.argmax, d.argmax) and torch.equal(f.top1, d.top1) and torch.equal(f.am, d.am))
    ceil_us = px * OPS_PER_PIXEL / VALU_LANES_PER_S * 1e6
    return {"B": B, "layers": nL, "maps": 2 * nL * B, "map_pixels": px,
            "layer_sweep_us": t_sweep[0], "layer_sweep_us_min_max": t_sweep[1:],
            "fused_metrics_us": t_fused[0], "fused_metrics_us_min_max": t_fused[1:],
            "small_resize_us": t_small[0],
            "materialise_then_measure_us": t_mat[0], "materialise_then_measure_us_min_max": t_mat[1:],
            "materialised_bytes_written": 4 * px,
            "fused_map_pixels_per_s": px / (t_fused[0] * 1e-6),
            "valu_ceiling_us": ceil_us, "fused_share_of_valu_ceiling": ceil_us / t_fused[0],
            "fused_equals_materialised_bits": same}


def restatement_case(n_images=2, nL=9):
    import grounding_ref as R
    rng = np.random.default_rng(1)
    sizes = TEXTVQA_LIKE_WH[:n_images]
    rows = (rng.random((2, nL, n_images, 576), dtype=np.float32) ** 4).astype(np.float32)
    boxes = [(W // 4, H // 4, W // 3, H // 3) for (W, H) in sizes]
    t0 = time.perf_counter()
    R.layer_sweep(rows[0], rows[1], sizes, boxes)
    dt = time.perf_counter() - t0
    return {"what": "numpy restatement of the study's loop (tests/grounding_ref.py), host, NOT OpenCV (absent)",
            "images": n_images, "sizes_WxH": sizes, "layers": nL, "s_total": dt, "s_per_image": dt / n_images}


def probe_case(dev, layers, B):
    import transformers
    from attwarp_amd import grounding as G
    cfg = transformers.LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=layers, num_attention_heads=32,
                                   num_key_value_heads=32, head_dim=128, vocab_size=32000, max_position_embeddings=4096)
    torch.manual_seed(0)
    with torch.device(dev):
        model = transformers.LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    ids = torch.randint(0, 32000, (B, 640), device=dev)
    out = {"B": B, "decoder_layers": layers, "seq": 640}
    for mode in ("sdpa_probe", "eager_output_attentions"):
        model.config._attn_implementation = "sdpa" if mode == "sdpa_probe" else "eager"
        probe = None
        if mode == "sdpa_probe":
            probe = G.LayerSweepProbe(model, list(range(layers)))
            probe.set_image_token_starts([35] * B)

        def run():
            with torch.no_grad():
                if probe is not None:
                    model.model(input_ids=ids)
                else:
                    model.model(input_ids=ids, output_attentions=True)
        try:
            run()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            t = timed(run, n=3, groups=3, warm=1)
            out[mode] = {"ms": t[0] / 1e3, "ms_min_max": [t[1] / 1e3, t[2] / 1e3],
                         "peak_bytes_above_weights": int(torch.cuda.max_memory_allocated(dev) - base)}
        except torch.cuda.OutOfMemoryError as e:
            out[mode] = {"error": f"out of memory: {str(e)[:120]}"}
        finally:
            if probe is not None:
                probe.remove()
            torch.cuda.empty_cache()
    del model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grounding_bench.json"))
    ap.add_argument("--probe-layers", type=int, default=4)
    ap.add_argument("--skip-probe", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "grounding_bench needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "sweep": [], "probe": []}
    for B in (32, 256):
        res["sweep"].append(sweep_case(dev, B))
        print(json.dumps(res["sweep"][-1]), flush=True)
    res["host_restatement"] = restatement_case()
    print(json.dumps(res["host_restatement"]), flush=True)
    if not args.skip_probe:
        import transformers
        res["transformers"] = transformers.__version__
        for B in (1, 32):
            res["probe"].append(probe_case(dev, args.probe_layers, B))
            print(json.dumps(res["probe"][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
