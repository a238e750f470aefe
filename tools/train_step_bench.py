"""Time one MarginalNet trainer step (MN/trainer.py:173-257, the network part) on the GPU: the fused route (library GEMMs +
the HIP tail, forward and backward) against the stock route (``net(..., stock=True)``: every op a stock ATen op).

    python tools/train_step_bench.py [--out FILE] [--quick]

The real call shape: MarginalNet(1024, 4096, 256), fmap [B,1024,24,24], ttok [B,32,4096], H = W = 24; B = 128
(cfg.batch_size) and B = 32.  One step = zero_grad, forward under torch.autocast("cuda"), a loss linear in (px, py),
GradScaler backward, unscale_, clip_grad_norm_(1.0), scaler.step(AdamW), scaler.update().
Reported per step and route: microseconds (CUDA events around n back-to-back steps, median of 5) and GPU ops
(torch.profiler).  For the fused route also the tail's own kernels: mean time per step from the profiler trace and the
fraction of the 8 TB/s HBM peak on the bytes each must move (film forward: v and gamma_beta read, vx / vy written;
film backward: v read, dv written, gx / gy read, dgamma_beta written; the softmax pair: their rows)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12
TAIL = ("film_axis_means_kernel", "film_axis_means_backward_kernel", "safe_softmax_kernel",
        "safe_softmax_backward_kernel")


def timed(fn, n, reps=5):
    times = []
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / n)
    return statistics.median(times)


def trace(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(e.name, e.time_range.elapsed_us()) for e in prof.events()
            if e.device_type == torch.autograd.DeviceType.CUDA]


def make_step(net, B, dev, stock):
    from attwarp_amd import model  # noqa: F401  (the package must be importable before the first step)
    g = torch.Generator(device=dev).manual_seed(B)
    fmap = torch.randn(B, 1024, 24, 24, device=dev, generator=g)
    ttok = torch.randn(B, 32, 4096, device=dev, generator=g)
    tmask = (torch.rand(B, 32, 1, device=dev, generator=g) < 0.8).float()
    wx = torch.randn(B, 24, device=dev, generator=g)
    wy = torch.randn(B, 24, device=dev, generator=g)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-6, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda")

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda"):
            px, py = net(fmap, 24, 24, ttok, tmask, stock=stock)
            loss = (px * wx).sum() + (py * wy).sum()
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        scaler.step(opt)
        scaler.update()
    return step


def tail_bytes(B, Ch=256, H=24, W=24, vb=2, gbb=2):
    """Bytes each tail kernel must move at least, autocast dtypes (v, gamma_beta float16; grads float32)."""
    plane = B * Ch * H * W
    return {"film_axis_means_kernel": plane * vb + B * 2 * Ch * gbb + B * Ch * (H + W) * 4,
            "film_axis_means_backward_kernel": 2 * plane * vb + B * Ch * (H + W) * 4 + 2 * B * 2 * Ch * gbb,
            "safe_softmax_kernel": 2 * (B * W * 4 + B * H * 4),
            "safe_softmax_backward_kernel": 3 * (B * W * 4 + B * H * 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer steps (for a profiler run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from attwarp_amd import model
    n = 3 if args.quick else 20
    rows = []
    for B in (128, 32):
        torch.manual_seed(0)
        net = model.MarginalNet(1024, 4096, 256).to(dev).train()
        fused, stock = make_step(net, B, dev, False), make_step(net, B, dev, True)
        for _ in range(3):
            fused()
            stock()
        t_f, t_s = timed(fused, n), timed(stock, n)
        tr_f, tr_s = trace(fused), trace(stock)
        row = {"B": B, "fused_us": round(t_f, 1), "stock_us": round(t_s, 1), "speedup": round(t_s / t_f, 3),
               "fused_gpu_ops": len(tr_f), "stock_gpu_ops": len(tr_s), "tail": {}}
        nbytes = tail_bytes(B)
        for k in TAIL:
            ts = [us for name, us in tr_f if k + "<" in name or name.endswith(k) or k + "(" in name]
            if ts:
                us = sum(ts) / 2 if k.startswith("safe_softmax") else sum(ts)    # per call: two heads
                row["tail"][k] = {"launches": len(ts), "us": round(us, 1),
                                  "hbm_frac": round(nbytes[k] / (us * 1e-6) / PEAK, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del net, fused, stock
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"run": f"tools/train_step_bench.py ({n} steps)", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
