"""Time the optimiser tail of a MarginalNet trainer step (MN/trainer.py:259-264) on the GPU, three routes alternating in
one process, on MarginalNet(1024, 4096, 256)'s parameter set (18 float32 tensors, N = 2,755,074) with seeded gradients:

    (a) scaler.unscale_(opt); clip_grad_norm_(params, 1.0); scaler.step(opt); scaler.update()   torch.optim.AdamW (foreach)
    (b) the same four lines with torch.optim.AdamW(fused=True)
    (c) scaler.step(opt); scaler.update()          attwarp_amd.optim.AdamW(max_grad_norm=1.0)   (csrc/optim.hip)

    python tools/optim_step_bench.py [--out FILE] [--tail-only] [--lib LIBRARY]

Per route: GPU ops per step (torch.profiler), microseconds per step of the tail alone (CUDA events around n back-to-back
steps; median, min and max over the repeats of the same route: the spread), and whether the step synchronises with the
host (torch.cuda.set_sync_debug_mode).  For (c) each kernel's time (profiler trace, mean over the traced steps) and its
share of the 8 TB/s HBM peak on the bytes it must move: 4N (norm: g read) and 28N (apply: p, g, m, v read; p, m, v written).
The scaler runs at scale 1 and the gradients' norm is below the clip, so unscale_ and clip_grad_norm_ (which always
multiply) leave the gradients as they are and every step of every route sees the same inputs.

Then the whole trainer step (tools/train_step_bench.py's, fused network route) at B = 128 and B = 32 under (a) and (c).
--lib times a library built with another chunk size (make EXTRA=-DATTWARP_ADAMW_CHUNK=8192 in a copy of csrc/)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12
HYPER = dict(lr=1e-6, weight_decay=1e-4)
ROUTES = ("a_stock_foreach", "b_stock_fused", "c_hip")


def make_tail(route, shapes, dev, seed=0):
    from attwarp_amd import optim
    gen = torch.Generator(device=dev).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-4          # total norm 0.17: below the clip
    scaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=1 << 30)
    scaler.scale(torch.zeros((), device=dev))
    if route == "c_hip":
        opt = optim.AdamW(params, **HYPER, max_grad_norm=1.0)

        def step():
            scaler.step(opt)
            scaler.update()
    else:
        opt = torch.optim.AdamW(params, **HYPER, fused=(route == "b_stock_fused"))

        def step():
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            scaler.step(opt)
            scaler.update()
    return step


def events_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def alternate(fns, n, reps):
    """fns: name -> step; the routes take turns, `reps` rounds of n steps each."""
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            times[k].append(events_us(fn, n))
    return {k: {"us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
            for k, v in times.items()}


def trace(fn, steps=1):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    return [(e.name, e.time_range.elapsed_us()) for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def syncs(fn):
    """True when a step makes a synchronising call (None when this build does not flag them)."""
    fn()
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones((), device="cuda").item()
            return None
        except RuntimeError:
            pass
        try:
            fn()
            return False
        except RuntimeError:
            return True
    finally:
        torch.cuda.set_sync_debug_mode(old)
        torch.cuda.synchronize()


def make_train_step(net, B, dev, route):
    from attwarp_amd import optim
    g = torch.Generator(device=dev).manual_seed(B)
    fmap = torch.randn(B, 1024, 24, 24, device=dev, generator=g)
    ttok = torch.randn(B, 32, 4096, device=dev, generator=g)
    tmask = (torch.rand(B, 32, 1, device=dev, generator=g) < 0.8).float()
    wx = torch.randn(B, 24, device=dev, generator=g)
    wy = torch.randn(B, 24, device=dev, generator=g)
    ours = route == "c_hip"
    opt = optim.AdamW(net.parameters(), **HYPER, max_grad_norm=1.0) if ours else torch.optim.AdamW(net.parameters(), **HYPER)
    scaler = torch.amp.GradScaler("cuda")

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda"):
            px, py = net(fmap, 24, 24, ttok, tmask)
            loss = (px * wx).sum() + (py * wy).sum()
        scaler.scale(loss).backward()
        if not ours:
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        scaler.step(opt)
        scaler.update()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tail-only", action="store_true")
    ap.add_argument("--lib", default=None, help="time this build of the library instead of the package's")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    from attwarp_amd import _lib, model
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in model.MarginalNet(1024, 4096, 256).parameters()]
    N = sum(torch.Size(s).numel() for s in shapes)
    tails = {r: make_tail(r, shapes, dev) for r in ROUTES}
    for fn in tails.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    result = {"run": f"tools/optim_step_bench.py ({args.reps} rounds of {args.steps} steps per route, alternating)",
              "library": os.path.relpath(_lib.LIB_PATH, ROOT), "tensors": len(shapes), "N": N, "tail": {}}
    timing = alternate(tails, args.steps, args.reps)
    for r in ROUTES:
        tr = trace(tails[r])
        result["tail"][r] = dict(timing[r], gpu_ops=len(tr), host_sync=syncs(tails[r]))
    tr = trace(tails["c_hip"], steps=20)
    kernels = {}
    for key, nbytes in (("adamw_norm_kernel", 4 * N), ("adamw_apply_kernel", 28 * N)):
        ts = [us for name, us in tr if key in name]
        us = sum(ts) / 20
        kernels[key] = {"launches_per_step": len(ts) / 20, "us": round(us, 2), "bytes": nbytes,
                        "hbm_frac": round(nbytes / (us * 1e-6) / PEAK, 3) if us else None}
    result["tail"]["c_hip"]["kernels"] = kernels
    result["tail"]["c_hip"]["other_gpu_ops"] = sorted({name for name, _ in trace(tails["c_hip"]) if "adamw_" not in name})
    print(json.dumps(result["tail"]), flush=True)

    if not args.tail_only:
        result["train_step"] = []
        for B in (128, 32):
            torch.manual_seed(0)
            nets = {r: model.MarginalNet(1024, 4096, 256).to(dev).train() for r in ("a_stock_foreach", "c_hip")}
            steps = {r: make_train_step(net, B, dev, r) for r, net in nets.items()}
            for fn in steps.values():
                for _ in range(3):
                    fn()
            row = {"B": B}
            row.update(alternate(steps, 20, 5))
            for r, fn in steps.items():
                row[r]["gpu_ops"] = len(trace(fn))
            result["train_step"].append(row)
            print(json.dumps(row), flush=True)
            del nets, steps
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
