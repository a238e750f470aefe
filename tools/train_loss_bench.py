"""Time the MarginalNet trainer's loss block (MN/trainer.py:173-257) on the GPU: the HIP entry points against the stock-op
sequence, forward plus backward, eager.

    python tools/train_loss_bench.py [--out FILE] [--quick]

Cases: B = 128 maps of 512 x 512 (the trainer's cfg.batch_size / cfg.image_size) and B = 32 maps of 336 x 336.
One step = the attention targets (transform + 24 x 24 pool + sanitise, GT marginals with the "none" override), the
prediction mixed with uniform, L_pdf at image resolution, L_ent and train_l1 (forward), and L_pdf's backward to the
low-resolution predictions (the network itself is not part of the block).
  * hip:   pipeline.trainer_attention_targets, model.mix_with_uniform / entropy, losses.pdf_l1_loss / recon_l1;
  * stock: the trainer's own sequence of ATen ops on the same GPU, with the right inverse as two float32 matmuls against
           a cached (A A^T + eps I)^-1 (the reference rebuilds it per call with 48 host syncs; that cost is left out).
Reported per step: microseconds (CUDA events around n back-to-back steps, median of 5) and GPU kernels (torch.profiler).
HBM fraction of trainer_attention_targets next to the plain attwarp_adaptive_avg_pool kernel on the same bytes
(B x H x W x 4 read once; fraction of 8 TB/s).  The maps cycle through a ring of >= 1 GiB (more than the 256 MiB
Infinity Cache holds)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12
TFMS = ("sqrt", "none", "identity", "sqrt")


def ring_of(B, S, dev, min_bytes):
    n = max(2, -(-min_bytes // (B * S * S * 4)))
    g = torch.Generator(device=dev).manual_seed(B + S)
    return [torch.rand(B, 1, S, S, device=dev, generator=g) for _ in range(n)]


def timed(fn, n, reps=5):
    times = []
    for _ in range(reps):
        fn(0)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / n)
    return statistics.median(times)


def kernel_count(fn):
    from torch.profiler import ProfilerActivity, profile
    fn(0)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(0)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def make_steps(B, S, dev, ring):
    from attwarp_amd import _tables, losses, model, pipeline
    tfms = [TFMS[i % len(TFMS)] for i in range(B)]
    g = torch.Generator(device=dev).manual_seed(7)
    logits_x = torch.randn(B, 24, device=dev, generator=g)
    logits_y = torch.randn(B, 24, device=dev, generator=g)
    alpha = 0.3

    def hip(i):
        A, pxg, pyg = pipeline.trainer_attention_targets(ring[i % len(ring)], tfms)
        px = torch.softmax(logits_x, 1).requires_grad_(True)
        py = torch.softmax(logits_y, 1).requires_grad_(True)
        px_s, py_s = model.mix_with_uniform(px, alpha), model.mix_with_uniform(py, alpha)
        L_pdf = losses.pdf_l1_loss(px_s, py_s, pxg, pyg, S, S)
        _ent = model.entropy(px_s) + model.entropy(py_s)
        _train_l1 = losses.recon_l1(px_s, py_s, A)
        L_pdf.backward()

    inv = _tables.right_inverse_inv(24, S, 1e-8, dev).float()
    i24 = torch.arange(24, device=dev)
    st, en = i24 * S // 24, ((i24 + 1) * S + 23) // 24
    cols = torch.arange(S, device=dev)
    Ap = ((cols[None] >= st[:, None]) & (cols[None] < en[:, None])).float() / (en - st)[:, None].float()
    none_mask = torch.tensor([t == "none" for t in tfms], device=dev)
    mask_sqrt = torch.tensor([1.0 if t == "sqrt" else 0.0 for t in tfms], device=dev).view(B, 1, 1, 1)

    def up(y):
        return (y @ inv) @ Ap                          # A^T (A A^T + eps I)^-1 y, rows

    def stock(i):
        A_full = ring[i % len(ring)]
        pos = A_full.clamp_min(0.0)
        A = F.adaptive_avg_pool2d(pos.sqrt() * mask_sqrt + pos * (1.0 - mask_sqrt), (24, 24))
        A = torch.nan_to_num(A, nan=0.0, posinf=0.0, neginf=0.0).clamp_min(0)
        px = torch.softmax(logits_x, 1).requires_grad_(True)
        py = torch.softmax(logits_y, 1).requires_grad_(True)
        px_s, py_s = (1 - alpha) * px + alpha / 24, (1 - alpha) * py + alpha / 24
        px_img, py_img = up(px_s).clamp_min(0), up(py_s).clamp_min(0)
        Apos = A.clamp_min(0)
        mx, my = Apos.sum(dim=2).squeeze(1), Apos.sum(dim=3).squeeze(1)
        pxg, pyg = mx / mx.sum(1, keepdim=True).clamp_min(1e-6), my / my.sum(1, keepdim=True).clamp_min(1e-6)
        pxg[none_mask] = 1.0 / 24
        pyg[none_mask] = 1.0 / 24
        pxg_img, pyg_img = up(pxg).clamp_min(0), up(pyg).clamp_min(0)
        n = [t / t.sum(1, keepdim=True).clamp_min(1e-6) for t in (px_img, py_img, pxg_img, pyg_img)]
        L_pdf = F.l1_loss(n[0], n[2]) + F.l1_loss(n[1], n[3])
        _ent = [-(q * q.log()).sum(1).mean() for q in (px_s.clamp_min(1e-8), py_s.clamp_min(1e-8))]
        An = Apos / Apos.sum(dim=(2, 3), keepdim=True).clamp_min(1e-6)
        P = torch.einsum("bh,bw->bhw", py_s, px_s)
        _train_l1 = F.l1_loss((P / P.sum(dim=(1, 2), keepdim=True).clamp_min(1e-6)).unsqueeze(1), An)
        L_pdf.backward()

    def targets(i):
        pipeline.trainer_attention_targets(ring[i % len(ring)], tfms)

    def plain_pool(i):
        pipeline.adaptive_avg_pool2d(ring[i % len(ring)], (24, 24), sanitize=True)

    return hip, stock, targets, plain_pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer steps (for a profiler run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 5 if args.quick else 40
    rows = []
    for B, S in ((128, 512), (32, 336)):
        ring = ring_of(B, S, dev, 1 << 30)
        hip, stock, targets, plain = make_steps(B, S, dev, ring)
        nbytes = B * S * S * 4
        t_hip, t_stock = timed(hip, n), timed(stock, n)
        t_tt, t_pool = timed(targets, n), timed(plain, n)
        row = {"B": B, "S": S, "hip_us": round(t_hip, 1), "stock_us": round(t_stock, 1),
               "speedup": round(t_stock / t_hip, 2), "hip_kernels": kernel_count(hip), "stock_kernels": kernel_count(stock),
               "targets_us": round(t_tt, 1), "targets_hbm_frac": round(nbytes / (t_tt * 1e-6) / PEAK, 3),
               "plain_pool_us": round(t_pool, 1), "plain_pool_hbm_frac": round(nbytes / (t_pool * 1e-6) / PEAK, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del ring
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
