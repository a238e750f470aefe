#!/usr/bin/env python3
"""Generate tests/golden/losses.npz by IMPORTING THE REFERENCE's training losses.

Run in the build container only (the reference does not exist on the GPU box):
``python tests/golden/make_golden_losses.py``

Loads the reference's ``losses.py`` (with MN/ on sys.path, as losses.py:8 expects), ``model.py`` and
``checkpoint_utils.py`` and records, per case, the inputs (float32), the forward values and the CPU-autograd gradients computed in
float64 (loss scalars also from a float32 pass; arrays stored rounded to float32, see ``Cases.put``) of every function of MN/losses.py and of ``mix_with_uniform`` / ``entropy``
(MN/model.py:98-106), plus the trainer's loss block (MN/trainer.py:173-257) restated from the reference's own
functions with line citations (trainer.py itself needs LLaVA and a dataset; it does not import here).

float64: the reference casts with ``.float()`` inside cdf_from_density, build_axis_cdf_targets and
cdf_from_density_downsample; while the float64 values are computed that cast keeps float64 tensors in float64.

Margins: an L1 case in which an image-resolution difference (or a clamp input of the up-sampled prediction) lies
within 1e-6 of zero, in units of a uniform density of the compared values, is re-drawn, so that its signs are the same in float32 and float64.  The exact ties are cases of
their own (``tie_*``), built from values that are exact in both precisions.  Output is byte-identical between runs.

Only inputs and the reference's outputs are stored (data, never source).
"""
from __future__ import annotations

import contextlib
import inspect
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import MN, OUT, _install_stubs, _load  # noqa: E402

MARGIN = 1e-6


@contextlib.contextmanager
def keep_float64():
    """Tensor.float() leaves float64 tensors as they are (the reference's internal casts) inside the block."""
    orig = torch.Tensor.float

    def _float(self, *a, **k):
        return self if self.dtype == torch.float64 else orig(self, *a, **k)

    torch.Tensor.float = _float
    try:
        yield
    finally:
        torch.Tensor.float = orig


# Inputs are drawn on coarse grids (multiples of 2^-16 for PDFs, 1/256 for maps): exact in float32 and float64, and
# they compress, which keeps the fixture small.
def softmax_rows(rng, B, N, peak=3.0):
    z = rng.standard_normal((B, N)) * peak
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    return (np.maximum(np.round(p * 65536.0), 1.0) / 65536.0).astype(np.float32)


def unit_map(rng, shape):
    return (rng.integers(0, 256, shape) / 256.0).astype(np.float32)


def hostile_map(rng, B, H, W):
    """Attention maps with NaN, +-inf, negative cells and (sample 1) an all-zero map."""
    A = unit_map(rng, (B, 1, H, W))
    A[0, 0, 1, 2] = np.nan
    A[0, 0, H // 2, W // 3] = np.inf
    A[0, 0, H - 1, W - 1] = -np.inf
    A[0, 0, 3:6, 4:9] = -rng.random((3, 5), dtype=np.float32)
    if B > 1:
        A[1] = 0.0
    if B > 2:
        A[2, 0, :, W // 2] = np.inf
        A[2, 0, H // 4, :] = -2.0
    return A


class Cases:
    def __init__(self):
        self.arrays = {}
        self.names = {}

    def put(self, fn, case, **arrays):
        """Scalars are stored as computed, float64 and float32.  Arrays computed in float64 (targets, gradients) are
        stored rounded once to float32 -- at most 6e-8 relative, three orders of magnitude below the tests' bounds --
        and the float32 pass's arrays are left out: the fixture stays small."""
        self.names.setdefault(fn, []).append(case)
        for k, v in arrays.items():
            v = np.asarray(v)
            if v.size > 1 and k.endswith("_f32"):
                continue
            if v.size > 1 and v.dtype == np.float64:
                v = v.astype(np.float32)
            self.arrays[f"{fn}__{case}__{k}"] = np.ascontiguousarray(v)

    def write(self, path, meta):
        self.arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
        self.arrays["cases"] = np.array(json.dumps(self.names, sort_keys=True))
        with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
            for k in sorted(self.arrays):
                buf = io.BytesIO()
                np.lib.format.write_array(buf, self.arrays[k], allow_pickle=False)
                info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
                info.compress_type = zipfile.ZIP_DEFLATED
                z.writestr(info, buf.getvalue())


def run(fn, inputs, grad_of, **kw):
    """fn(*inputs64, **kw) in float64 with CPU autograd -> (values64 tuple, grads64 list); float32 values as well."""
    xs = [torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(i in grad_of) for i, x in enumerate(inputs)]
    with keep_float64():
        out = fn(*xs, **kw)
    outs = out if isinstance(out, tuple) else (out,)
    grads = []
    if grad_of:
        torch.autograd.backward(outs[0])
        grads = [xs[i].grad.numpy().copy() for i in grad_of]
    with torch.no_grad():
        o32 = fn(*[torch.from_numpy(np.asarray(x, dtype=np.float32)) for x in inputs], **kw)
    o32 = o32 if isinstance(o32, tuple) else (o32,)
    return [o.detach().numpy() for o in outs], grads, [o.numpy() for o in o32]


def l1_margin_ok(a, b, scale=1.0):
    """No |a - b| within MARGIN * scale of zero.  scale: the size of a uniform density of the compared values (1 for
    CDFs, 1/(H W) for the recon maps, 1/L for image-resolution PDFs), so the margin is 1e-6 in units of the data."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return bool(d.min() >= MARGIN * scale) if d.size else True


def redraw(draw, ok, tries=500):
    for _ in range(tries):
        case = draw()
        if ok(*case):
            return case
    raise RuntimeError("no case with the sign margin found")


def main():
    _install_stubs()
    torch.set_num_threads(1)
    sys.path.insert(0, MN)                                   # losses.py:8: from checkpoint_utils import cdf_from_density
    ckpt = _load("checkpoint_utils", os.path.join(MN, "checkpoint_utils.py"))
    losses = _load("ref_losses", os.path.join(MN, "losses.py"))
    model = _load("ref_model", os.path.join(MN, "model.py"))
    C = Cases()

    # ---- l1_cdf_loss (losses.py:11-12) ----
    def cdf64(p):
        with keep_float64():
            return ckpt.cdf_from_density(torch.from_numpy(p.astype(np.float64))).numpy()

    for seed, (B, N) in enumerate([(1, 24), (3, 37), (3, 1000), (128, 24)]):
        rng = np.random.default_rng(100 + seed)
        p, q = redraw(lambda: (softmax_rows(rng, B, N), softmax_rows(rng, B, N)),
                      lambda p, q: l1_margin_ok(cdf64(p)[:, :-1], cdf64(q)[:, :-1]))
        v, g, v32 = run(losses.l1_cdf_loss, [p, q], (0, 1))
        C.put("l1_cdf_loss", f"b{B}_n{N}", p_pred=p, p_gt=q, loss=v[0], loss_f32=v32[0], g_p_pred=g[0], g_p_gt=g[1])
    # hostile densities (NaN, +-inf, negatives, an all-zero row; their gradient is 0 where nan_to_num / clamp_min
    # block it) and the exact ties: row 0 prediction == GT, zeros exactly at the clamp bound 0
    rng = np.random.default_rng(150)
    p, q = softmax_rows(rng, 3, 37), softmax_rows(rng, 3, 37)
    p[1, 3], p[1, 7], p[1, 11], p[1, 12] = np.nan, np.inf, -np.inf, -0.25
    p[2] = 0.0
    v, g, v32 = run(losses.l1_cdf_loss, [p, q], (0, 1))
    C.put("l1_cdf_loss", "hostile_b3_n37", p_pred=p, p_gt=q, loss=v[0], loss_f32=v32[0], g_p_pred=g[0], g_p_gt=g[1])
    p, q = softmax_rows(rng, 3, 24), softmax_rows(rng, 3, 24)
    q[0] = p[0]
    p[1, ::5] = 0.0
    q[2, ::3] = 0.0
    v, g, v32 = run(losses.l1_cdf_loss, [p, q], (0, 1))
    C.put("l1_cdf_loss", "tie_b3_n24", p_pred=p, p_gt=q, loss=v[0], loss_f32=v32[0], g_p_pred=g[0], g_p_gt=g[1])

    # ---- sym_kl (losses.py:15-22) ----
    for seed, (B, N) in enumerate([(1, 24), (3, 256), (128, 24)]):
        rng = np.random.default_rng(200 + seed)
        p, q = softmax_rows(rng, B, N), softmax_rows(rng, B, N)
        v, g, v32 = run(losses.sym_kl, [p, q], (0, 1))
        C.put("sym_kl", f"b{B}_n{N}", p=p, q=q, eps=np.float64(1e-6), loss=v[0], loss_f32=v32[0], g_p=g[0], g_q=g[1])
    eps = 2.0 ** -20                                          # exact in float32 and float64: a tie at the clamp bound
    rng = np.random.default_rng(250)
    p, q = softmax_rows(rng, 3, 37), softmax_rows(rng, 3, 37)
    p[0, ::4] = eps
    q[1, ::3] = eps
    p[2, 1::5] = eps / 2
    v, g, v32 = run(losses.sym_kl, [p, q], (0, 1), eps=eps)
    C.put("sym_kl", "tie_b3_n37", p=p, q=q, eps=np.float64(eps), loss=v[0], loss_f32=v32[0], g_p=g[0], g_q=g[1])

    # ---- separable_recon_loss / recon_l1 (losses.py:25-47) ----
    def recon_diff(px, py, A):
        Ap = np.maximum(A[:, 0].astype(np.float64), 0)
        Ap = Ap / np.maximum(Ap.sum((1, 2), keepdims=True), 1e-6)
        P = py.astype(np.float64)[:, :, None] * px.astype(np.float64)[:, None, :]
        P = P / np.maximum(P.sum((1, 2), keepdims=True), 1e-6)
        return P, Ap

    for seed, (B, H, W, hostile) in enumerate([(1, 24, 24, False), (3, 37, 24, False), (128, 6, 6, False),
                                               (3, 24, 24, True), (3, 12, 256, False)]):
        rng = np.random.default_rng(300 + seed)
        def draw():
            px, py = softmax_rows(rng, B, W), softmax_rows(rng, B, H)
            A = unit_map(rng, (B, 1, H, W)) + np.float32(1 / 16)
            if hostile:
                A[0, 0, 3:9, 2:7] = -rng.random((6, 5), dtype=np.float32)
                A[1] = 0.0
                A[2] = -A[2]
            return px, py, A
        def ok(px, py, A):                                    # (cells with A+ = 0 against P > 0 have a stable sign)
            P, Ap = recon_diff(px, py, A)
            return l1_margin_ok(P[Ap > 0], Ap[Ap > 0], scale=1.0 / (H * W))
        px, py, A = redraw(draw, ok)
        case = f"{'hostile_' if hostile else ''}b{B}_h{H}_w{W}"
        for fn in ("separable_recon_loss", "recon_l1"):
            v, g, v32 = run(getattr(losses, fn), [px, py, A], (0, 1))
            C.put(fn, case, px=px, py=py, A=A, loss=v[0], loss_f32=v32[0], g_px=g[0], g_py=g[1])

    # ---- build_axis_cdf_targets (losses.py:50-67) ----
    for seed, (B, H, W, L, hostile) in enumerate([(1, 24, 24, 128, False), (3, 37, 128, 128, True),
                                                  (3, 16, 512, 24, True), (128, 6, 6, 24, False),
                                                  (3, 4, 1000, 512, False)]):
        rng = np.random.default_rng(400 + seed)
        A = hostile_map(rng, B, H, W) if hostile else unit_map(rng, (B, 1, H, W))
        v, _, v32 = run(losses.build_axis_cdf_targets, [A], (), L=L)
        C.put("build_axis_cdf_targets", f"{'hostile_' if hostile else ''}b{B}_h{H}_w{W}_L{L}", A=A, L=np.int64(L),
              Fx=v[0], Fy=v[1], Fx_f32=v32[0], Fy_f32=v32[1])

    # ---- cdf_from_density_downsample (losses.py:70-77) ----
    for seed, (B, N, L) in enumerate([(1, 24, 24), (3, 1000, 128), (128, 24, 37), (3, 512, 37), (3, 37, 256)]):
        rng = np.random.default_rng(500 + seed)
        p = softmax_rows(rng, B, N)
        if seed == 1:
            p[0, 5], p[0, 9], p[0, 10], p[1] = np.nan, np.inf, -3.0, 0.0
        v, _, v32 = run(losses.cdf_from_density_downsample, [p], (), L=L)
        C.put("cdf_from_density_downsample", f"b{B}_n{N}_L{L}", p=p, L=np.int64(L), F=v[0], F_f32=v32[0])

    # ---- mix_with_uniform (model.py:98-101): the gradient is that of sum(out * w) for a fixed weight w ----
    rng = np.random.default_rng(600)
    for i, alpha in enumerate([0.0, -1.0, 0.3, 1.0]):
        for B, N in ([(3, 24), (1, 37)] if alpha == 0.3 else [(3, 24)]):
            p = softmax_rows(rng, B, N)
            w = rng.standard_normal((B, N)).astype(np.float32)
            v, _, v32 = run(lambda x, alpha=alpha: model.mix_with_uniform(x, alpha), [p], ())
            x = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
            out = model.mix_with_uniform(x, alpha)
            (out * torch.from_numpy(w.astype(np.float64))).sum().backward()
            C.put("mix_with_uniform", f"a{i}_b{B}_n{N}", p=p, alpha=np.float64(alpha), w=w, out=v[0], out_f32=v32[0],
                  g_p=x.grad.numpy().copy())

    # ---- entropy (model.py:104-106) ----
    for seed, (B, N) in enumerate([(1, 24), (128, 24), (3, 512)]):
        rng = np.random.default_rng(700 + seed)
        p = softmax_rows(rng, B, N, peak=6.0)
        v, g, v32 = run(model.entropy, [p], (0,))
        C.put("entropy", f"b{B}_n{N}", p=p, eps=np.float64(1e-8), loss=v[0], loss_f32=v32[0], g_p=g[0])
    eps = 2.0 ** -27
    p = softmax_rows(np.random.default_rng(750), 3, 37)
    p[0, ::4], p[1, 1::3], p[2, 2::5] = eps, eps / 4, 0.0
    v, g, v32 = run(model.entropy, [p], (0,), eps=eps)
    C.put("entropy", "tie_b3_n37", p=p, eps=np.float64(eps), loss=v[0], loss_f32=v32[0], g_p=g[0])

    # ---- the trainer's loss block (MN/trainer.py:173-257) from the reference's own functions ----
    def trainer_block(A_full, px_s, py_s, tfms, img_h, img_w):
        B_att = A_full.size(0)
        # trainer.py:187-193: mask_sqrt from the per-sample transform names, transform on the full-resolution map
        mask_sqrt = torch.tensor([1.0 if t == "sqrt" else 0.0 for t in tfms], dtype=A_full.dtype).view(B_att, 1, 1, 1)
        A_full_pos = A_full.clamp_min(0.0)
        A_full_sqrt = A_full_pos.sqrt()
        A_full = A_full_sqrt * mask_sqrt + A_full_pos * (1.0 - mask_sqrt)
        # :197 pool to low-res after transform; :202 sanitize
        A = F.adaptive_avg_pool2d(A_full, (24, 24))
        A = torch.nan_to_num(A, nan=0.0, posinf=0.0, neginf=0.0).clamp_min(0)
        # :216-218 (px_s, py_s = mix_with_uniform(net(...), alpha), :213-214, are inputs here)
        px_img = ckpt.upsample_pdf_right_inverse(px_s, img_w).clamp_min(0)
        py_img = ckpt.upsample_pdf_right_inverse(py_s, img_h).clamp_min(0)
        # :220 and the "none" override :222-236
        px_gt_vis, py_gt_vis = ckpt.gt_marginals(A)
        none_mask = torch.tensor([t == "none" for t in tfms])
        if none_mask.any():
            px_gt_vis[none_mask] = 1.0 / max(1, px_gt_vis.size(1))
            py_gt_vis[none_mask] = 1.0 / max(1, py_gt_vis.size(1))
        # :238-239
        px_gt_img = ckpt.upsample_pdf_right_inverse(px_gt_vis, img_w).clamp_min(0)
        py_gt_img = ckpt.upsample_pdf_right_inverse(py_gt_vis, img_h).clamp_min(0)
        # :241-245 normalise, :247-248 L_pdf
        px_img = px_img / px_img.sum(dim=1, keepdim=True).clamp_min(1e-6)
        py_img = py_img / py_img.sum(dim=1, keepdim=True).clamp_min(1e-6)
        px_gt_img = px_gt_img / px_gt_img.sum(dim=1, keepdim=True).clamp_min(1e-6)
        py_gt_img = py_gt_img / py_gt_img.sum(dim=1, keepdim=True).clamp_min(1e-6)
        L_pdf = F.l1_loss(px_img, px_gt_img) + F.l1_loss(py_img, py_gt_img)
        return L_pdf, A, px_gt_vis, py_gt_vis, (px_img - px_gt_img), (py_img - py_gt_img), px_img, py_img

    for seed, (B, H, W, img_h, img_w, tfms, hostile) in enumerate([
            (1, 24, 24, 24, 24, ["sqrt"], False),
            (3, 50, 58, 336, 512, ["sqrt", "none", "identity"], True),
            (3, 48, 48, 37, 256, ["none", "sqrt", "other"], True),
            (8, 48, 24, 512, 512, None, False),
            (3, 48, 40, 1000, 37, ["identity", "sqrt", "sqrt"], False)]):
        rng = np.random.default_rng(800 + seed)
        if tfms is None:
            tfms = [("sqrt", "none", "identity", "x")[i % 4] for i in range(B)]
        A_full = hostile_map(rng, B, H, W) if hostile else unit_map(rng, (B, 1, H, W))
        def ok(px_s, py_s):
            # an exact 0 on both sides (clamped or all-zero rows) is a tie in either precision; anything else keeps a margin
            with torch.no_grad():
                t64 = [torch.from_numpy(x.astype(np.float64)) for x in (A_full, px_s, py_s)]
                out = [o.numpy() for o in trainer_block(*t64, tfms, img_h, img_w)]
                up = [ckpt.upsample_pdf_right_inverse(torch.from_numpy(np.asarray(x, np.float64)), n).numpy()
                      for x, n in ((px_s, img_w), (py_s, img_h), (out[2], img_w), (out[3], img_h))]
            for d, a, n in ((out[4], out[6], img_w), (out[5], out[7], img_h)):
                live = (d != 0) | (a != 0)
                if not l1_margin_ok(d[live], 0, 1.0 / n):
                    return False
            return all(l1_margin_ok(x[x != 0], 0, 1.0 / n) for x, n in zip(up, (img_w, img_h, img_w, img_h)))
        px_s, py_s = redraw(lambda: (softmax_rows(rng, B, 24, peak=1.0), softmax_rows(rng, B, 24, peak=1.0)), ok)
        v, g, v32 = run(lambda A, x, y: trainer_block(A, x, y, tfms, img_h, img_w)[:4], [A_full, px_s, py_s], (1, 2))
        C.put("trainer_block", f"{'hostile_' if hostile else ''}b{B}_h{H}_w{W}_img{img_h}x{img_w}",
              A_full=A_full, px_s=px_s, py_s=py_s, transforms=np.array(tfms), img_h=np.int64(img_h), img_w=np.int64(img_w),
              loss=v[0], A=v[1], px_gt=v[2], py_gt=v[3], loss_f32=v32[0], A_f32=v32[1], px_gt_f32=v32[2],
              py_gt_f32=v32[3], g_px_s=g[0], g_py_s=g[1])

    # ---- parameter names and defaults (inspect.signature of the reference) ----
    def sig(f):
        return [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in inspect.signature(f).parameters.items()]

    meta = {"signatures": {n: sig(getattr(losses, n)) for n in ("l1_cdf_loss", "sym_kl", "separable_recon_loss", "recon_l1",
                                                                 "build_axis_cdf_targets", "cdf_from_density_downsample")}}
    meta["signatures"].update({n: sig(getattr(model, n)) for n in ("mix_with_uniform", "entropy")})
    path = os.path.join(OUT, "losses.npz")
    C.write(path, meta)
    print("losses.npz", os.path.getsize(path) // 1024, "KiB,", sum(len(v) for v in C.names.values()), "cases")


if __name__ == "__main__":
    main()
