"""Float64 restatement of the training path on plain torch-CPU ops: one function per operation of attwarp_amd.losses,
model.mix_with_uniform / entropy, pipeline.trainer_attention_targets and losses.pdf_l1_loss.

Each function is the formula of the package's own docstring and stock-op fallback (``_recon_stock``, ``_pdf_l1_stock``, the
``needs_grad`` branches, ``stock_transform`` of test_losses_gpu.py) with every internal cast kept in float64; gradients
come from CPU autograd (``grads``).  tests/test_losses_ref_cpu.py pins every function to the stored values of
tests/golden/losses.npz, which is what lets the GPU sweep and the fuzzers use it as the expected value at shapes the
fixture does not hold.

The right inverse takes its (Lo, Lo) table as an argument: the GPU tests pass the one ``_tables.right_inverse_inv``
gives the kernels (for L < Lo the ridge system is ill-conditioned and two LAPACK routes need not agree), the CPU pin
passes ``right_inverse_table`` (the same system kept in float64, as the fixture's generator had it).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def t64(x, grad: bool = False) -> torch.Tensor:
    """numpy array / tensor (any float dtype) -> float64 CPU tensor, exactly (float32 -> float64 is exact)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return torch.from_numpy(np.array(x, dtype=np.float64)).requires_grad_(grad)


def grads(value: torch.Tensor, inputs, upstream: float = 1.0):
    """d (upstream * value) / d inputs by CPU autograd, as float64 numpy arrays."""
    gs = torch.autograd.grad(value * upstream, list(inputs), allow_unused=True)
    return [np.zeros(tuple(x.shape)) if g is None else g.numpy().copy() for g, x in zip(gs, inputs)]


def _finite_pos(x: torch.Tensor) -> torch.Tensor:
    return torch.nan_to_num(x.clamp_min(0), nan=0.0, posinf=0.0, neginf=0.0)


def _last_one(Fp: torch.Tensor) -> torch.Tensor:
    return torch.cat([Fp[:, :-1], torch.ones_like(Fp[:, -1:])], dim=1)


def cdf_from_density(p: torch.Tensor) -> torch.Tensor:
    q = _finite_pos(p)
    return _last_one(torch.cumsum(q / q.sum(dim=1, keepdim=True).clamp_min(1e-6), dim=1))


def l1_cdf_loss(p_pred: torch.Tensor, p_gt: torch.Tensor) -> torch.Tensor:
    return (cdf_from_density(p_pred) - cdf_from_density(p_gt)).abs().mean()


def sym_kl(p: torch.Tensor, q: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    P = p.clamp_min(eps)
    P = P / P.sum(dim=1, keepdim=True)
    Q = q.clamp_min(eps)
    Q = Q / Q.sum(dim=1, keepdim=True)
    return 0.5 * ((P * (P.log() - Q.log())).sum(dim=1).mean() + (Q * (Q.log() - P.log())).sum(dim=1).mean())


def _recon_pair(px, py, A):
    if A.dim() == 3:
        A = A.unsqueeze(1)
    Apos = A.clamp_min(0)
    Apos = Apos / Apos.sum(dim=(2, 3), keepdim=True).clamp_min(1e-6)
    P = py[:, :, None] * px[:, None, :]
    P = P / P.sum(dim=(1, 2), keepdim=True).clamp_min(1e-6)
    return P.unsqueeze(1), Apos


def separable_recon_loss(px, py, A) -> torch.Tensor:
    P, Apos = _recon_pair(px, py, A)
    return ((P - Apos) ** 2).mean()


def recon_l1(px, py, A) -> torch.Tensor:
    P, Apos = _recon_pair(px, py, A)
    return (P - Apos).abs().mean()


def cdf_from_density_downsample(p: torch.Tensor, L: int) -> torch.Tensor:
    q = _finite_pos(p)
    q = q / q.sum(dim=1, keepdim=True).clamp_min(1e-6)
    Fp = torch.cumsum(F.adaptive_avg_pool1d(q.unsqueeze(1), int(L)).squeeze(1), dim=1)
    return _last_one(Fp / Fp[:, -1:].clamp_min(1e-6))


def build_axis_cdf_targets(A: torch.Tensor, L: int = 128):
    if A.dim() == 3:
        A = A.unsqueeze(1)
    Ac = _finite_pos(A)
    return cdf_from_density_downsample(Ac.sum(dim=2).squeeze(1), L), cdf_from_density_downsample(Ac.sum(dim=3).squeeze(1), L)


def mix_with_uniform(p: torch.Tensor, alpha: float) -> torch.Tensor:
    return p if alpha <= 0 else (1 - alpha) * p + alpha / p.size(1)


def entropy(p: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    q = p.clamp_min(eps)
    return -(q * q.log()).sum(dim=1).mean()


# ---- the right inverse of adaptive_avg_pool1d ------------------------------------------------------------------------
def pooling_matrix(Lo: int, L: int) -> torch.Tensor:
    """(Lo, L) float64: row k averages window [floor(k L / Lo), ceil((k+1) L / Lo)) of L inputs."""
    A = torch.zeros(Lo, L, dtype=F64)
    for k in range(Lo):
        s, e = (k * L) // Lo, ((k + 1) * L + Lo - 1) // Lo
        A[k, s:e] = 1.0 / max(e - s, 1)
    return A


def right_inverse_table(Lo: int, L: int, eps: float = 1e-8) -> torch.Tensor:
    """(A A^T + eps I)^-1 with everything in float64 (the package's device table rounds the Gram matrix to float32)."""
    A = pooling_matrix(Lo, L)
    G = A @ A.T
    if eps > 0:
        G = G + eps * torch.eye(Lo, dtype=F64)
    return torch.linalg.solve(G, torch.eye(Lo, dtype=F64))


def upsample_pdf_right_inverse(y: torch.Tensor, L: int, inv) -> torch.Tensor:
    """x_hat = A^T (inv y) for rows y (B, Lo); ``inv`` is the (Lo, Lo) table, tensor or array."""
    inv = inv if isinstance(inv, torch.Tensor) else torch.from_numpy(np.asarray(inv, dtype=np.float64))
    inv = inv.detach().cpu().to(F64)
    return (y @ inv.T) @ pooling_matrix(y.shape[1], int(L))


def image_pdf(p: torch.Tensor, L: int, inv) -> torch.Tensor:
    u = upsample_pdf_right_inverse(p, L, inv).clamp_min(0)
    return u / u.sum(dim=1, keepdim=True).clamp_min(1e-6)


def pdf_l1_loss(px_s, py_s, px_gt, py_gt, W: int, H: int, inv_x, inv_y) -> torch.Tensor:
    return ((image_pdf(px_s, W, inv_x) - image_pdf(px_gt, W, inv_x)).abs().mean()
            + (image_pdf(py_s, H, inv_y) - image_pdf(py_gt, H, inv_y)).abs().mean())


# ---- the trainer's attention targets -------------------------------------------------------------------------------
def gt_marginals(A: torch.Tensor):
    Ap = A.clamp_min(0)
    mx, my = Ap.sum(dim=2).squeeze(1), Ap.sum(dim=3).squeeze(1)
    return mx / mx.sum(dim=1, keepdim=True).clamp_min(1e-6), my / my.sum(dim=1, keepdim=True).clamp_min(1e-6)


def trainer_attention_targets(A_full: torch.Tensor, transforms, grid=(24, 24)):
    """Transform by sample ("sqrt": sqrt of the clamped map, anything else: the clamped map; a blend by a 0/1 mask, so a
    NaN or +inf cell becomes NaN) -> adaptive_avg_pool2d to ``grid`` -> sanitise -> marginals, "none" rows uniform."""
    m = torch.tensor([1.0 if t == "sqrt" else 0.0 for t in transforms], dtype=A_full.dtype).view(-1, 1, 1, 1)
    pos = A_full.clamp_min(0.0)
    A = F.adaptive_avg_pool2d(pos.sqrt() * m + pos * (1.0 - m), tuple(grid))
    A = torch.nan_to_num(A, nan=0.0, posinf=0.0, neginf=0.0).clamp_min(0)
    px, py = gt_marginals(A)
    none = torch.tensor([t == "none" for t in transforms])
    if bool(none.any()):
        px, py = px.clone(), py.clone()
        px[none] = 1.0 / max(1, px.size(1))
        py[none] = 1.0 / max(1, py.size(1))
    return A, px, py


def trainer_block(A_full, px_s, py_s, transforms, img_h: int, img_w: int, inv_x, inv_y):
    """-> (L_pdf, A, px_gt, py_gt): the targets feed ``pdf_l1_loss`` as constants of the prediction."""
    A, pxg, pyg = trainer_attention_targets(A_full, transforms)
    return pdf_l1_loss(px_s, py_s, pxg, pyg, img_w, img_h, inv_x, inv_y), A, pxg, pyg


# ---- the generator's sign margin -------------------------------------------------------------------------------------
MARGIN = 1e-6


def l1_margin_ok(a, b, scale: float = 1.0) -> bool:
    """No |a - b| within MARGIN * scale of zero; scale is the size of a uniform density of the compared values."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return bool(d.min() >= MARGIN * scale) if d.size else True


def redraw(draw, ok, tries: int = 500):
    """The first draw (of at most ``tries``, each the next of the same seeded generator) that ``ok`` accepts."""
    for _ in range(tries):
        case = draw()
        if ok(*case):
            return case
    raise RuntimeError("no case with the sign margin found")


def l1_cdf_margin_ok(p, q) -> bool:
    with torch.no_grad():
        a, b = cdf_from_density(t64(p)).numpy(), cdf_from_density(t64(q)).numpy()
    return l1_margin_ok(a[:, :-1], b[:, :-1])


def recon_margin_ok(px, py, A) -> bool:
    """Cells with A+ = 0 against P > 0 have a stable sign; every other compared cell keeps the margin."""
    with torch.no_grad():
        P, Ap = (x.numpy() for x in _recon_pair(t64(px), t64(py), t64(A)))
    live = np.isfinite(Ap) & (Ap > 0)
    if P.shape[-1] * P.shape[-2] == 1:
        # a 1 x 1 map: P = x / x and A+ / A+ are exactly 1 in any IEEE precision, an exact tie on both sides (sign 0), and
        # no draw can move it
        live &= ~((P == 1.0) & (Ap == 1.0))
    return l1_margin_ok(P[live], Ap[live], scale=1.0 / (P.shape[-1] * P.shape[-2]))


def pdf_l1_margin_ok(px_s, py_s, px_gt, py_gt, W: int, H: int, inv_x, inv_y) -> bool:
    """Neither an image-resolution difference nor a clamp input of an up-sampled row within the margin of zero (an exact 0
    on both sides is a tie in either precision; so is a row whose prediction equals its GT bit for bit, where both
    sides run the same arithmetic on the same numbers: every row of length 1, [1.0], is one)."""
    with torch.no_grad():
        for p, g, n, inv in ((px_s, px_gt, W, inv_x), (py_s, py_gt, H, inv_y)):
            p, g = t64(p), t64(g)
            a, b = image_pdf(p, n, inv).numpy(), image_pdf(g, n, inv).numpy()
            d = a - b
            live = ((d != 0) | (a != 0)) & ~(p == g).all(dim=1).numpy()[:, None]
            if not l1_margin_ok(d[live], 0, 1.0 / n):
                return False
            for y in (p, g):
                u = upsample_pdf_right_inverse(y, n, inv).numpy()
                if not l1_margin_ok(u[u != 0], 0, 1.0 / n):
                    return False
    return True


def pdf_l1_well_conditioned(px_s, py_s, px_gt, py_gt, W: int, H: int, inv_x, inv_y, rel: float = 1e-5) -> bool:
    """Whether a loss bound of ``rel`` is attainable for pdf_l1 from float32 up-sampled rows (the kernels keep the rows the
    inference path and the reference's float32 trainer have).  An output adds at most 3 or, for L < Lo, up to
    ceil(Lo / L) + 1 window terms tmp[k] / len in float32: a relative error of at most (n + 3) 2^-24 per entry (tmp, 1 / len,
    the product, n - 1 sums, the normaliser).  Both rows of an axis sum to 1, so the axis' sum |a - b| moves by at most
    4 (n + 3) 2^-24; the bound holds when that is below ``rel`` times the sum itself.  Rows closer than that (two nearly
    uniform rows on a two-pixel axis) make the loss a small difference of rounded numbers: random draws skip them."""
    with torch.no_grad():
        for p, g, L, inv in ((px_s, px_gt, W, inv_x), (py_s, py_gt, H, inv_y)):
            p, g = t64(p), t64(g)
            Lo = p.shape[1]
            n = 3 if L >= Lo else -(-Lo // L) + 1
            dist = (image_pdf(p, L, inv) - image_pdf(g, L, inv)).abs().sum(dim=1)
            live = ~(p == g).all(dim=1)
            if bool((dist[live] * rel < 4 * (n + 3) * 2.0 ** -24).any()):
                return False
    return True


# ---- input recipes (the fixture generator's: coarse grids that are exact in float32 and float64) ---------------------
def softmax_rows(rng, B, N, peak=3.0):
    """Rows of a softmax on the 2^-16 grid, every entry at least 2^-16."""
    z = rng.standard_normal((B, N)) * peak
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    return (np.maximum(np.round(p * 65536.0), 1.0) / 65536.0).astype(np.float32)


def unit_map(rng, shape):
    return (rng.integers(0, 256, shape) / 256.0).astype(np.float32)


def hostile_map(rng, B, H, W):
    """Attention maps with NaN, +-inf and negative cells at seeded places of sample 0, an all-zero sample 1, an inf
    column and a negative row in sample 2 (the generator's recipe, with places drawn so that any H, W >= 1 works)."""
    A = unit_map(rng, (B, 1, H, W))
    for v in (np.nan, np.inf, -np.inf):
        A[0, 0, int(rng.integers(0, H)), int(rng.integers(0, W))] = v
    h0, w0 = int(rng.integers(0, H)), int(rng.integers(0, W))
    blk = A[0, 0, h0:h0 + 3, w0:w0 + 5]
    blk[...] = -rng.random(blk.shape, dtype=np.float32)
    if B > 1:
        A[1] = 0.0
    if B > 2:
        A[2, 0, :, W // 2] = np.inf
        A[2, 0, H // 4, :] = -2.0
    return A
