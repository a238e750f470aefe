"""float64 numpy restatements of the backwards of MarginalNet's training tail (reference MN/model.py:8-14, 80-88), for
tests/test_marginalnet_train_{cpu,gpu}.py.  Each follows torch autograd's rules for the reference formula step by step
(mean backward = expand then divide; amax backward = split evenly over tied maxima; nan_to_num backward = 0 at non-finite
inputs; clamp_min backward = pass where the input >= the bound)."""
import numpy as np


def film_axis_means_backward(v, gamma_beta, gx, gy):
    """w = gamma*v + beta; vx = w.mean(2); vy = w.mean(3) (model.py:80-88).  v [B,Ch,H,W], gamma_beta [B,2Ch],
    gx [B,Ch,W], gy [B,Ch,H] -> dv [B,Ch,H,W], dgamma_beta [B,2Ch], and the per-(b,c) sums of |v*gw| and |gw|
    (the magnitude the float64 sums of a float32 implementation are measured against)."""
    v, gb, gx, gy = (np.asarray(a, np.float64) for a in (v, gamma_beta, gx, gy))
    B, Ch, H, W = v.shape
    gamma = gb[:, :Ch]
    gw = gx[:, :, None, :] / H + gy[:, :, :, None] / W
    dv = gamma[:, :, None, None] * gw
    dgb = np.concatenate([(v * gw).sum((2, 3)), gw.sum((2, 3))], axis=1)
    mag = np.concatenate([np.abs(v * gw).sum((2, 3)), np.abs(gw).sum((2, 3))], axis=1)
    return dv, dgb, mag


def safe_softmax_backward(logits, g, eps=1e-6):
    """Rows of safe_softmax (model.py:8-14): logits, g [B,N] -> (dlogits [B,N], scale [B,1]) where ``scale`` is the
    row's magnitude of the terms a float32 evaluation rounds (for tolerances)."""
    x = np.asarray(logits, np.float64)
    g = np.asarray(g, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        z = np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
        mx = z.max(1, keepdims=True)
        zc = z - mx
        e = np.exp(zc - zc.max(1, keepdims=True))            # F.softmax's own max shift (no gradient)
        sm = e / e.sum(1, keepdims=True)
        fin = np.isfinite(sm)
        pv = np.where(fin, sm, 0.0)
        S2 = pv.sum(1, keepdims=True)
        d = np.maximum(S2, eps)
        # out = pv / d
        dpv = g / d
        dd = -(g * pv / (d * d)).sum(1, keepdims=True)
        dpv = dpv + np.where(S2 >= eps, dd, 0.0)              # clamp_min, then sum backward (broadcast)
        dpv = np.where(fin, dpv, 0.0)                         # nan_to_num(pv)
        c = (dpv * sm).sum(1, keepdims=True)
        dzc = sm * (dpv - c)                                  # softmax backward
        tie = z == mx
        dz = dzc - tie * dzc.sum(1, keepdims=True) / tie.sum(1, keepdims=True)    # z - amax(z)
        dl = np.where(np.isfinite(x), dz, 0.0)                # nan_to_num(logits)
    scale = (sm * (np.abs(dpv) + np.abs(c))).max(1, keepdims=True) + np.abs(g).max(1, keepdims=True) * 1e-30
    return dl, scale
