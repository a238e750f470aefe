"""Generate tests/golden/grounding_metrics.npz by IMPORTING THE REFERENCE's box metrics
(Ablations/attention_redistribution/metrics.py: BBOX_METHODS, interpret_bbox, top1, am_all).

    ATTWARP_REFERENCE=<checkout of the reference> python tests/golden/make_golden_grounding.py

Small float32 maps (random, peaked, constant = ties everywhere, negative lobes, one NaN, all zero) against raw boxes
(fractional, negative, out of range, zero size, valid only as xyxy), each box under both interpretations; the arrays hold
what the reference's functions return under the numpy this runs with (recorded in the file).
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def _load_metrics():
    ref = os.environ.get("ATTWARP_REFERENCE")
    if not ref:
        sys.exit("set ATTWARP_REFERENCE to a checkout of the reference")
    path = os.path.join(ref, "Ablations", "attention_redistribution", "metrics.py")
    spec = importlib.util.spec_from_file_location("ref_grounding_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def maps(H=37, W=53):
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:H, 0:W]
    out = {
        "random": rng.random((H, W), dtype=np.float32),
        "peaked": (np.exp(-((xx - 40.3) ** 2 + (yy - 8.7) ** 2) / 20.0) + 0.01 * rng.random((H, W))).astype(np.float32),
        "constant": np.full((H, W), 1.0 / 576, dtype=np.float32),
        "negative": (np.sin(xx / 4.0) * np.cos(yy / 5.0) * 3e-3).astype(np.float32),
        "nan": rng.random((H, W), dtype=np.float32),
        "zero": np.zeros((H, W), dtype=np.float32),
    }
    out["nan"][20, 11] = np.nan
    out["negative"][0, 0] = -0.0
    return out


RAW_BOXES = np.array([
    [10.0, 5.0, 20.0, 12.0],        # plain
    [10.7, 5.2, 20.9, 12.5],        # fractional (int() truncates)
    [-5.0, -3.0, 12.0, 9.0],        # negative start: numpy counts from the end
    [-20.0, 2.0, 8.0, 40.0],        # negative start, stop below it under xyxy
    [45.0, 30.0, 30.0, 30.0],       # runs past the map
    [70.0, 50.0, 5.0, 5.0],         # entirely outside
    [12.0, 7.0, 0.0, 6.0],          # zero width
    [12.0, 7.0, 5.0, 0.0],          # zero height
    [30.0, 4.0, 45.0, 12.0],        # xyxy: x2 > x1, y2 > y1
    [30.0, 20.0, 10.0, 15.0],       # valid only as xywh (xyxy gives negative sizes)
    [5.0, 5.0, 3.0, 30.0],          # xywh valid, xyxy negative width
    [38.0, 1.0, 52.0, 36.0],        # the peaked map's maximum inside
], dtype=np.float64)


def main():
    m = _load_metrics()
    mp = maps()
    names = list(mp)
    stack = np.stack([mp[n] for n in names])
    nb = len(RAW_BOXES)
    boxes = np.zeros((nb, len(m.BBOX_METHODS), 4), np.int64)
    top1 = np.zeros((len(names), nb, len(m.BBOX_METHODS)), np.int64)
    am = np.zeros((len(names), nb, len(m.BBOX_METHODS)), np.float32)
    argmax = np.zeros(len(names), np.int64)
    for j, raw in enumerate(RAW_BOXES):
        for k, meth in enumerate(m.BBOX_METHODS):
            boxes[j, k] = m.interpret_bbox(list(raw), meth)
    with np.errstate(invalid="ignore"):
        for i, n in enumerate(names):
            argmax[i] = int(np.argmax(mp[n]))
            for j in range(nb):
                for k in range(len(m.BBOX_METHODS)):
                    b = tuple(int(v) for v in boxes[j, k])
                    top1[i, j, k] = m.top1(mp[n], b)
                    am[i, j, k] = m.am_all(mp[n], b)
    np.savez_compressed(os.path.join(OUT, "grounding_metrics.npz"), maps=stack, names=np.array(names), raw_boxes=RAW_BOXES,
                        methods=np.array(m.BBOX_METHODS), boxes=boxes, top1=top1, am=am, argmax=argmax,
                        numpy_version=np.array(np.__version__))
    print("wrote grounding_metrics.npz:", stack.shape, "maps x", nb, "boxes; numpy", np.__version__)


if __name__ == "__main__":
    main()
