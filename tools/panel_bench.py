"""Measure the trainer's debug / validation panel (attwarp_amd.panels) against the block it replaces.

    python tools/panel_bench.py [--out profiles/panel_bench.json]

Batches: B = 128 x 512^2 (the trainer's) and B = 32 x 336^2, num_vis = 4, four rows (MN/trainer.py:283-325) and five rows
(:455-517).  Inputs of every variant: the float32 batch, the 24 x 24 attention and the image-resolution CDFs of each warp.
Per case, one process, every variant timed to FILES ON DISK (the grid and 2 x num_vis per-sample files) with the host clock
around a device synchronise:
  (a) the block as the trainer writes it, on this package without attwarp_amd.panels: whole-batch heat (stock torch),
      whole-batch warps through warp_from_cdf_torch, torch.cat, (grid * 255).byte(), make_grid assembled with stock indexing
      ops as torchvision's loop does, download of the raw pixels, Pillow ``save`` per file;
  (b) the same with [:n] slicing before anything is computed;
  (c) warps of img[:n] and panels.write_trainer_debug: one panel launch, one PngBatch, download of compressed bytes;
and on the device clock (HIP events, 50 back-to-back calls, median of 5 groups):
  the panel launch alone (the C entry point on prepared records; ``make_grid_u8_call`` is the Python call, host bound), and
  (d) a plain streaming launch (csrc/calib.hip, tuning flavour) that reads the panel's source bytes once and writes the
      canvas bytes: the ruler.
None of these numbers is a pass mark; the one condition DESIGN.md 3.13 states is that (c) is not slower than (b)."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


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
    return {"us_median": float(np.median(per)), "us_min": float(min(per)), "us_max": float(max(per)), "calls_per_group": n,
            "groups": groups, "timer": "HIP events"}


def wall(fn, n=5):
    fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e6)
    return {"us_median": float(np.median(per)), "us_min": float(min(per)), "us_max": float(max(per)), "calls": n,
            "timer": "host clock around a synchronise, to files on disk"}


def stock_make_grid(tensor, nrow, padding=2):
    """torchvision.utils.make_grid's loop on a uint8 [K,3,H,W] tensor, with stock indexing ops."""
    K = tensor.size(0)
    xmaps = min(nrow, K)
    ymaps = -(-K // xmaps)
    height, width = tensor.size(2) + padding, tensor.size(3) + padding
    grid = tensor.new_full((3, height * ymaps + padding, width * xmaps + padding), 0)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= K:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k += 1
    return grid


def trainer_block(img, A, cdfs, paths, sliced):
    """MN/trainer.py:289-325 (and :504-517 with a third warp) as written; ``sliced``: [:n] before anything is computed."""
    from PIL import Image
    from attwarp_amd import checkpoint_utils as cu
    num_vis = min(4, img.size(0))
    if sliced:
        img, A, cdfs = img[:num_vis], A[:num_vis], [(fx[:num_vis], fy[:num_vis]) for fx, fy in cdfs]
    warps = [cu.warp_from_cdf_torch(img, fx, fy).clamp(0, 1) for fx, fy in cdfs]
    heat = A / (A.amax(dim=(2, 3), keepdim=True) + 1e-6)
    heat = heat.repeat(1, 3, 1, 1)
    heat = F.interpolate(heat, size=img.shape[-2:], mode="bilinear", align_corners=False)
    grid = torch.cat([img[:num_vis], heat[:num_vis]] + [w[:num_vis] for w in warps], dim=0)
    grid = stock_make_grid((grid * 255).byte(), nrow=num_vis)
    Image.fromarray(grid.permute(1, 2, 0).cpu().numpy()).save(paths[0])
    for i in range(num_vis):
        for j in (0, 1):
            w_img = (warps[j][i].clamp(0, 1) * 255).byte().permute(1, 2, 0).cpu().numpy()
            Image.fromarray(w_img).save(paths[1 + 2 * i + j])


def panel_block(img, A, cdfs, paths):
    from attwarp_amd import checkpoint_utils as cu, panels
    n = min(4, img.size(0))
    warps = [cu.warp_from_cdf_torch(img[:n], fx[:n], fy[:n]) for fx, fy in cdfs]
    panels.write_trainer_debug(paths[0], [(paths[1 + 2 * i], paths[2 + 2 * i]) for i in range(n)], img, A, warps, num_vis=n)


def case(dev, gen, B, S, nwarps, tmp):
    from PIL import Image
    from attwarp_amd import _lib, checkpoint_utils as cu, panels
    n = 4
    yy = torch.linspace(0, 1, S, device=dev)
    img = (0.5 + 0.35 * torch.sin(12 * yy[None, None, :, None] + torch.arange(B, device=dev)[:, None, None, None])
           * torch.cos(9 * yy[None, None, None, :] + torch.arange(3, device=dev)[None, :, None, None])
           + 0.03 * torch.randn(B, 3, S, S, device=dev, generator=gen)).clamp(0, 1)
    A = torch.rand(B, 1, 24, 24, device=dev, generator=gen) ** 3
    cdfs = []
    for k in range(nwarps):
        Ak = torch.rand(B, 1, 24, 24, device=dev, generator=gen) ** 3 if k else A
        px, py = cu.gt_marginals(Ak)
        cdfs.append((cu.cdf_from_density(cu.upsample_pdf_right_inverse(px, S).clamp_min(0)),
                     cu.cdf_from_density(cu.upsample_pdf_right_inverse(py, S).clamp_min(0))))
    res = {"case": f"B{B}_{S}x{S}_{2 + nwarps}_rows", "B": B, "image": [3, S, S], "rows": 2 + nwarps, "num_vis": n}
    sets = {k: [os.path.join(tmp, f"{k}_{res['case']}_{i}.png") for i in range(1 + 2 * n)] for k in "abc"}
    res["a_trainer_block_whole_batch"] = wall(lambda: trainer_block(img, A, cdfs, sets["a"], False))
    res["b_trainer_block_sliced"] = wall(lambda: trainer_block(img, A, cdfs, sets["b"], True))
    res["c_write_trainer_debug"] = wall(lambda: panel_block(img, A, cdfs, sets["c"]))
    res["a_over_c"] = res["a_trainer_block_whole_batch"]["us_median"] / res["c_write_trainer_debug"]["us_median"]
    res["b_over_c"] = res["b_trainer_block_sliced"]["us_median"] / res["c_write_trainer_debug"]["us_median"]
    # the three routes write the same pixels (the heat row within one grey level of torch's)
    same, heat_off = True, 0
    for i in range(1 + 2 * n):
        pa, pb, pc = (np.asarray(Image.open(sets[k][i])).astype(int) for k in "abc")
        same &= bool(np.array_equal(pa, pb))
        if i == 0:
            d = np.abs(pa - pc)
            hrow = slice(S + 2, 2 * (S + 2))
            heat_off = int((d[hrow] != 0).sum())
            same &= bool(d[hrow].max() <= 1) and bool((d[:hrow.start] == 0).all()) and bool((d[hrow.stop:] == 0).all())
        else:
            same &= bool(np.array_equal(pa, pc))
    res["files_decode_to_the_same_pixels"] = same
    res["heat_bytes_one_level_off_torch"] = heat_off
    res["file_bytes"] = {k: int(sum(os.path.getsize(p) for p in sets[k])) for k in "abc"}

    # the panel launch alone against a plain streaming launch of its bytes
    warps = [cu.warp_from_cdf_torch(img[:n], fx[:n], fy[:n]) for fx, fy in cdfs]
    rows = [img[:n], panels.Heat(A[:n])] + warps
    out = panels.make_grid_u8(rows, n=n)
    read = (1 + nwarps) * n * 3 * S * S * 4 + n * 24 * 24 * 4
    write = out.numel()
    res["make_grid_u8_call"] = timed(lambda: panels.make_grid_u8(rows, n=n, out=out))      # bound by the host: Python builds the records
    recs = (_lib.PanelSource * len(rows))(*[_lib.PanelSource(**panels._source(r, False)[0]) for r in rows])
    lib, st = _lib.load(), _lib.stream_ptr(dev)

    def launch():
        rc = lib.attwarp_panel_grid(recs, len(rows), n, S, S, n, 2, 0, _lib.HWC, 0, 0, out.data_ptr(), st)
        assert rc == 0
    res["panel_launch"] = timed(launch, n=50)
    res["panel_launch"].update(source_bytes=read, canvas_bytes=write,
                               fraction_of_8TBs_peak=(read + write) / (res["panel_launch"]["us_median"] * 1e-6) / HBM_PEAK)
    tl = _lib.load_tuning()
    src = torch.empty(read // 16 * 16, device=dev, dtype=torch.uint8)
    dst = torch.empty(write // 16 * 16, device=dev, dtype=torch.uint8)

    def copy():
        rc = tl.attwarp_debug_stream_copy(ctypes.c_void_p(src.data_ptr()), src.numel(), ctypes.c_void_p(dst.data_ptr()), dst.numel(), st)
        assert rc == 0
    res["d_stream_copy_same_bytes"] = timed(copy, n=50)
    res["panel_over_copy"] = res["panel_launch"]["us_median"] / res["d_stream_copy_same_bytes"]["us_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "panel_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    gen = torch.Generator(device=dev).manual_seed(13)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        for B, S in ((128, 512), (32, 336)):
            for nwarps in (2, 3):
                res["cases"].append(case(dev, gen, B, S, nwarps, tmp))
                print(json.dumps(res["cases"][-1]), flush=True)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
