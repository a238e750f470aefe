"""CPU checks of the panel restatement (tests/panel_ref.py) against the stock torch-CPU expressions written as
MN/trainer.py:301-307 writes them (the make_grid step taken from the restatement's geometry: torchvision is not installed
where this project is built, tests/test_panel_vs_torchvision.py pins it on arrival), of the value policy, and of the
entry point's host-side refusals, which need no GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import panel_ref as R

# (h, w) -> (H, W): up-sampled, down-sampled, one cell, odd sizes, both aspect extremes, the LDS limit
HEAT_SHAPES = [((24, 24), (512, 512)), ((24, 24), (336, 336)), ((24, 24), (37, 53)), ((7, 5), (64, 65)), ((1, 1), (3, 3)),
               ((24, 24), (12, 12)), ((5, 9), (1024, 17)), ((64, 64), (129, 63))]
HEAT_MAX_SHARE = 1e-4          # of the heat bytes of the whole test, each at most 1 grey level off


def stock_cells(img, A, warps, num_vis=4):
    """MN/trainer.py:301-307 up to the bytes: uint8 [4 * n, 3, H, W] and n."""
    heat = A / (A.amax(dim=(2, 3), keepdim=True) + 1e-6)
    heat = heat.repeat(1, 3, 1, 1)
    heat = F.interpolate(heat, size=img.shape[-2:], mode="bilinear", align_corners=False)
    num_vis = min(num_vis, img.size(0))
    grid = torch.cat([img[:num_vis], heat[:num_vis]] + [w[:num_vis] for w in warps], dim=0)
    return (grid * 255).byte(), num_vis


def test_heat_rows_against_stock_torch_cpu():
    """Every heat byte within 1 grey level of torch's, at most 1e-4 of them different over all shapes: torch's CPU kernel
    contracts / orders the four-tap sum differently, which shows where v * 255 lies within an ulp of an integer."""
    g = torch.Generator().manual_seed(301)
    total = flips = 0
    for (h, w), (H, W) in HEAT_SHAPES:
        A = torch.rand(4, 1, h, w, generator=g)
        img = torch.zeros(4, 3, H, W)
        cells, n = stock_cells(img, A, [])
        want = cells[n:2 * n].numpy()
        assert (want[:, 0] == want[:, 1]).all() and (want[:, 0] == want[:, 2]).all()
        got = R.row_cells(R.Heat(A.numpy()), n, H, W)
        d = np.abs(got[:, 0].astype(int) - want[:, 0].astype(int))
        print(f"heat {h}x{w} -> {H}x{W}: {int((d != 0).sum())} of {d.size} bytes differ, max {int(d.max())}")
        assert d.max() <= 1, ((h, w), (H, W), int(d.max()))
        total, flips = total + d.size, flips + int((d != 0).sum())
    print(f"heat rows: {flips} of {total} bytes differ from torch-CPU ({flips / total:.2e})")
    assert flips <= HEAT_MAX_SHARE * total, (flips, total)


@pytest.mark.parametrize("H,W,B", [(17, 23, 6), (64, 65, 3), (1, 1, 5)])
def test_trainer_block_against_stock_torch_cpu(H, W, B):
    """The whole block: image, warp and uint8 rows bit for bit, the heat row under its condition, the grid placed by the
    restatement's geometry on both sides."""
    g = torch.Generator().manual_seed(H * 100 + W)
    img = torch.rand(B, 3, H, W, generator=g)
    A = torch.rand(B, 1, 24, 24, generator=g)
    Wimg = (torch.rand(B, 3, H, W, generator=g) * 1.2 - 0.1).clamp(0, 1)
    Wgt = (torch.rand(B, 3, H, W, generator=g) * 1.2 - 0.1).clamp(0, 1)
    cells, n = stock_cells(img, A, [Wimg, Wgt])
    want = R.place(cells.numpy(), nrow=n)
    got = R.make_grid_u8([img.numpy(), R.Heat(A.numpy()), Wimg.numpy(), Wgt.numpy()], n, H, W, layout="chw")
    assert got.shape == want.shape
    xm, ym, pad, Hg, Wt = R.geometry(4 * n, H, W, n)
    assert (xm, ym, pad) == (n, 4, 2) and got.shape == (3, Hg, Wt)
    rows = [slice(r * (H + pad), (r + 1) * (H + pad)) for r in range(4)]
    for r in (0, 2, 3):
        assert np.array_equal(got[:, rows[r]], want[:, rows[r]]), r
    d = np.abs(got[:, rows[1]].astype(int) - want[:, rows[1]].astype(int))
    assert d.max() <= 1 and (d != 0).sum() <= max(1, HEAT_MAX_SHARE * d.size)
    assert np.array_equal(got[:, Hg - pad:], want[:, Hg - pad:])
    # uint8 rows are copied; the HWC layout is the permuted CHW one; the per-sample files' bytes are two cells of the grid
    u8 = (img * 255).byte().numpy()
    assert np.array_equal(R.make_grid_u8([u8], n, H, W, layout="chw"), R.place(u8[:n], nrow=n))
    hwc = R.make_grid_u8([img.numpy(), R.Heat(A.numpy()), Wimg.numpy(), Wgt.numpy()], n, H, W, clamp=[False, False, True, True])
    assert np.array_equal(hwc, got.transpose(1, 2, 0))
    for i in range(n):
        w_img = (Wimg[i].clamp(0, 1) * 255).byte().permute(1, 2, 0).numpy()
        y, x = 2 * (H + pad) + pad, i * (W + pad) + pad
        assert np.array_equal(hwc[y:y + H, x:x + W], w_img)


def test_byte_values_where_torch_defines_them():
    """All 256 values k / 255 and their float32 neighbours, 0, 1, nextafter(1, 0), -0.0, values in (-1/255, 0): the byte
    is torch's (x * 255).byte(), with and without the clamp where the clamp changes nothing."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    v = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
                        np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), -0.0, -1e-3, -0.0039, 1.003], np.float32)])
    want = (torch.from_numpy(v) * 255).byte().numpy()
    assert np.array_equal(R.to_byte(v), want)
    assert np.array_equal(R.to_byte(v, clamp=True), (torch.from_numpy(v).clamp(0, 1) * 255).byte().numpy())
    assert np.array_equal(R.to_byte(v, clamp=True), want)
    assert R.to_byte(np.float32(1.0)) == 255 and R.to_byte(np.float32(-0.0)) == 0


def test_out_of_range_policy():
    """Outside -1 < t < 256 torch's cast is undefined: the policy saturates and sends NaN to 0."""
    inf = np.float32(np.inf)
    low = np.array([-1.0 / 255 * 1.01, -1.0, -1e30, -inf], np.float32)
    high = np.array([256.0 / 255, 1.1, 2.0, 1e30, inf], np.float32)
    assert (low * np.float32(255) <= -1).all() and (high[:1] * np.float32(255) >= 256).all()
    for clamp in (False, True):
        assert (R.to_byte(low, clamp) == 0).all()
        assert (R.to_byte(high, clamp) == 255).all()
        assert R.to_byte(np.float32(np.nan), clamp) == 0
    # a heat image whose maximum is NaN or +inf is all zeros; the other images of the row are not touched by it
    A = np.random.default_rng(5).random((3, 1, 6, 7), dtype=np.float32)
    A[0, 0, 2, 3] = np.nan
    A[1, 0, 0, 0] = inf
    cells = R.row_cells(R.Heat(A), 3, 20, 19)
    assert (cells[0] == 0).all() and (cells[1] == 0).all() and cells[2].max() > 200
    # constant, all-zero and one-hot maps
    assert (R.heat_bytes(np.full((5, 4), 0.25, np.float32), 9, 11) == int(np.float32(0.25) / (np.float32(0.25) + np.float32(1e-6)) * np.float32(255))).all()
    assert (R.heat_bytes(np.zeros((5, 4), np.float32), 9, 11) == 0).all()
    hot = np.zeros((4, 4), np.float32)
    hot[3, 0] = 2.0
    b = R.heat_bytes(hot, 16, 16)
    assert b[15, 0] == 254 and b[0, 15] == 0 and b.max() == 254          # 2 / (2 + 1e-6) * 255 = 254.99987


def test_geometry_is_make_grids():
    """make_grid's published geometry on a brute-force reading of its loop (torchvision/utils.py)."""
    for K, nrow, pad in [(1, 8, 2), (5, 8, 2), (8, 8, 2), (9, 8, 2), (20, 4, 2), (7, 3, 0), (7, 3, 1), (6, 1, 3), (20, 5, 2)]:
        H, W = 3, 5
        cells = np.random.default_rng(K).integers(0, 256, (K, 3, H, W), dtype=np.uint8)
        got = R.place(cells, nrow, pad, 255, right_margin=4)
        if K == 1:
            assert np.array_equal(got[:, :, :W], cells[0]) and (got[:, :, W:] == 255).all() and got.shape == (3, H, W + 4)
            continue
        xmaps = min(nrow, K)
        ymaps = int(np.ceil(float(K) / xmaps))
        height, width = H + pad, W + pad
        grid = np.full((3, height * ymaps + pad, width * xmaps + pad), 255, np.uint8)
        k = 0
        for y in range(ymaps):
            for x in range(xmaps):
                if k >= K:
                    break
                grid[:, y * height + pad: y * height + pad + height - pad, x * width + pad: x * width + pad + width - pad] = cells[k]
                k += 1
        assert np.array_equal(got[:, :, :-4], grid) and (got[:, :, -4:] == 255).all()


@pytest.fixture(scope="module")
def lib():
    import os
    from attwarp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entry_point_refusals_need_no_gpu(lib):
    """Every limit is refused on the host before anything is enqueued, with attwarp_last_error text."""
    from attwarp_amd import _lib
    fake = 0x1000                                     # never dereferenced: a refusal comes before any launch

    def src(kind=_lib.PANEL_F32, C=3, N=4, h=0, w=0, stride=None, data=fake):
        return _lib.PanelSource(data=data, batch_stride=C * 8 * 8 if stride is None else stride, kind=kind, C=C, N=N, h=h, w=w, clamp=0)

    def refused(sources, n=4, H=8, W=8, nrow=4, padding=2, pad_value=0, layout=_lib.HWC, margin=0, flags=0, out=fake, text=""):
        arr = (_lib.PanelSource * max(1, len(sources)))(*sources)
        rc = lib.attwarp_panel_grid(arr, len(sources), n, H, W, nrow, padding, pad_value, layout, margin, flags, out, None)
        msg = lib.attwarp_last_error().decode()
        assert rc < 0 and text in msg, (rc, msg)
        return rc

    heat = dict(kind=_lib.PANEL_HEAT, C=1, stride=4096)
    assert refused([], text="no source") == -1
    assert refused([src()] * (_lib.PANEL_MAX_SRC + 1), text="ATTWARP_PANEL_MAX_SRC") == -2
    assert refused([src(**heat, h=64, w=65)], text="ATTWARP_PANEL_MAX_HEAT") == -2
    assert refused([src(**heat, h=1, w=4097)], text="ATTWARP_PANEL_MAX_HEAT") == -2
    assert refused([src(**heat, h=0, w=5)], text="zero size") == -1
    assert refused([src()], n=0, text="zero size") == -1
    assert refused([src()], H=0, text="zero size") == -1
    assert refused([src()], W=0, text="zero size") == -1
    assert refused([src(), src(N=3)], text="fewer than n=4") == -1
    assert refused([src()], nrow=0, text="nrow") == -1
    assert refused([src()], padding=-1, text="negative") == -1
    assert refused([src()], margin=-1, text="negative") == -1
    assert refused([src()], pad_value=256, text="not a byte") == -1
    assert refused([src()], layout=2, text="layout") == -1
    assert refused([src()], flags=2, text="flags") == -1
    assert refused([src(C=2)], text="C=2") == -1
    assert refused([src(kind=3)], text="kind") == -1
    assert refused([src(stride=3 * 8 * 8 - 1)], text="batch stride") == -1
    assert refused([src(data=0)], text="null") == -1
    assert refused([src()], out=0, text="null") == -1
    assert refused([src(data=fake + 2)], text="aligned") == -1
    # PNG output requested: 1 + 3 * (Wg + margin) bytes must fit a row of the encoder
    assert refused([src(stride=3 * 8 * 2046)], W=2046, flags=_lib.PANEL_FOR_PNG, text="ATTWARP_PNG_MAX_ROW_BYTES") == -2   # Wg = 8194
    assert refused([src()], margin=8192 - 42, flags=_lib.PANEL_FOR_PNG, text="ATTWARP_PNG_MAX_ROW_BYTES") == -2            # Wg = 42
    assert _lib.PANEL_MAX_SRC == 8 and _lib.PANEL_MAX_HEAT == 4096 == R.MAX_HEAT and R.MAX_SRC == 8
    assert ctypes.sizeof(_lib.PanelSource) == 40


def test_python_surface_refuses_without_gpu():
    from attwarp_amd import panels
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(TypeError):
        panels.make_grid_u8([x.half()])
    with pytest.raises(TypeError):
        panels.make_grid_u8([x.double()])
    with pytest.raises(TypeError):
        panels.make_grid_u8([panels.Heat(torch.zeros(2, 1, 4, 4, dtype=torch.uint8))])
    with pytest.raises(ValueError):
        panels.make_grid_u8([x, torch.zeros(2, 3, 4, 5)])
    with pytest.raises(ValueError):
        panels.make_grid_u8([torch.zeros(2, 2, 4, 4)])
    with pytest.raises(ValueError):
        panels.make_grid_u8([torch.zeros(2, 3, 0, 4)])
    with pytest.raises(ValueError):
        panels.make_grid_u8([panels.Heat(torch.zeros(2, 1, 4, 4))])          # no cell size
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        panels.make_grid_u8([x])
