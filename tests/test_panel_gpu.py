"""GPU tests of the panel kernel (attwarp_panel_grid, attwarp_amd/panels.py): byte for byte against the restatement of
tests/panel_ref.py, always, heat rows included; against the stock expressions of MN/trainer.py:301-307 evaluated on the same
GPU, image / warp / uint8 rows byte for byte and heat rows within 1 grey level with at most 1e-4 of the heat bytes of a
test differing (torch-ROCm's bilinear kernel may contract the four-tap sum)."""
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import panel_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HEAT_MAX_SHARE = 1e-4
WIDTHS = [1, 2, 3, 5, 7, 16, 17, 63, 64, 65, 129, 257]     # every residue of 3 * Wg mod 4, both sides of a wave's and a workgroup's span


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rand(g, *shape):
    return torch.rand(*shape, device=DEV, generator=g)


def to_ref(row):
    from attwarp_amd import panels
    return R.Heat(row.A.cpu().numpy()) if isinstance(row, panels.Heat) else row.cpu().numpy()


def check(rows, n, H, W, **kw):
    """make_grid_u8 against the restatement, byte for byte -> the canvas as numpy."""
    from attwarp_amd import panels
    got = panels.make_grid_u8(rows, n=n, size=(H, W), **kw).cpu().numpy()
    want = R.make_grid_u8([to_ref(r) for r in rows], n, H, W, **kw)
    assert got.shape == want.shape, (got.shape, want.shape, kw)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{len(bad)} of {got.size} bytes differ from the restatement, first at {bad[0]}: "
                             f"{got[tuple(bad[0])]} against {want[tuple(bad[0])]} ({H}x{W}, n={n}, {kw})")
    return got


def mixed_rows(g, N, H, W, heat=(7, 5)):
    from attwarp_amd import panels
    return [rand(g, N, 3, H, W), panels.Heat(rand(g, N, 1, *heat)), (rand(g, N, 3, H, W) * 255).to(torch.uint8),
            rand(g, N, 1, H, W) * 1.5 - 0.25, (rand(g, N, 1, H, W) * 255).to(torch.uint8)]


@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_cell_sizes_against_the_restatement(layout):
    """Tiny cells and every width class, mixed source kinds (float32 and uint8, three channels and one, heat) in one call."""
    g = gen(1)
    for H, W in [(1, 1), (2, 3), (3, 2)] + [(3, w) for w in WIDTHS]:
        check(mixed_rows(g, 3, H, W), 3, H, W, layout=layout)


def test_geometry_against_the_restatement():
    """n 1..5, nrow below / at / above K, a last grid row that is not full, K = 1, padding 0..3, both pad values, right
    margins, both layouts."""
    g = gen(2)
    H, W = 5, 7
    x, y = rand(g, 5, 3, H, W), rand(g, 5, 1, H, W)
    for n in range(1, 6):
        for nrow in (1, 3, 2 * n, 2 * n + 3):
            check([x, y], n, H, W, nrow=nrow)                          # (n = 2, nrow = 3: K = 4, a last row of one cell)
    for n, margin in [(1, 0), (1, 1), (1, 400)]:                       # K = 1: the bare image, no padding
        for layout in ("hwc", "chw"):
            got = check([x], n, H, W, right_margin=margin, pad_value=255, layout=layout)
            assert got.shape == ((H, W + margin, 3) if layout == "hwc" else (3, H, W + margin))
    for padding in (0, 1, 2, 3):
        for pad_value in (0, 255):
            for margin in (0, 1, 400):
                for layout in ("hwc", "chw"):
                    check([x, y], 3, H, W, nrow=4, padding=padding, pad_value=pad_value, right_margin=margin, layout=layout)


def test_source_counts_kinds_and_clamp():
    from attwarp_amd import _lib, panels
    g = gen(3)
    H, W = 9, 13
    check([rand(g, 2, 3, H, W)], 2, H, W)
    check([panels.Heat(rand(g, 2, 1, 4, 6))], 2, H, W)                    # heat alone: size= names the cell
    rows = mixed_rows(g, 4, H, W) + [panels.Heat(rand(g, 4, 1, 24, 24)), rand(g, 4, 3, H, W) * 3 - 1, rand(g, 4, 1, H, W)]
    assert len(rows) == _lib.PANEL_MAX_SRC == panels.PANEL_MAX_SRC
    a = check(rows, 4, H, W)
    b = check(rows, 4, H, W, clamp=True)
    c = check(rows, 3, H, W, clamp=[False, False, False, True, False, False, True, False], layout="chw", nrow=5)
    assert np.array_equal(a, b) and c.shape[0] == 3                         # under the value policy the clamp changes no byte
    # out-of-range values and NaN / inf in float rows: the policy, on the device as in the restatement
    v = torch.tensor([-2.0, -1.0, -1 / 255, -0.0039, -0.0, 0.0, 1.0, 1.0039, 256 / 255, 2.0, float("nan"), float("inf"), -float("inf")],
                     device=DEV)
    row = v.repeat(3 * 13)[:3 * H * W].reshape(1, 3, H, W).contiguous()
    got = check([row], 1, H, W, layout="chw")
    assert got[0, 0, :13].tolist() == [0, 0, 0, 0, 0, 0, 255, 255, 255, 255, 0, 255, 0]


def test_slice_of_a_larger_batch_is_read_where_it_lies():
    from attwarp_amd import panels
    g = gen(4)
    H, W = 6, 10
    big, A = rand(g, 9, 3, H, W), rand(g, 9, 1, 5, 5)
    for view in (big[:4], big[3:7], big[1::2]):
        rec, _, _ = panels._source(view, False)
        assert rec["data"] == view.data_ptr() and rec["batch_stride"] == view.stride(0) and rec["N"] == 4
    assert big[3:7].data_ptr() == big.data_ptr() + 3 * 3 * H * W * 4
    check([big[3:7], panels.Heat(A[2:]), big[1::2], big], 3, H, W)        # N = 4, 7, 4, 9 > n = 3
    from attwarp_amd import panels as P
    got = P.make_grid_u8([big, P.Heat(A)], size=(H, W))                   # n defaults to the smallest N, nrow to n
    assert np.array_equal(got.cpu().numpy(), R.make_grid_u8([big.cpu().numpy(), R.Heat(A.cpu().numpy())], 9, H, W))


def test_output_buffer_at_every_byte_alignment():
    from attwarp_amd import panels
    g = gen(5)
    H, W = 4, 5
    rows = mixed_rows(g, 2, H, W)
    want = R.make_grid_u8([to_ref(r) for r in rows], 2, H, W, pad_value=9)
    for off in range(4):
        flat = torch.full((want.size + 8,), 77, dtype=torch.uint8, device=DEV)
        out = flat[off:off + want.size].view(want.shape)
        ret = panels.make_grid_u8(rows, n=2, pad_value=9, out=out)
        assert ret is out and out.data_ptr() % 4 == off
        assert np.array_equal(out.cpu().numpy(), want)
        assert (flat[:off] == 77).all() and (flat[off + want.size:] == 77).all()      # nothing written outside the canvas
    with pytest.raises(ValueError):
        panels.make_grid_u8(rows, n=2, out=torch.empty(3, 3, 3, dtype=torch.uint8, device=DEV))


def test_captured_graph_replays_on_changed_sources():
    from attwarp_amd import panels
    g = gen(6)
    H, W = 16, 17
    rows = mixed_rows(g, 3, H, W)
    out = panels.make_grid_u8(rows, n=3)                                   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        panels.make_grid_u8(rows, n=3, out=out)
    rows[0].copy_(rand(g, 3, 3, H, W))
    rows[1].A.copy_(rand(g, 3, 1, 7, 5) * 4)
    rows[2].fill_(200)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), R.make_grid_u8([to_ref(r) for r in rows], 3, H, W))


@pytest.mark.parametrize("hw", [(1, 1), (1, 24), (24, 1), (7, 5), (24, 24), (64, 64)])
def test_heat_maps_against_the_restatement(hw):
    """Up-sampled, down-sampled (H < h) and same-size heat; random, constant, all-zero and negative maps, one hot cell in
    each corner, NaN and +inf (policy: such an image is all zeros)."""
    from attwarp_amd import panels
    h, w = hw
    g = gen(7)
    A = rand(g, 11, 1, h, w)
    A[1] = 0.25
    A[2] = 0.0
    A[3] = -A[3] - 0.5
    for i, (y, x) in enumerate([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]):
        A[4 + i] = 0.0
        A[4 + i, 0, y, x] = 3.0
    A[8, 0, h // 2, w // 3] = float("nan")
    A[9, 0, h - 1, 0] = float("inf")
    A[10, 0, 0, w - 1] = -float("inf")
    for H, W in [(h, w), (3 * h + 1, 2 * w + 3), (max(1, h // 2), max(1, w // 3)), (37, 53)]:
        got = check([panels.Heat(A)], 11, H, W, layout="chw", padding=1)
        cells = [got[:, 1:1 + H, 1 + i * (W + 1): 1 + i * (W + 1) + W] for i in range(11)]
        assert (cells[2] == 0).all() and (cells[8] == 0).all() and (cells[9] == 0).all()
        assert (cells[1] == cells[1][0, 0, 0]).all() and cells[1][0, 0, 0] == 254


def stock_cells(img, A, warps, num_vis=4):
    """MN/trainer.py:301-307 up to the bytes, on whatever device the tensors live."""
    heat = A / (A.amax(dim=(2, 3), keepdim=True) + 1e-6)
    heat = heat.repeat(1, 3, 1, 1)
    heat = F.interpolate(heat, size=img.shape[-2:], mode="bilinear", align_corners=False)
    num_vis = min(num_vis, img.size(0))
    grid = torch.cat([img[:num_vis], heat[:num_vis]] + [w[:num_vis] for w in warps], dim=0)
    return (grid * 255).byte(), num_vis


def heat_condition(got, want, what):
    d = np.abs(got.astype(int) - want.astype(int))
    flips = int((d != 0).sum())
    print(f"[panel] {what}: {flips} of {d.size} heat bytes differ from torch on the GPU, max {int(d.max())}")
    assert d.max() <= 1, (what, int(d.max()))
    return flips, d.size


def test_heat_rows_against_stock_torch_on_the_gpu():
    from attwarp_amd import panels
    g = gen(8)
    flips = total = 0
    for (h, w), (H, W) in [((24, 24), (512, 512)), ((24, 24), (336, 336)), ((24, 24), (37, 53)), ((7, 5), (64, 65)), ((1, 1), (3, 3)),
                           ((24, 24), (12, 12)), ((5, 9), (1024, 17)), ((64, 64), (129, 63))]:
        A = rand(g, 4, 1, h, w)
        cells, n = stock_cells(torch.zeros(4, 3, H, W, device=DEV), A, [])
        want = cells[n:, 0].cpu().numpy()
        got = panels.make_grid_u8([panels.Heat(A)], n=4, size=(H, W), padding=0, layout="chw").cpu().numpy()[0]
        got = got.reshape(H, 4, W).transpose(1, 0, 2)
        f, t = heat_condition(got, want, f"{h}x{w} -> {H}x{W}")
        flips, total = flips + f, total + t
    print(f"[panel] heat rows: {flips} of {total} bytes differ from torch on the GPU ({flips / total:.2e})")
    assert flips <= HEAT_MAX_SHARE * total, (flips, total)


def test_the_trainers_case_512_five_rows():
    """B = 6, 512 x 512, n = 4, five rows (the validation panel) with its 400-pixel margin: against the restatement byte for
    byte, against the stock block on the same GPU byte for byte in the image / warp rows and under the condition in the heat row."""
    from attwarp_amd import panels
    g = gen(9)
    B, H, W = 6, 512, 512
    img, A = rand(g, B, 3, H, W), rand(g, B, 1, 24, 24)
    warps = [(rand(g, B, 3, H, W) * 1.2 - 0.1).clamp(0, 1) for _ in range(3)]
    grid, cells = panels.trainer_debug_grid(img, A, warps, num_vis=4, right_margin=400)
    rows = [img, R.Heat(A.cpu().numpy())] + warps
    want = R.make_grid_u8([r if isinstance(r, R.Heat) else r.cpu().numpy() for r in rows], 4, H, W, right_margin=400)
    got = grid.cpu().numpy()
    assert got.shape == want.shape == (5 * 514 + 2, 4 * 514 + 2 + 400, 3)
    assert np.array_equal(got, want)
    stock, n = stock_cells(img, A, warps)
    placed = R.place(stock.cpu().numpy(), nrow=n, right_margin=400).transpose(1, 2, 0)
    for r in (0, 2, 3, 4):
        assert np.array_equal(got[r * 514:(r + 1) * 514], placed[r * 514:(r + 1) * 514]), r
    f, t = heat_condition(got[514:2 * 514], placed[514:2 * 514], "trainer case")
    assert f <= HEAT_MAX_SHARE * t
    for r in range(5):
        for i in range(4):
            c = cells[r][i]
            assert tuple(c.shape) == (H, W, 3) and c.untyped_storage().data_ptr() == grid.untyped_storage().data_ptr()
            assert c.data_ptr() == grid.data_ptr() + ((r * 514 + 2) * grid.shape[1] + i * 514 + 2) * 3
            assert np.array_equal(c.cpu().numpy(), got[r * 514 + 2:r * 514 + 2 + H, i * 514 + 2:i * 514 + 2 + W])


def test_every_refusal_raises_and_launches_nothing():
    from attwarp_amd import _lib, panels
    g = gen(10)
    H, W = 4, 6
    x = rand(g, 4, 3, H, W)

    def refused(rows, text, exc=_lib.AttWarpError, **kw):
        n = kw.pop("n", 4)
        shape = None
        if kw.get("nrow", 1) >= 1 and kw.get("padding", 2) >= 0 and kw.get("right_margin", 0) >= 0 and n >= 1:
            _, _, _, Hg, Wt = R.geometry(len(rows) * n, H, W, kw.get("nrow", n), kw.get("padding", 2), kw.get("right_margin", 0))
            shape = (Hg, Wt, 3)
        out = torch.full(shape, 123, dtype=torch.uint8, device=DEV) if shape else None
        with pytest.raises(exc, match=text):
            panels.make_grid_u8(rows, n=n, size=(H, W), out=out, **kw)
        torch.cuda.synchronize()
        assert out is None or bool((out == 123).all())

    refused([x] * 9, "ATTWARP_PANEL_MAX_SRC")
    refused([x, panels.Heat(rand(g, 4, 1, 64, 65))], "ATTWARP_PANEL_MAX_HEAT")
    refused([x, rand(g, 3, 3, H, W)], "fewer than n=4")
    refused([x], "zero size", n=0)
    refused([x], "nrow", nrow=0)
    refused([x], "negative", padding=-1)
    refused([x], "negative", right_margin=-1)
    refused([x], "not a byte", pad_value=256)
    refused([x], "ATTWARP_PNG_MAX_ROW_BYTES", right_margin=8192 - 34, for_png=True)      # Wg = 4 * 8 + 2
    refused([rand(g, 4, 3, 0, W)], "zero size", exc=ValueError)
    refused([x.half()], "float32", exc=TypeError)
    refused([x.cpu()], "no CPU fallback", exc=RuntimeError)
    refused([x[:, :, :, ::2]], "dense", exc=ValueError)
    with pytest.raises(ValueError):
        panels.make_grid_u8([x], layout="nhwc")


def decode(png):
    return np.asarray(Image.open(io.BytesIO(png)))


def test_write_trainer_debug_files(tmp_path):
    """Every file decodes with Pillow to the bytes of its cell or of the grid; the per-sample files are
    (W.clamp(0, 1) * 255).byte() of the warps passed in (values outside [0, 1] included)."""
    from attwarp_amd import panels
    g = gen(11)
    B, H, W = 5, 33, 47
    img, A = rand(g, B, 3, H, W), rand(g, B, 1, 24, 24)
    warps = [rand(g, B, 3, H, W) * 1.4 - 0.2, rand(g, 3, 3, H, W) * 1.4 - 0.2]            # the second holds just n samples
    grid_path = tmp_path / "dbg_000100.png"
    pairs = [(tmp_path / f"s{i}.png", tmp_path / f"s{i}_gt.png") for i in range(3)]
    paths = panels.write_trainer_debug(grid_path, pairs, img, A, warps, num_vis=3)
    assert paths == [grid_path] + [p for pair in pairs for p in pair]
    grid, cells = panels.trainer_debug_grid(img, A, warps, num_vis=3)
    assert np.array_equal(np.asarray(Image.open(grid_path)), grid.cpu().numpy())
    assert np.array_equal(grid.cpu().numpy(), R.make_grid_u8([img.cpu().numpy(), R.Heat(A.cpu().numpy())] + [w.cpu().numpy() for w in warps],
                                                             3, H, W))
    for i, (p, q) in enumerate(pairs):
        for path, w, cell in ((p, warps[0], cells[2][i]), (q, warps[1], cells[3][i])):
            want = (w[i].clamp(0, 1) * 255).byte().permute(1, 2, 0).cpu().numpy()
            assert np.array_equal(np.asarray(Image.open(path)), want)
            assert np.array_equal(cell.cpu().numpy(), want)
            assert cell.untyped_storage().data_ptr() == grid.untyped_storage().data_ptr()
    with pytest.raises(ValueError):
        panels.write_trainer_debug(grid_path, pairs[:2], img, A, warps, num_vis=3)
    with pytest.raises(ValueError):
        panels.write_trainer_debug(grid_path, pairs, img, A, warps[:1], num_vis=3)


def test_trainer_block_end_to_end_with_this_packages_warps():
    """trainer_debug_grid with warps of img[:n] from this package's warp_from_cdf_torch equals the stock block run on the
    whole batch, sliced: the image and warp rows byte for byte, the heat row under its condition."""
    from attwarp_amd import checkpoint_utils as cu, panels
    g = gen(12)
    B, H, W, n = 7, 48, 40, 4
    img, A = rand(g, B, 3, H, W), rand(g, B, 1, 24, 24) ** 3
    px, py = cu.gt_marginals(A)
    Fx = cu.cdf_from_density(cu.upsample_pdf_right_inverse(px, W).clamp_min(0))
    Fy = cu.cdf_from_density(cu.upsample_pdf_right_inverse(py, H).clamp_min(0))
    Fx2, Fy2 = cu.cdf_from_density(rand(g, B, W) + 0.1), cu.cdf_from_density(rand(g, B, H) + 0.1)
    whole = [cu.warp_from_cdf_torch(img, Fx, Fy).clamp(0, 1), cu.warp_from_cdf_torch(img, Fx2, Fy2).clamp(0, 1)]
    stock, nv = stock_cells(img, A, whole, num_vis=n)
    want = R.place(stock.cpu().numpy(), nrow=nv).transpose(1, 2, 0)
    sliced = [cu.warp_from_cdf_torch(img[:n], Fx[:n], Fy[:n]), cu.warp_from_cdf_torch(img[:n], Fx2[:n], Fy2[:n])]
    grid, _ = panels.trainer_debug_grid(img, A, sliced, num_vis=n)
    got = grid.cpu().numpy()
    assert got.shape == want.shape
    ph = H + 2
    for r in (0, 2, 3):
        assert np.array_equal(got[r * ph:(r + 1) * ph], want[r * ph:(r + 1) * ph]), r
    assert np.array_equal(got[4 * ph:], want[4 * ph:])
    f, t = heat_condition(got[ph:2 * ph], want[ph:2 * ph], "end to end")
    assert f <= max(1, HEAT_MAX_SHARE * t)
