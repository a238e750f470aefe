"""The case tables of tests/test_axis_limits_gpu.py have the properties their names claim, and the host-side plan of numpy's
pairwise sum fits its tables at every row length the launchers accept.  No GPU needed."""
import numpy as np
import pytest

from oracle import warp_oracle as O
import axis_limit_cases as C

F32 = np.float32


def test_pairwise_plan_at_the_row_limit():
    """16384 elements split into 128 leaves of 128 and a program depth of 8; no row of <= 16384 elements needs a deeper
    stack than 10 (the finalize kernel's per-thread stack) -- and the leaf COUNT is not n / 128 rounded up: the right half
    of a split keeps the remainder, so 889 lengths between 15369 and 16383 make 129 leaves.  PairwisePlan's tables
    (PW_MAX_LEAVES in profiles_blocks.hpp) were 128 long and the 129th leaf was written past them."""
    leaves, depth = C.pairwise_plan(C.MAX_L)
    assert leaves == [(128 * i, 128) for i in range(128)] and depth == 8
    most, deepest, over = 0, 0, []
    for n in range(1, C.MAX_L + 1):
        lv, d = C.pairwise_plan(n)
        assert sum(m for _, m in lv) == n and all(1 <= m <= 128 for _, m in lv)
        assert [o for o, _ in lv] == list(np.cumsum([0] + [m for _, m in lv[:-1]]))
        most, deepest = max(most, len(lv)), max(deepest, d)
        if len(lv) > 128:
            over.append(n)
    assert most == 129 and deepest == 9 <= 10
    assert len(over) == 889 and over[0] == 15369 and over[-1] == 16383 and all(n % 8 for n in over)


def test_library_plans_every_accepted_width():
    """The library's own host plan (pw_build), seen through attwarp_axis_sums_workspace_bytes = 8 B (W + H leaves(W)):
    the restatement's leaf count at every width up to 16384 -- 129 of them included -- and 0 above it."""
    import os
    from attwarp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for W in range(1, C.MAX_L + 1):
        assert lib.attwarp_axis_sums_workspace_bytes(1, 1, W) == 8 * (W + len(C.pairwise_plan(W)[0])), W
    assert lib.attwarp_axis_sums_workspace_bytes(3, 7, 16383) == 3 * 8 * (16383 + 7 * 129)
    assert lib.attwarp_axis_sums_workspace_bytes(1, 1, C.MAX_L + 1) == 0


def test_attention_widths_cover_the_plan_shapes():
    """Which widths of the part-2 cases split into how many leaves: the limit (128 leaves of 128), the 129-leaf plans, a
    plan with leaves that are no multiple of 4 (the float32 fast kernel steps aside, the generic kernel runs), and plans of
    short rows (< 8: the uint8 fast kernel steps aside)."""
    want = {16384: (128, 128, 8), 16383: (129, 64, 9), 16381: (129, 64, 9), 8200: (65, 64, 8), 12296: (128, 96, 8),
            8: (1, 8, 1), 5: (1, 5, 1), 4: (1, 4, 1), 3: (1, 3, 1), 6: (1, 6, 1)}
    seen_odd_leaf = False
    for h, w in C.ATT_HW:
        for n in (h, w):
            lv, d = C.pairwise_plan(n)
            assert (len(lv), min(m for _, m in lv), d) == want[n], n
        seen_odd_leaf |= any(m % 4 for _, m in C.pairwise_plan(w)[0]) and w > 128
    assert seen_odd_leaf
    assert max(len(C.pairwise_plan(n)[0]) for hw in C.ATT_HW for n in hw) == 129
    assert any(w % 4 for _, w in C.ATT_HW) and any(w % 4 == 0 for _, w in C.ATT_HW)


@pytest.mark.parametrize("L", C.AXIS_LENGTHS)
def test_density_cases(L):
    p = C.densities(L)
    assert p.shape == (4, L) and p.dtype == F32
    seq = [C.takes_sequential_scan(r) for r in p]
    assert seq == [False, True, True, False], seq                 # rows as C.DENSITY_ROWS
    assert (p[3] == 0).all() and np.count_nonzero(p[2]) == 2 and 0 < p[2].min(initial=1, where=p[2] > 0) < 1.2e-38
    F = O.cdf_from_density(p)
    assert np.isfinite(F).all() and (np.diff(F, axis=1) >= 0)[:, :-1].all() and (F[:, -1] == 1).all()
    assert (F[3, :-1] == 0).all()


@pytest.mark.parametrize("N", C.AXIS_LENGTHS)
def test_cdf_cases(N):
    F = C.cdfs(N)
    assert F.shape == (4, N)
    assert (np.diff(F[0]) >= 0).all() and F[0, -1] == 1
    floor = F32(1e-4 / N)
    nd = np.maximum.accumulate(F[1])
    assert (np.diff(nd) < floor).all()                            # flat: every step is raised to the floor
    assert N < 16384 or abs(float(floor) - 6.1e-9) < 1e-10
    assert np.isnan(F[2]).sum() == 1 and np.isposinf(F[2]).sum() == 1 and np.isneginf(F[2]).sum() == 1
    assert (np.diff(F[3]) <= 0).all() and F[3, 0] == 1 and F[3, -1] == 0
    m = O.make_strictly_increasing(F)
    assert np.isfinite(m).all() and (m[:, -1] == 1).all() and (np.diff(m, axis=1) >= 0).all()
    # the flat row really sits on the floor: its repaired steps are N - 1 equal increments (to float32 rounding of the sum)
    steps = np.diff(m[1].astype(np.float64))
    assert np.abs(steps - steps.mean()).max() <= 2.0 ** -23


@pytest.mark.parametrize("NL", C.RESAMPLE_NL)
def test_resample_cases(NL):
    N, L = NL
    r = O.resample_cdf(C.cdfs(N), L)
    assert r.shape == (4, L) and np.isfinite(r).all() and (r[:, -1] == 1).all()
    assert N + L <= 2 * C.MAX_L


@pytest.mark.parametrize("L", C.AXIS_LENGTHS)
def test_map_cdf_cases(L):
    Ft, Fs = C.map_cdfs(L)
    assert (np.diff(Ft, axis=1) == 0).any(axis=1).all() and (np.diff(Ft, axis=1) >= 0)[:, :-1].all()
    assert (np.diff(Fs, axis=1) > 0).all() and (Fs[:, 0] > 0).all()
    for n_out in C.MAP_N_OUT:
        # the ramp is decided on the float64 knots F * n_out: taken for the ties, not for the strict rows
        for F, ties in ((Ft, True), (Fs, False)):
            for row in F:
                knots = np.concatenate(([0.0], row)) * float(n_out)
                knots[-1] = n_out
                assert bool(np.any(np.diff(knots) <= 0)) == ties
        mx, my = O.maps_from_cdf(Ft, Fs, (n_out, n_out))
        assert np.isfinite(mx).all() and np.isfinite(my).all()


@pytest.mark.parametrize("N", C.AXIS_LENGTHS)
def test_softmax_cases(N):
    x = C.logits(N)
    assert set(np.unique(x[0])) == {F32(-80), F32(80)}
    assert np.isnan(x[1]).sum() == 1 and np.isposinf(x[1]).sum() == 1 and np.isneginf(x[1]).sum() == 1
    assert (x[2] == x[2, 0]).all()
    s = O.safe_softmax(x)
    assert np.isfinite(s).all() and np.abs(s.astype(np.float64).sum(1) - 1).max() <= N * 2.0 ** -24
    assert (s[0][x[0] < 0] == 0).all()                            # exp(-160) underflows float32
    assert np.abs(s[2] - 1.0 / N).max() <= 2.0 ** -24 / N * 4


def test_attention_cases():
    for h, w in C.ATT_HW:
        assert max(h, w) in (16384, 16383, 16381, 8200, 12296) and min(h, w) <= 8
        for dt in ("uint8", "float32", "float64"):
            a = C.attention(h, w, dt)
            assert a.shape == (2, h, w) and a.dtype == np.dtype(dt)
        assert (C.attention(h, w, "float32") < 0).any()
        A = C.marginal_maps(h, w)
        assert np.isfinite(A[0]).all() and np.isnan(A[1]).sum() == 1 and np.isposinf(A[2]).sum() == 1
        with np.errstate(invalid="ignore"):
            px, py = O.gt_marginals(A)
        assert np.isfinite(px[0]).all() and np.isfinite(py[0]).all()
        assert not np.isfinite(px[1]).all() and not np.isfinite(px[2]).all()
    h, w = C.ATT_HW[0]
    for dt in ("uint8", "float32", "float64"):
        for tr in ("identity", "square"):
            mx, my = O.maps_from_attention(C.attention(h, w, dt)[0], 500, 400, tr)
            assert np.isfinite(mx).all() and np.isfinite(my).all()


def test_unaligned_view_recipe():
    """The GPU test takes a uint8 view one byte into its buffer (torch allocations are 256-byte aligned): the same recipe
    on the host gives an odd address, and a float32 view one element in gives a base that is 4- but not 16-byte aligned."""
    import torch
    buf = torch.zeros(1 + 2 * 5 * 16383, dtype=torch.uint8)
    view = buf[1:].view(2, 5, 16383)
    assert view.is_contiguous() and (view.data_ptr() - buf.data_ptr()) % 2 == 1
    fbuf = torch.zeros(1 + 2 * 3 * 16384, dtype=torch.float32)
    fview = fbuf[1:].view(2, 3, 16384)
    assert fview.is_contiguous() and (fview.data_ptr() - fbuf.data_ptr()) % 16 == 4


def test_fused_and_batch_cases():
    for Lo in (1, 64):
        px, py = C.low_res_pdfs(Lo)
        assert px.shape == (2, Lo) and np.abs(px.sum(1) - 1).max() < 1e-6
    px, py = C.low_res_pdfs(64)
    mx, my = C.pdf_chain(px, py, 8191, 8192, (3, 500))
    assert np.isfinite(mx).all() and np.isfinite(my).all()
    for g in (1, 2, C.AM_MAX_G, 64):
        s = C.step_maps(g)
        assert s.shape == (3, 2, g * g) and np.abs(s.sum(-1) - 1).max() < 1e-5
    assert C.AM_MAX_G ** 2 % 4 == 0 and C.AM_MAX_G ** 2 <= 768 and any(((g * g) % 4 or g * g > 768) for g in (27, 28))
    src = C.batch_sources()
    assert len(src) == C.MAX_B == 65535 and src[-1] == 5 and set(src[:-1]) == {0, 1, 2, 3, 4}
    six = C.six_maps()
    assert len({a.tobytes() for a in six}) == 6
    mx, my = C.steps_chain(C.six_step_maps(), 2, 8, 8)
    assert np.isfinite(mx).all() and len({r.tobytes() for r in mx}) == 6
