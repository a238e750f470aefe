"""GPU tests of the JPEG decoder at its limits (files of tests/jpegdec_limit_cases.py, each proved on the CPU by
test_jpegdec_limits_ref_cpu.py): narrow and extremely long images against Pillow; blocks of 432 raw bytes through the
entropy kernel's ring and through the sub-streams; restart markers and the EOI on the scan's thread and tile boundaries;
data that ends on a segment boundary, segments behind the data, the smallest plan and the cap on segments.  Pixels,
statuses, units, restart counts and (segments, rounds, accepted) are compared for equality; there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

import jpegdec_cases as C
import jpegdec_limit_cases as L
import jpegdec_ref as D
import jpegdec_sync_cases as SC
import jpegdec_sync_ref as R
from test_jpegdec_gpu import DEV, G, back_to_back, check_views
from test_jpegdec_sync_gpu import want_info

pytestmark = pytest.mark.gpu


def names(status):
    return [D.STATUS_NAMES[s] for s in status]


def guarded(jf):
    """jf's output and scratch buffers replaced by ones with 0xA5 guard bytes around them -> the two whole buffers."""
    out = torch.full((jf.out_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    scr = torch.full((jf.scratch.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    jf.buffer, jf.scratch = out[G:G + jf.out_bytes], scr[G:G + jf.scratch.numel()]
    return out, scr


def guards_intact(*buffers):
    return all(bool((t[:G] == 0xA5).all()) and bool((t[-G:] == 0xA5).all()) for t in buffers)


def check_ok_views(views, files, status, judged_by_pillow):
    ok = [(nf, v) for nf, v, s in zip(files, views, status) if s == 0]
    for pillow in (True, False):
        sel = [(nf, v) for nf, v in ok if (nf[0] in judged_by_pillow) == pillow]
        check_views([v for _, v in sel], [nf for nf, _ in sel], "RGB", pillow=pillow)


# ---- 1. geometry against Pillow ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["narrow", "extreme"])
@pytest.mark.parametrize("mode", ["RGB", "keep"])
def test_narrow_and_extremely_long_images_equal_pillow(mode, which):
    from attwarp_amd import jpeg
    files = L.narrow() if which == "narrow" else L.extreme()
    jf = jpeg.JpegFiles([f for _, f in files], mode, device=DEV)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    check_views(views, files, mode)
    back_to_back(views, jf.buffer)
    want = [D.decode(f)[2]["nunits"] for _, f in files]
    assert jf.units() == want and [r + 1 for r in jf.restarts()] == want
    assert jf.substream_info() == want_info(files, R.DEFAULT_SEGMENT_BYTES, R.DEFAULT_MAX_ROUNDS)
    if which == "extreme":
        assert max(want) == 4094 and sum(a for _, _, a in jf.substream_info()) == 3


# ---- 2. the longest blocks ---------------------------------------------------------------------------------------------------------
def long_batch():
    ordinary = [(n, C.good_file(n)) for n in ("noise_64x48_s1", "ri_wrap")]
    return ordinary[:1] + L.long_files() + L.long_cuts() + ordinary[1:], {n for n, _ in ordinary}


def test_long_blocks_through_the_ring():
    from attwarp_amd import jpeg
    files, ordinary = long_batch()
    want = [D.decode(f)[0] for _, f in files]
    assert sorted(want) == [D.OK] * 6 + [D.E_TRUNCATED] * 2
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, substreams=False)
    out, scr = guarded(jf)
    views, status = jf.run()
    got = status.cpu().tolist()
    assert names(got) == names(want) and guards_intact(out, scr)
    back_to_back(views, jf.buffer)
    check_ok_views(views, files, got, ordinary)
    assert jf.units() == [D.decode(f)[2]["nunits"] for _, f in files] and jf.substream_info() == [(0, 0, 0)] * len(files)


@pytest.mark.parametrize("S", [32, 64, 512])
def test_long_blocks_as_sub_streams(S):
    from attwarp_amd import jpeg
    files, ordinary = long_batch()
    info = want_info(files, S, 256)
    assert sum(a for _, _, a in info) >= 4 and sum(1 for n, _, a in info if n and not a) >= 1       # the restatement decides first
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, segment_bytes=S, max_rounds=256)
    assert jf.substreams() == [n for n, _, _ in info]
    out, scr = guarded(jf)
    views, status = jf.run()
    got = status.cpu().tolist()
    assert names(got) == names([D.decode(f)[0] for _, f in files]) and guards_intact(out, scr)
    assert jf.substream_info() == info
    check_ok_views(views, files, got, ordinary)


# ---- 3. the restart scan -----------------------------------------------------------------------------------------------------------
def test_restart_markers_on_thread_and_tile_boundaries():
    from attwarp_amd import jpeg
    files = L.restart_files() + L.restart_damaged()
    want = [D.decode(f)[0] for _, f in files]
    assert want == [D.OK] * 7 + [D.E_RESTART] * 7
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV)
    out, scr = guarded(jf)
    views, status = jf.run()
    got = status.cpu().tolist()
    assert names(got) == names(want) and guards_intact(out, scr)
    assert jf.units() == [D.geometry(D.parse(f))["nunits"] for _, f in files] and max(jf.units()) >= 1000
    assert jf.restarts() == [len(L.scan_offsets(D.parse(f)["stream"])[0]) for _, f in files]
    check_ok_views(views, files, got, set())


# ---- 4. sub-stream boundaries and the cap ---------------------------------------------------------------------------------------
def both_routes(files, S, max_rounds):
    """The batch with sub-streams and without: (segments, rounds, accepted) equal the restatement's, statuses the sequential
    restatement's, pixels each other -> the sub-stream run's views and statuses."""
    from attwarp_amd import jpeg
    info = want_info(files, S, max_rounds)
    runs = []
    for kw in (dict(segment_bytes=S, max_rounds=max_rounds), dict(substreams=False)):
        jf = jpeg.JpegFiles([f for _, f in files], device=DEV, **kw)
        out, scr = guarded(jf)
        views, status = jf.run()
        runs.append((views, status.cpu().tolist(), jf.substreams(), jf.substream_info()))
        assert guards_intact(out, scr)
    (va, sa, pa, ia), (vf, sf, pf, inf) = runs
    assert pa == [n for n, _, _ in info] and ia == info and pf == [0] * len(files) and inf == [(0, 0, 0)] * len(files)
    assert names(sa) == names(sf) == names([D.decode(f)[0] for _, f in files])
    for a, b, s in zip(va, vf, sa):
        assert s != 0 or torch.equal(a, b)
    return va, sa, info


def test_data_that_ends_at_a_segment_boundary_and_segments_behind_it():
    files = L.data_ends() + L.behind_end() + [(n, f) for n, f, S, _ in L.smallest_plans() if S == 32]
    views, status, info = both_routes(files, 32, SC.MAX_ROUNDS)
    assert status == [0] * len(files) and [a for _, _, a in info] == [1] * 7 + [0] and info[6][0] == 2 and info[7] == (0, 0, 0)
    check_views(views, files, "RGB")


def test_the_smallest_plan_at_512_bytes():
    files = [(n, f) for n, f, S, _ in L.smallest_plans() if S == 512]
    views, status, info = both_routes(files, 512, SC.MAX_ROUNDS)
    assert status == [0, 0] and [(n, a) for n, _, a in info] == [(2, 1), (0, 0)]
    check_views(views, files, "RGB")


@pytest.mark.parametrize("S", [64, 512])
def test_every_one_unit_good_file_at_the_untested_segment_sizes(S):
    from attwarp_amd import jpeg
    files = SC.all_one_unit_good()
    want = want_info(files, S)
    assert all(a == 1 for n, _, a in want if n) and sum(1 for n, _, _ in want if n) >= 9
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, segment_bytes=S, max_rounds=SC.MAX_ROUNDS)
    assert jf.substreams() == [n for n, _, _ in want]
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    assert jf.substream_info() == want
    back_to_back(views, jf.buffer)
    check_views(views, files, "RGB")


def test_the_cap_on_segments():
    """16384 segments of 32 bytes: every lane sums 64 segments.  One byte more and the image is decoded sequentially."""
    from attwarp_amd import jpeg
    files = L.cap_files()
    info = want_info(files, 32, 256)
    assert info[0][0] == L.CAP_SEGMENTS and info[0][2] == 1 and info[1] == (0, 0, 0)
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, segment_bytes=32, max_rounds=256)
    assert jf.substreams() == [L.CAP_SEGMENTS, 0]
    views, status = jf.run()
    assert status.cpu().tolist() == [0, 0] and jf.substream_info() == info
    want = C.pillow(files[0][1], "RGB")
    for v in views:
        assert np.array_equal(v.cpu().numpy(), want)
