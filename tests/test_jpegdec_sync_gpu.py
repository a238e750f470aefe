"""GPU tests of the JPEG decoder's sub-streams (jpegdec_substream_kernel, attwarp_amd/jpeg.py): marker-less files cut into
segments give the pixels of the restatement and of Pillow, the rounds and accepted flags of tests/jpegdec_sync_ref.py, and
the statuses of the sequential path; there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

import jpegdec_cases as C
import jpegdec_ref as D
import jpegdec_sync_cases as SC
import jpegdec_sync_ref as R
from test_jpegdec_gpu import DEV, G, back_to_back, check_views

pytestmark = pytest.mark.gpu


def want_info(files, S, max_rounds=SC.MAX_ROUNDS):
    out = []
    for _, f in files:
        accepted, rounds, _, nseg = R.decode_file(f, S, max_rounds)
        out.append((nseg, rounds, accepted))
    return out


@pytest.mark.parametrize("S", [32, 128])
@pytest.mark.parametrize("mode,order", [("RGB", "rgb"), ("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr")])
def test_every_one_unit_good_file_in_one_call(mode, order, S):
    from attwarp_amd import jpeg
    files = SC.all_one_unit_good()
    want = want_info(files, S)
    assert all(a == 1 for n, _, a in want if n) and sum(1 for n, _, _ in want if n) >= 9      # the restatement decides first
    jf = jpeg.JpegFiles([f for _, f in files], mode, order, device=DEV, segment_bytes=S, max_rounds=SC.MAX_ROUNDS)
    assert jf.substreams() == [n for n, _, _ in want]
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    assert jf.substream_info() == want
    back_to_back(views, jf.buffer)
    check_views(views, files, mode, order)


def test_more_segments_than_lanes():
    from attwarp_amd import jpeg
    files = [(SC.LARGE, SC.good_file(SC.LARGE))]
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, segment_bytes=32, max_rounds=SC.MAX_ROUNDS)
    nseg = jf.substreams()[0]
    assert nseg > 256 and nseg % 256 != 0
    views, status = jf.run()
    assert status.cpu().tolist() == [0] and jf.substream_info() == want_info(files, 32)
    assert jf.substream_info()[0][2] == 1
    assert np.array_equal(views[0].cpu().numpy(), C.pillow(files[0][1], "RGB"))


def test_a_file_that_misses_the_cap_falls_back_to_the_sequential_decode():
    from attwarp_amd import jpeg
    files = [(SC.SLOW, SC.good_file(SC.SLOW)), ("noise_8x8_s1", C.good_file("noise_8x8_s1"))]      # the second needs 3 rounds
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, segment_bytes=32, max_rounds=4)
    views, status = jf.run()
    info = jf.substream_info()
    assert info == want_info(files, 32, 4) and [i[2] for i in info] == [0, 1] and info[0][1] == 4
    assert status.cpu().tolist() == [0, 0]
    for (_, f), v in zip(files, views):
        assert np.array_equal(v.cpu().numpy(), C.pillow(f, "RGB"))


def edited(f, count, seed):
    """`count` files with one single-byte edit each at seeded positions of the entropy data, then the file with all of them.
    No edit touches or creates an FF, so none creates a marker."""
    segs, tail = C.split(f)
    r = np.random.RandomState(seed)
    every = bytearray(tail)
    out = []
    while len(out) < count:
        i = int(r.randint(1, len(tail) - 2))
        v = int(r.randint(0, 255))                           # never FF
        if tail[i] == 0xFF or tail[i - 1] == 0xFF or v == tail[i]:
            continue
        one = bytearray(tail)
        one[i] = every[i] = v
        out.append(C.join(segs, bytes(one)))
    return out + [C.join(segs, bytes(every))]


@pytest.fixture(scope="module")
def damaged():
    base = SC.good_file("blocky_128x128_q75_optimize")
    assert 6000 <= len(base) <= 8000
    segs, tail = C.split(base)
    files = edited(base, 48, 7) + [C.join(segs, tail[:len(tail) // 2])] + [f for _, f, _ in C.malformed()]
    return [(str(i), f) for i, f in enumerate(files)]


def test_statuses_and_pixels_equal_the_sequential_path_on_damaged_files(damaged):
    from attwarp_amd import jpeg
    files = [f for _, f in damaged]
    want = want_info(damaged, R.DEFAULT_SEGMENT_BYTES, R.DEFAULT_MAX_ROUNDS)
    assert sum(a for _, _, a in want) >= 5 and sum(1 for n, _, a in want if n and not a) >= 5     # both ends of the rule are met
    runs = {}
    for sub in ("auto", False):
        jf = jpeg.JpegFiles(files, device=DEV, substreams=sub)
        out = torch.full((jf.out_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
        scr = torch.full((jf.scratch.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
        jf.buffer, jf.scratch = out[G:G + jf.out_bytes], scr[G:G + jf.scratch.numel()]
        views, status = jf.run()
        runs[sub] = (status.cpu().tolist(), [v.cpu().numpy() for v in views], jf.substream_info())
        for t in (out, scr):
            assert bool((t[:G] == 0xA5).all()) and bool((t[-G:] == 0xA5).all())
    (st_a, px_a, info_a), (st_f, px_f, info_f) = runs["auto"], runs[False]
    assert [D.STATUS_NAMES[s] for s in st_a] == [D.STATUS_NAMES[s] for s in st_f] == [D.STATUS_NAMES[D.decode(f)[0]] for f in files]
    for s, a, b in zip(st_a, px_a, px_f):
        if s == 0:
            assert np.array_equal(a, b)
    assert all(i == (0, 0, 0) for i in info_f) and info_a == want


def test_a_mixed_batch():
    from attwarp_amd import jpeg
    files = [(n, C.good_file(n)) for n in ("ri_wrap", "noise_64x48_s1", "ri_stuffed_end")]
    files += [(n, SC.good_file(n)) for n in (SC.SHORT, "grey_160x120_q75", "smooth_256x192_q75_s2")]
    files += [("big_200x136", C.good_file("big_200x136"))]
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV)
    assert [n != 0 for n in jf.substreams()] == [False, True, False, False, True, True, False]
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    back_to_back(views, jf.buffer)
    check_views(views, files, "RGB")
    want = [D.decode(f)[2]["nunits"] for _, f in files]
    assert jf.units() == want and [r + 1 for r in jf.restarts()] == want and max(want) > 8
    assert jf.substream_info() == want_info(files, R.DEFAULT_SEGMENT_BYTES, R.DEFAULT_MAX_ROUNDS)


def test_two_runs_a_stream_a_graph_and_substreams_off_give_the_same_bytes():
    from attwarp_amd import jpeg
    files = [(n, SC.good_file(n)) for n in ("noise_128x96_q50_s1", "grey_160x120_q75")] + [("ri_wrap", C.good_file("ri_wrap"))]
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV)
    views, status = jf.run()
    first = jf.buffer.clone()
    info = jf.substream_info()
    assert status.cpu().tolist() == [0] * len(files) and [i[2] for i in info] == [1, 1, 0]
    check_views(views, files, "RGB")
    jf.buffer.fill_(0x5A)
    jf.run()
    assert torch.equal(jf.buffer, first) and jf.substream_info() == info
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        jf.buffer.fill_(0x5A)
        jf.run()
        s.synchronize()
        assert torch.equal(jf.buffer, first)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            jf.run()
        jf.buffer.zero_()
        jf.status.fill_(-1)
        g.replay()
        s.synchronize()
    assert jf.status.cpu().tolist() == [0] * len(files) and torch.equal(jf.buffer, first) and jf.substream_info() == info
    off = jpeg.JpegFiles([f for _, f in files], device=DEV, substreams=False)
    _, status = off.run()
    assert status.cpu().tolist() == [0] * len(files) and torch.equal(off.buffer, first)
    assert off.substreams() == [0, 0, 0] and off.substream_info() == [(0, 0, 0)] * 3
