"""GPU tests of the progressive scans' sub-streams (``scan_substreams``, jpegprog_substream_kernel): with the
keyword every pixel still equals Pillow's, statuses, pixels and the coefficient bytes in scratch equal those of the run
without it, the per-scan records equal the restatement's (tests/jpegprog_sync_ref.py) exactly, and every cut scan of a good file is
accepted given rounds enough.  Files of
at most a few hundred pixels a side at 32 bytes per segment, so that small scans still cut into several segments; the one
large file is the EOB run of 32767.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import jpegdec_cases as B
import jpegprog_cases as C
import jpegprog_ref as R
import jpegprog_sync_cases as SC
import jpegprog_sync_ref as Y
from test_jpegprog_gpu import DEV, G, pil, want_pixels

pytestmark = pytest.mark.gpu


BIG = ("eob_run", "eob_run_textured")                     # (their rounds in Python take too long: held by the plan alone)


def check_info(name, f, info, segment_bytes, status, max_rounds):
    """scan_substream_info() of one file = the restatement's record per scan (tests/jpegprog_sync_ref.py), exactly: route,
    segments, rounds and accepted.  (An AC refinement behind a failing scan reads coefficients the failure left: plan alone.)"""
    if name in BIG:
        assert [r[:2] for r in info] == Y.plan(R.parse(f), segment_bytes), name
        assert all(r[3] == (r[0] != 0) for r in info), name
        return
    want, _, exact = Y.records(f, segment_bytes, max_rounds)
    for i, (got, w, ex) in enumerate(zip(info, want, exact)):
        assert (got == w) if ex else (got[:2] == w[:2]), (name, i, got, w)
    assert len(info) == len(want), name


def both(files, segment_bytes, **kw):
    from attwarp_amd import jpeg
    on = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True, scan_substreams=True, segment_bytes=segment_bytes, **kw)
    off = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True, segment_bytes=segment_bytes, **kw)
    return on, off


def corpus():
    return C.good() + SC.limits() + SC.larger()


@pytest.mark.parametrize("segment_bytes,max_rounds", [(32, 4096), (32, None), (None, None)])
def test_whole_corpus_and_limit_files_in_one_call(segment_bytes, max_rounds):
    """max_rounds = 4096: a round settles at least one more segment, and the longest first pass of these files has fewer than 4096
    segments of 32 bytes, so every cut scan of a good file is accepted.  With the default rounds at 32 bytes the scans the
    restatement says fall back do, and nothing else changes."""
    from attwarp_amd import jpeg
    files = corpus() + ([("eob_run_textured", SC.eob_run_textured()), ("most_segments", SC.most_segments(0)),
                         ("one_segment_more", SC.most_segments(1))] if max_rounds else [])
    on, off = both(files, segment_bytes, max_rounds=max_rounds)
    sb, mr = segment_bytes or jpeg.SEGMENT_BYTES, max_rounds or jpeg.MAX_ROUNDS
    assert on.segment_bytes == sb and on.max_rounds == mr
    von, son = on.run()
    voff, soff = off.run()
    assert son.cpu().tolist() == soff.cpu().tolist() == [0] * len(files)
    assert torch.equal(on.buffer, off.buffer)
    infos = on.scan_substream_info()
    routes, cut, fell = set(), 0, 0
    for (name, f), v, ca, cb, info, segs in zip(files, von, on.coefficients(), off.coefficients(), infos, [p["scan_segments"] for p in on.parsed]):
        if max(v.shape) < 1000:
            assert np.array_equal(v.cpu().numpy(), want_pixels(name, f, "RGB", "rgb")), name
        assert torch.equal(ca, cb), name
        check_info(name, f, info, sb, 0, mr)
        assert [r[1] for r in info] == segs, name
        routes |= {r[0] for r in info}
        cut += sum(r[0] != 0 for r in info)
        fell += sum(r[0] != 0 and r[3] == 0 for r in info)
    assert (routes == {0, 1, 2, 3, 4} and cut > 150) if segment_bytes == 32 else cut > 0, (routes, cut)
    assert (fell == 0) if max_rounds or segment_bytes is None else fell >= 1, fell      # every cut scan of a good file is accepted
    assert all(r == (0, 0, 0, 0) for info in off.scan_substream_info() for r in info)
    if max_rounds:
        by = dict(zip([n for n, _ in files], infos))
        assert by["smallest_cut"][1][:2] == (2, 2) and by["one_byte_less"][1] == (0, 0, 0, 0)
        assert by["most_segments"][1] == (2, 16384, 0, 1) and by["one_segment_more"][1] == (0, 0, 0, 0)
        assert sum(r[0] == 4 for r in by["two_bands"]) == 2


def test_malformed_and_truncated_files_among_good_ones_and_guard_bytes():
    from attwarp_amd import jpeg
    bad = C.malformed()
    good = SC.larger()
    files = []
    for i, nf in enumerate(bad):                             # good files at the start, in between and at the end
        if i % 3 == 0:
            files.append(good[(i // 3) % len(good)])
        files.append(nf)
    big = SC.larger()[1][1]                                  # a larger file cut inside each of its scans: the cut scan is several segments long
    p = R.parse(big)
    for i, sc in enumerate(p["scans"]):
        end = next(x for x in R.markers(big) if x >= sc["off"])
        if end - sc["off"] >= 96:
            files.append((f"larger_cut_in_scan_{i}", big[:end - 7]))
    files.append(good[-1])
    want = [R.decode(f)[0] for _, f in files]
    assert sum(w != 0 for w in want) >= len(bad) + 5
    on, off = both(files, 32)
    out = torch.full((on.out_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    scr = torch.full((on.scratch.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    on.buffer, on.scratch = out[G:G + on.out_bytes], scr[G:G + on.scratch.numel()]
    von, son = on.run()
    voff, soff = off.run()
    got = son.cpu().tolist()
    assert got == soff.cpu().tolist() and [R.D.STATUS_NAMES[s] for s in got] == [R.D.STATUS_NAMES[s] for s in want]
    for t in (out, scr):
        assert bool((t[:G] == 0xA5).all()) and bool((t[-G:] == 0xA5).all())
    for (name, f), a, b, s, info in zip(files, von, voff, got, on.scan_substream_info()):
        if s == 0:
            assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), pil(f, "RGB")), name
        check_info(name, f, info, 32, s, jpeg.MAX_ROUNDS)


def test_a_scan_that_needs_more_rounds_than_max_rounds_falls_back():
    files = SC.larger()[:3] + SC.dc_scripts()
    on, off = both(files, 32, max_rounds=1)
    von, son = on.run()
    voff, soff = off.run()
    assert son.cpu().tolist() == soff.cpu().tolist() == [0] * len(files) and torch.equal(on.buffer, off.buffer)
    fell = 0
    for (name, f), ca, cb, info in zip(files, on.coefficients(), off.coefficients(), on.scan_substream_info()):
        assert torch.equal(ca, cb), name
        check_info(name, f, info, 32, 0, 1)
        for route, nseg, rounds, acc in info:
            if route in (1, 3) and nseg > 2:
                assert (rounds, acc) == (1, 0), (name, route, nseg)      # one round cannot settle three segments
                fell += 1
            elif route in (2, 4):
                assert acc == 1, (name, route)
    assert fell >= 10


def test_mixed_lists_keep_their_order_and_paths():
    from attwarp_amd import jpeg
    base = [(n, B.good_file(n)) for n in ("ri_wrap", "noise_64x48_s1", "big_200x136")]
    rows = C.save(C.noise(80, 96, 3, 51), quality=90, progressive=True, restart_marker_rows=1, subsampling=2)
    prog = SC.larger()[:2]
    files = [base[0], prog[0], ("rows", rows), base[1], base[2], prog[1]]
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True, scan_substreams=True, segment_bytes=32)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    for (name, f), v in zip(files, views):
        assert np.array_equal(v.cpu().numpy(), pil(f, "RGB")), name
    alone = jpeg.JpegFiles([f for _, f in base], device=DEV, segment_bytes=32)
    alone.run()
    idx, part = jf.parts[0]
    assert idx == [0, 3, 4] and not part.progressive and torch.equal(part.buffer, alone.buffer)
    assert part.substreams() == alone.substreams() and part.substream_info() == alone.substream_info()    # the baseline files' own sub-streams
    infos = jf.scan_substream_info()
    assert [infos[i] for i in idx] == [[], [], []]
    assert all(r == (0, 0, 0, 0) for r in infos[2]) and all(u > 1 for u in [s["units"] for s in jf.parsed[2]["scans"]])   # the restart rows keep their waves
    for i in (1, 5):
        check_info(files[i][0], files[i][1], infos[i], 32, 0, jpeg.MAX_ROUNDS)
        assert sum(r[3] for r in infos[i]) >= 4
    # an all_scans list: its plain progressive files take the same path
    every = jpeg.JpegFiles([f for _, f in files], device=DEV, all_scans=True, scan_substreams=True, segment_bytes=32)
    every.run()
    assert every.scan_substream_info() == infos


def test_two_runs_a_side_stream_and_a_replayed_graph_give_the_same_bytes():
    from attwarp_amd import jpeg
    files = SC.limits() + SC.larger()
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True, scan_substreams=True, segment_bytes=32)
    views, status = jf.run()
    first, coefs, infos = jf.buffer.clone(), [c.clone() for c in jf.coefficients()], jf.scan_substream_info()
    assert status.cpu().tolist() == [0] * len(files)
    for (name, f), v in zip(files, views):
        assert np.array_equal(v.cpu().numpy(), pil(f, "RGB")), name
    jf.buffer.fill_(0x5A)
    jf.run()
    assert torch.equal(jf.buffer, first) and jf.scan_substream_info() == infos
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    jf.buffer.fill_(0x5A)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _, status = jf.run()
        s.synchronize()
        assert status.cpu().tolist() == [0] * len(files) and torch.equal(jf.buffer, first)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            jf.run()
        for _ in range(2):
            jf.buffer.zero_()
            jf.status.fill_(-1)
            g.replay()
            s.synchronize()
            assert jf.status.cpu().tolist() == [0] * len(files) and torch.equal(jf.buffer, first)
            assert all(torch.equal(a, b) for a, b in zip(jf.coefficients(), coefs)) and jf.scan_substream_info() == infos


def test_the_upload_helpers_take_the_keyword():
    from attwarp_amd import jpeg, pipeline
    files = [f for _, f in SC.larger()[:3]]
    for up in (pipeline.upload_jpeg_files(files, device=DEV, progressive=True, scan_substreams="auto", segment_bytes=32),
               pipeline.upload_image_files(files, device=DEV, progressive=True, scan_substreams=True),
               jpeg.decode_jpeg(files, device=DEV, progressive=True, scan_substreams=True, segment_bytes=64)):
        for f, v in zip(files, up):
            assert np.array_equal(v.cpu().numpy(), pil(f, "RGB"))
    with pytest.raises(ValueError, match="scan_substreams"):
        jpeg.JpegFiles(files, device=DEV, progressive=True, scan_substreams="on")


def test_auto_cuts_only_the_kinds_that_pay():
    """scan_substreams="auto" = True for the scans of jpeg.AUTO_SCAN_KINDS, one lane for every other scan; the same pixels."""
    from attwarp_amd import jpeg
    files = SC.limits() + SC.larger()
    auto = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True, scan_substreams="auto", segment_bytes=32)
    every = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True, scan_substreams=True, segment_bytes=32)
    _, sa = auto.run()
    _, se = every.run()
    assert sa.cpu().tolist() == se.cpu().tolist() == [0] * len(files) and torch.equal(auto.buffer, every.buffer)
    assert 1 <= len(jpeg.AUTO_SCAN_KINDS) <= 4 and set(jpeg.AUTO_SCAN_KINDS) <= set(jpeg.SCAN_KINDS)
    kept = dropped = 0
    for (name, f), p, ia, ie in zip(files, auto.parsed, auto.scan_substream_info(), every.scan_substream_info()):
        for s, a, e, n in zip(p["scans"], ia, ie, p["scan_segments"]):
            want = e if jpeg.scan_kind(s) in jpeg.AUTO_SCAN_KINDS else (0, 0, 0, 0)
            assert a == want and n == want[1], (name, s["ss"], s["ah"])
            kept += a[0] != 0
            dropped += a[0] == 0 and e[0] != 0
    assert kept >= 20 and (dropped >= 5 or len(jpeg.AUTO_SCAN_KINDS) == 4)
