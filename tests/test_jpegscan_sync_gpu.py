"""GPU tests of the sub-streams of the scans-of-every-layout family (``scan_substreams`` with ``all_scans``,
jpegscan_substream_kernel): with the keyword every pixel still equals Pillow's, statuses, pixels and the
coefficient bytes in scratch equal those of the run without it, the per-scan records equal the restatement's
(tests/jpegscan_sync_ref.py) exactly, and every cut scan of a good file is accepted (every cut first pass of the corpus is
shorter than max_rounds - 1 segments, so its rounds settle for certain).  Small files at 32 bytes per segment.  No tolerance
anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import jpegdec_cases as B
import jpegfmt_cases as L
import jpegprog_sync_cases as PSC
import jpegscan_ref as R
import jpegscan_sync_cases as SC
import jpegscan_sync_ref as Y
from test_jpegscan_gpu import DEV, G, pil

pytestmark = pytest.mark.gpu


def check_info(name, f, info, segment_bytes, max_rounds, kinds=(0, 1, 2, 3)):
    """scan_substream_info() of one file = the restatement's record per scan, exactly: route, segments, rounds and accepted.
    (An AC refinement behind a failing scan reads coefficients the failure left: plan alone.)"""
    want, _, exact = Y.records(f, segment_bytes, max_rounds, kinds)
    assert len(info) == len(want), name
    for i, (got, w, ex) in enumerate(zip(info, want, exact)):
        assert (got == w) if ex else (got[:2] == w[:2]), (name, i, got, w)


def both(files, segment_bytes, mode="RGB", **kw):
    from attwarp_amd import jpeg
    on = jpeg.JpegFiles([f for _, f in files], mode, device=DEV, all_scans=True, scan_substreams=True, segment_bytes=segment_bytes, **kw)
    off = jpeg.JpegFiles([f for _, f in files], mode, device=DEV, all_scans=True, segment_bytes=segment_bytes, **kw)
    assert on.all_scans and off.all_scans and on.parts is None
    return on, off


def same_coefficients(a, b):
    return all(torch.equal(x, y) for pa, pb in zip(a.coefficients(), b.coefficients()) for x, y in zip(pa, pb))


def test_the_library_has_the_entry_points():
    from attwarp_amd import _lib
    for lib in (_lib.load(), _lib.load_tuning()):
        assert hasattr(lib, "attwarp_jpegdec_plan_layout_scans_ex") and hasattr(lib, "attwarp_jpegdec_layout_scans_table_bytes_ex")


@pytest.mark.parametrize("mode", ["RGB", "L", "keep"])
def test_whole_corpus_in_one_call_keyword_on_and_off(mode):
    from attwarp_amd import jpeg
    files = SC.good()
    on, off = both(files, 32, mode)
    assert on.segment_bytes == 32 and on.max_rounds == jpeg.MAX_ROUNDS
    von, son = on.run()
    voff, soff = off.run()
    assert son.cpu().tolist() == soff.cpu().tolist() == [0] * len(files)
    assert torch.equal(on.buffer, off.buffer) and same_coefficients(on, off)
    infos = on.scan_substream_info()
    routes, cut = set(), 0
    for (name, f), v, info, p in zip(files, von, infos, on.parsed):
        want = pil(f, mode)
        assert v.shape == want.shape and np.array_equal(v.cpu().numpy(), want), (name, mode)
        check_info(name, f, info, 32, jpeg.MAX_ROUNDS)
        assert [r[1] for r in info] == p["scan_segments"], name
        assert all(r[3] == (r[0] != 0) for r in info), (name, info)              # every cut scan of a good file is accepted
        routes |= {r[0] for r in info}
        cut += sum(r[0] != 0 for r in info)
    assert routes == {0, 1, 2, 3, 4} and cut > 100, (routes, cut)
    assert all(r == (0, 0, 0, 0) for info in off.scan_substream_info() for r in info)
    by = dict(zip([n for n, _ in files], infos))
    assert by["smallest_cut"][1][:2] == (2, 2) and by["one_byte_less"][1] == (0, 0, 0, 0)
    assert by["sequential"] == [(0, 0, 0, 0)] * 3 and sum(r[0] == 4 for r in by["two_bands"]) == 2
    assert by["ten_blocks"][0][0] == 1 and by["ten_blocks"][-1][0] == 2
    ticks = on.scan_substream_ticks()
    assert all((sum(t) > 0) == (r[0] != 0) for ti, info in zip(ticks, infos) for t, r in zip(ti, info))


def test_malformed_files_among_good_ones_and_guard_bytes():
    from attwarp_amd import jpeg
    bad = SC.malformed()
    good = SC.good()[::3]
    files = []
    for i, nf in enumerate(bad):                             # good files at the start, in between and at the end
        if i % 3 == 0:
            files.append(good[(i // 3) % len(good)])
        files.append(nf)
    files.append(good[-1])
    want = [R.decode(f)[0] for _, f in files]
    assert sum(w != 0 for w in want) == len(bad)
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
    refused = 0
    for (name, f), a, b, s, info in zip(files, von, voff, got, on.scan_substream_info()):
        if s == 0:
            assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), pil(f, "RGB")), name
        check_info(name, f, info, 32, jpeg.MAX_ROUNDS)
        refused += sum(r[0] != 0 and r[3] == 0 for r in info)
    assert refused >= 5                                      # the scans damaged inside their segments went to the one-lane route


def test_a_scan_that_needs_more_rounds_than_max_rounds_falls_back():
    files = [nf for nf in SC.good() if nf[0] in ("ten_blocks", "padded_411", "distinct_2111", "pil_cmyk_444", "subset_02_of_k2x2")]
    on, off = both(files, 32, max_rounds=1)
    von, son = on.run()
    voff, soff = off.run()
    assert son.cpu().tolist() == soff.cpu().tolist() == [0] * len(files) and torch.equal(on.buffer, off.buffer) and same_coefficients(on, off)
    fell = 0
    for (name, f), info in zip(files, on.scan_substream_info()):
        check_info(name, f, info, 32, 1)
        for route, nseg, rounds, acc in info:
            if route in (1, 3) and nseg > 2:
                assert (rounds, acc) == (1, 0), (name, route, nseg)      # one round cannot settle three segments
                fell += 1
            elif route in (2, 4):
                assert acc == 1, (name, route)
    assert fell >= 10


def test_a_mixed_list_keeps_the_older_parts_as_they_are():
    """Baseline, plain progressive, layout and scanned files in one list: each older part's buffer and records equal those of
    the call on it alone, and the scanned part's equal its own."""
    from attwarp_amd import jpeg
    base = [(n, B.good_file(n)) for n in ("ri_wrap", "noise_64x48_s1")]
    prog = PSC.larger()[:2]
    lay = [(n, L.good_file(n)) for n in ("cmyk_s2_33x20", "coef_410_33x17")]
    scanned = [nf for nf in SC.good() if nf[0] in ("ten_blocks", "repeating_abab", "sequential")]
    files = [base[0], scanned[0], prog[0], lay[0], scanned[1], base[1], prog[1], lay[1], scanned[2]]
    kw = dict(device=DEV, scan_substreams=True, segment_bytes=32)
    jf = jpeg.JpegFiles([f for _, f in files], all_scans=True, **kw)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    for (name, f), v in zip(files, views):
        assert np.array_equal(v.cpu().numpy(), pil(f, "RGB")), name
    infos = jf.scan_substream_info()
    alone = [jpeg.JpegFiles([f for _, f in base], **kw), jpeg.JpegFiles([f for _, f in prog], progressive=True, **kw),
             jpeg.JpegFiles([f for _, f in lay], all_layouts=True, **kw), jpeg.JpegFiles([f for _, f in scanned], all_scans=True, **kw)]
    assert [idx for idx, _ in jf.parts] == [[0, 5], [2, 6], [3, 7], [1, 4, 8]]
    for (idx, part), one in zip(jf.parts, alone):
        one.run()
        assert bytes(part.table_host) == bytes(one.table_host) and torch.equal(part.buffer, one.buffer)
        assert part.scan_substream_info() == one.scan_substream_info() == [infos[i] for i in idx]
        assert part.substream_info() == one.substream_info()
    assert infos[0] == infos[3] == [] and sum(r[3] for r in infos[2]) >= 4 and sum(r[3] for r in infos[1]) >= 4
    for i in (1, 4, 8):
        check_info(files[i][0], files[i][1], infos[i], 32, jpeg.MAX_ROUNDS)
    # the older parts do not depend on the keyword's reach into the scanned part: the same list without a scanned file
    three = jpeg.JpegFiles([f for i, (_, f) in enumerate(files) if i not in (1, 4, 8)], all_scans=True, **kw)
    three.run()
    for (_, a), (_, b) in zip(three.parts, jf.parts[:3]):
        assert bytes(a.table_host) == bytes(b.table_host) and torch.equal(a.buffer, b.buffer)


def test_auto_cuts_exactly_the_kinds_it_names():
    from attwarp_amd import jpeg
    files = SC.good()
    auto = jpeg.JpegFiles([f for _, f in files], device=DEV, all_scans=True, scan_substreams="auto", segment_bytes=32)
    every = jpeg.JpegFiles([f for _, f in files], device=DEV, all_scans=True, scan_substreams=True, segment_bytes=32)
    _, sa = auto.run()
    _, se = every.run()
    assert sa.cpu().tolist() == se.cpu().tolist() == [0] * len(files) and torch.equal(auto.buffer, every.buffer)
    assert 1 <= len(jpeg.AUTO_LAYOUT_SCAN_KINDS) <= 4 and set(jpeg.AUTO_LAYOUT_SCAN_KINDS) <= set(jpeg.SCAN_KINDS)
    kinds = [jpeg.SCAN_KINDS.index(k) for k in jpeg.AUTO_LAYOUT_SCAN_KINDS]
    kept = dropped = 0
    for (name, f), p, ia, ie in zip(files, auto.parsed, auto.scan_substream_info(), every.scan_substream_info()):
        check_info(name, f, ia, 32, jpeg.MAX_ROUNDS, kinds)
        for s, a, e, n in zip(p["scans"], ia, ie, p["scan_segments"]):
            named = not s.get("sequential") and jpeg.scan_kind(s) in jpeg.AUTO_LAYOUT_SCAN_KINDS
            assert a == (e if named else (0, 0, 0, 0)) and n == a[1], (name, s["ss"], s["ah"])
            kept += a[0] != 0
            dropped += a[0] == 0 and e[0] != 0
    assert kept >= 20 and (dropped >= 5 or len(jpeg.AUTO_LAYOUT_SCAN_KINDS) == 4)


def test_two_runs_a_side_stream_and_a_replayed_graph_give_the_same_bytes():
    from attwarp_amd import jpeg
    files = SC.good()
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, all_scans=True, scan_substreams=True, segment_bytes=32)
    views, status = jf.run()
    first, coefs, infos = jf.buffer.clone(), [[c.clone() for c in pl] for pl in jf.coefficients()], jf.scan_substream_info()
    assert status.cpu().tolist() == [0] * len(files)
    for (name, f), v in zip(files, views):
        assert np.array_equal(v.cpu().numpy(), pil(f, "RGB")), name

    def same():
        return (torch.equal(jf.buffer, first) and jf.scan_substream_info() == infos and
                all(torch.equal(a, b) for pa, pb in zip(jf.coefficients(), coefs) for a, b in zip(pa, pb)))

    jf.buffer.fill_(0x5A)
    jf.run()
    assert same()
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    jf.buffer.fill_(0x5A)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _, status = jf.run()
        s.synchronize()
        assert status.cpu().tolist() == [0] * len(files) and same()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            jf.run()
        for _ in range(2):
            jf.buffer.zero_()
            jf.status.fill_(-1)
            g.replay()
            s.synchronize()
            assert jf.status.cpu().tolist() == [0] * len(files) and same()


def test_keyword_off_table_is_plan_layout_scans_byte_for_byte_and_launches_are_the_plans():
    from attwarp_amd import _lib, jpeg
    files = [f for _, f in SC.good()]
    seen = {}
    inner = jpeg.planned_table

    def spy(size, planner, *a, **k):
        assert planner[0] == "attwarp_jpegdec_plan_layout_scans" and size[0] == "attwarp_jpegdec_layout_scans_table_bytes"
        _, rp, nb, srec, nscans, _, by_level = planner
        lib = _lib.load()
        n = lib.attwarp_jpegdec_layout_scans_table_bytes(rp, ctypes.c_int(nb), ctypes.c_int(nscans))
        buf = (ctypes.c_uint8 * n)(*([0xA5] * n))
        assert lib.attwarp_jpegdec_plan_layout_scans(rp, ctypes.c_int(nb), ctypes.c_void_p(srec), ctypes.c_int(nscans), buf, ctypes.c_size_t(n),
                                                     ctypes.c_int(by_level)) == 0
        seen["plain"] = bytes(buf)
        return inner(size, planner, *a, **k)

    jpeg.planned_table = spy
    try:
        off = jpeg.JpegFiles(files, device=DEV, all_scans=True, segment_bytes=32)
    finally:
        jpeg.planned_table = inner
    assert bytes(off.table_host) == seen["plain"]
    on = jpeg.JpegFiles(files, device=DEV, all_scans=True, scan_substreams=True, segment_bytes=32)
    n = len(seen["plain"])
    assert bytes(on.table_host)[64:n] == seen["plain"][64:] and len(bytes(on.table_host)) > n       # the parent's records, then the trailer


def test_the_upload_helpers_take_the_keyword():
    from attwarp_amd import jpeg, pipeline
    files = [f for n, f in SC.good() if n in ("pil_cmyk_420", "pil_440", "ten_blocks")]
    for up in (pipeline.upload_jpeg_files(files, device=DEV, all_scans=True, scan_substreams="auto", segment_bytes=32),
               pipeline.upload_image_files(files, device=DEV, all_scans=True, scan_substreams=True),
               jpeg.decode_jpeg(files, device=DEV, all_scans=True, scan_substreams=True, segment_bytes=64)):
        for f, v in zip(files, up):
            assert np.array_equal(v.cpu().numpy(), pil(f, "RGB"))
    with pytest.raises(ValueError, match="scan_substreams"):
        jpeg.JpegFiles(files, device=DEV, all_scans=True, scan_substreams="on")
