"""GPU tests of the JPEG decoder's scans-of-any-layout family (attwarp_jpegdec_decode_layout_scans, attwarp_amd/jpeg.py with
``all_scans=True``): every pixel equals Pillow's, every status equals the restatement's (tests/jpegscan_ref.py), the level
plan leaves the same coefficient bytes as one launch per scan position, and the three older kinds of a list keep the
tables they take today.  No tolerance anywhere."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpegdec_cases as B
import jpegfmt_cases as L
import jpegfmt_ref as F
import jpegprog_cases as PC
import jpegscan_cases as C
import jpegscan_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = 256                                                    # guard bytes (the scratch buffer is 256-byte aligned)


def pil(f, mode, order="rgb"):
    a = F.pillow(f, mode)
    return a[:, :, ::-1] if order == "bgr" and a.shape[2] == 3 else a


@pytest.mark.parametrize("mode,order", [("RGB", "rgb"), ("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr"), ("L", "bgr"), ("keep", "bgr")])
def test_whole_corpus_in_one_call(mode, order):
    from attwarp_amd import jpeg
    files = C.good()
    jf = jpeg.JpegFiles([f for _, f in files], mode, order, device=DEV, all_scans=True)
    assert jf.all_scans and jf.parts is None
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    off = jf.buffer.data_ptr()
    for (name, f), v in zip(files, views):
        assert v.data_ptr() == off
        off += v.numel()
        want = pil(f, mode, order)
        got = v.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (name, mode, order)
    parsed = [R.parse(f) for _, f in files]
    assert jf.units() == [p["units"] for p in parsed]
    assert [r + len(p["scans"]) for r, p in zip(jf.restarts(), parsed)] == jf.units()
    assert jf.levels() == [max(p["levels"]) + 1 for p in parsed] and all(l == 1 for l, p in zip(jf.levels(), parsed) if p["sequential"])


def test_level_plan_equals_one_launch_per_scan_down_to_the_coefficient_bytes():
    """The test of the band rule: quality-100 noise and the scripts with one scan per band, where every band of every block
    is busy and one level holds several bands of one block."""
    from attwarp_amd import jpeg
    files = [nf for nf in C.good() if "q100" in nf[0] or "split_at" in nf[0] or "approx" in nf[0] or nf[0].startswith("seq_")][::2]
    files += [(n, f) for n, f, _ in C.limits()] + C.malformed()
    assert sum("q100" in n for n, _ in files) >= 3 and sum("split_at" in n for n, _ in files) >= 10
    a = jpeg.JpegFiles([f for _, f in files], "keep", device=DEV, all_scans=True)
    b = jpeg.JpegFiles([f for _, f in files], "keep", device=DEV, all_scans=True, levels=False)
    assert max(a.levels()) < max(len(p["scans"]) for p in b.parsed) == 64
    va, sa = a.run()
    vb, sb = b.run()
    sa, sb = sa.cpu().tolist(), sb.cpu().tolist()
    assert sa == sb == [R.decode(f)[0] for _, f in files]
    for (name, f), x, y, ca, cb, s in zip(files, va, vb, a.coefficients(), b.coefficients(), sa):
        if s == 0:
            assert torch.equal(x, y), name
            for pa, pb, want in zip(ca, cb, R.decode(f)[2]["planes"]):
                assert torch.equal(pa, pb) and np.array_equal(pa.cpu().numpy(), want), name


def test_malformed_files_among_good_ones_and_guard_bytes():
    from attwarp_amd import jpeg
    bad = C.malformed()
    good = C.good()[5::40]
    files = []
    for i, nf in enumerate(bad):                             # good files at the start, in between and at the end
        if i % 3 == 0:
            files.append(good[(i // 3) % len(good)])
        files.append(nf)
    files.append(good[-1])
    want = [R.decode(f)[0] for _, f in files]
    assert sum(w != 0 for w in want) == len(bad) and set(want) == {0, 1, 2, 3, 4, 5}
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, all_scans=True)
    out = torch.full((jf.out_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    scr = torch.full((jf.scratch.numel() + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    jf.buffer, jf.scratch = out[G:G + jf.out_bytes], scr[G:G + jf.scratch.numel()]
    views, status = jf.run()
    got = status.cpu().tolist()
    assert [R.D.STATUS_NAMES[s] for s in got] == [R.D.STATUS_NAMES[s] for s in want]
    for t in (out, scr):
        assert bool((t[:G] == 0xA5).all()) and bool((t[-G:] == 0xA5).all())
    for (name, f), v, s in zip(files, views, got):
        if s == 0:
            assert np.array_equal(v.cpu().numpy(), pil(f, "RGB")), name
    first_bad = next(i for i, s in enumerate(want) if s)
    with pytest.raises(OSError, match=rf"file {first_bad} .*{R.D.STATUS_NAMES[want[first_bad]]}"):
        jpeg.decode_jpeg([f for _, f in files], device=DEV, all_scans=True)


def _mixed():
    png = io.BytesIO()
    Image.fromarray(C.C.noise(21, 30, 3, 3)).save(png, "PNG")
    return [("baseline", B.good_file("noise_64x48_s1")), ("prog_420", PC.pillow()[10][1]), ("new_prog_cmyk", C.good_file("pil_cmyk_s2_33x20")),
            ("png", png.getvalue()), ("seq_cmyk", L.good_file("cmyk_s2_33x20")), ("new_seq_420", C.good_file("seq_420_33x20_ri_row")),
            ("baseline_ri", B.good_file("ri_wrap")), ("new_prog_440", C.good_file("edit_440_24x32")), ("prog_420_b", PC.pillow()[30][1])]


def test_a_list_of_all_kinds_comes_back_in_input_order_and_the_older_parts_keep_their_tables():
    from attwarp_amd import jpeg, pipeline
    files = _mixed()
    up = pipeline.upload_image_files([f for _, f in files], device=DEV, all_scans=True)
    for (name, f), v in zip(files, up):
        assert np.array_equal(v.cpu().numpy(), pil(f, "RGB")), name
    jpegs = [(n, f) for n, f in files if n != "png"]
    jf = jpeg.JpegFiles([f for _, f in jpegs], device=DEV, all_scans=True)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(jpegs)
    for (name, f), v in zip(jpegs, views):
        assert np.array_equal(v.cpu().numpy(), pil(f, "RGB")), name
    assert [idx for idx, _ in jf.parts] == [[0, 5], [1, 7], [3], [2, 4, 6]]
    older = (dict(), dict(progressive=True), dict(all_layouts=True))
    for (idx, part), kw in zip(jf.parts[:3], older):
        alone = jpeg.JpegFiles([jpegs[i][1] for i in idx], device=DEV, **kw)
        alone.run()
        assert part._entry == alone._entry and part.table_host.tobytes() == alone.table_host.tobytes() and torch.equal(part.buffer, alone.buffer)
    assert jf.parts[3][1].all_scans and jf.levels()[0] == 0 and jf.levels()[4] == 1 and jf.levels()[2] == 1 + max(R.parse(jpegs[2][1])["levels"])
    with pytest.raises(ValueError, match="out must be None"):
        jpeg.JpegFiles([f for _, f in jpegs], device=DEV, all_scans=True, out=torch.empty(1 << 20, dtype=torch.uint8, device=DEV))


def test_without_the_keyword_the_same_list_raises():
    from attwarp_amd import jpeg, pipeline
    files = [f for _, f in _mixed()]
    for kw in (dict(), dict(progressive=True), dict(all_layouts=True), dict(progressive=True, all_layouts=True)):
        with pytest.raises(ValueError, match="progressive|all_layouts covers sequential files only|more than one scan|components"):
            pipeline.upload_image_files(files, device=DEV, **kw)
    with pytest.raises(ValueError, match="all_layouts covers sequential files only"):
        jpeg.decode_jpeg([C.good_file("pil_cmyk_s2_33x20")], device=DEV, progressive=True, all_layouts=True)
    with pytest.raises(ValueError, match="more than one scan"):
        jpeg.decode_jpeg([C.good_file("seq_420_33x20_ri_row")], device=DEV, progressive=True, all_layouts=True)


def test_two_runs_a_side_stream_and_a_replayed_graph_give_the_same_bytes():
    from attwarp_amd import jpeg
    files = C.good()[3::23]
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, all_scans=True)
    views, status = jf.run()
    first = jf.buffer.clone()
    assert status.cpu().tolist() == [0] * len(files)
    for (name, f), v in zip(files, views):
        assert np.array_equal(v.cpu().numpy(), pil(f, "RGB")), name
    jf.buffer.fill_(0x5A)
    jf.run()
    assert torch.equal(jf.buffer, first)
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
