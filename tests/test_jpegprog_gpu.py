"""GPU tests of the progressive JPEG decoder (attwarp_jpegdec_decode_scans, attwarp_amd/jpeg.py with ``progressive=True``):
every pixel equals Pillow's (the restatement's, tests/jpegprog_ref.py, for the hostile file), every status equals the
restatement's, and the level plan leaves the same coefficients as one launch per scan.  No tolerance anywhere."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpegdec_cases as B
import jpegprog_cases as C
import jpegprog_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = 256                                                    # guard bytes (the scratch buffer is 256-byte aligned)


def pil(f, mode):
    a = np.asarray(Image.open(io.BytesIO(f)).convert(mode))
    return a if a.ndim == 3 else a[:, :, None]


def want_pixels(name, f, mode, order):
    hostile = {n for n, _ in C.hostile()}
    if name in hostile:
        return R.decode(f, mode, order)[1]
    if mode == "keep":
        mode = "L" if R.parse(f)["ncomp"] == 1 else "RGB"
    p = pil(f, mode)
    return p[:, :, ::-1] if order == "bgr" and p.shape[2] == 3 else p


@pytest.mark.parametrize("mode,order", [("RGB", "rgb"), ("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr")])
def test_whole_corpus_in_one_call(mode, order):
    from attwarp_amd import jpeg
    files = C.good()
    jf = jpeg.JpegFiles([f for _, f in files], mode, order, device=DEV, progressive=True)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    off = jf.buffer.data_ptr()
    for (name, f), v in zip(files, views):
        assert v.data_ptr() == off
        off += v.numel()
        want = want_pixels(name, f, mode, order)
        got = v.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (name, mode, order)
    assert jf.units() == [R.parse(f)["units"] for _, f in files]
    assert [r + len(R.parse(f)["scans"]) for r, (_, f) in zip(jf.restarts(), files)] == jf.units()
    assert jf.levels() == [max(R.parse(f)["levels"]) + 1 for _, f in files] and jf.levels()[0] == 3 and max(jf.levels()) == 14


def test_malformed_files_among_good_ones_and_guard_bytes():
    from attwarp_amd import jpeg
    bad = C.malformed()
    good = C.pillow()[3:40:6]
    files = []
    for i, nf in enumerate(bad):                             # good files at the start, in between and at the end
        if i % 3 == 0:
            files.append(good[(i // 3) % len(good)])
        files.append(nf)
    files.append(good[-1])
    want = [R.decode(f)[0] for _, f in files]
    assert sum(w != 0 for w in want) == len(bad) and set(want) == {0, 1, 2, 3, 4, 5}
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True)
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
        jpeg.decode_jpeg([f for _, f in files], device=DEV, progressive=True)


def test_level_plan_equals_one_launch_per_scan_down_to_the_coefficients():
    """The test of the band rule: quality-100 noise, where every band of every block is busy, and the transcoded scripts
    whose levels hold several bands of one block."""
    from attwarp_amd import jpeg
    files = [nf for nf in C.good() if "q100" in nf[0] or "split_at" in nf[0] or "refinements" in nf[0] or "dc_" in nf[0]] + C.malformed()
    assert sum("q100" in n for n, _ in files) == 9
    a = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True)
    b = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True, levels=False)
    assert max(a.levels()) < max(len(p["scans"]) for p in b.parsed)
    va, sa = a.run()
    vb, sb = b.run()
    sa, sb = sa.cpu().tolist(), sb.cpu().tolist()
    assert sa == sb == [R.decode(f)[0] for _, f in files]
    for (name, f), x, y, ca, cb, s in zip(files, va, vb, a.coefficients(), b.coefficients(), sa):
        if s == 0:
            assert torch.equal(x, y) and torch.equal(ca, cb), name
            planes = R.decode(f)[2]["planes"]
            want = np.concatenate([p.reshape(-1, 64) for p in planes])
            assert np.array_equal(ca.cpu().numpy(), want), name


def test_mixed_baseline_and_progressive_files_keep_their_order_and_paths():
    from attwarp_amd import jpeg
    base = [(n, B.good_file(n)) for n in ("ri_wrap", "noise_64x48_s1", "big_200x136")]
    prog = C.pillow()[4:20:5]
    files = [base[0], prog[0], prog[1], base[1], base[2], prog[2]]
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True)
    views, status = jf.run()
    assert status.cpu().tolist() == [0] * len(files)
    for (name, f), v in zip(files, views):
        assert np.array_equal(v.cpu().numpy(), pil(f, "RGB")), name
    alone = jpeg.JpegFiles([f for _, f in base], device=DEV)
    alone.run()
    idx, part = jf.parts[0]
    assert idx == [0, 3, 4] and not part.progressive and torch.equal(part.buffer, alone.buffer)
    assert part.substreams() == alone.substreams() and part.substream_info() == alone.substream_info()
    assert [jf.substream_info()[i] for i in idx] == alone.substream_info()
    with pytest.raises(ValueError, match="out must be None"):
        jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True, out=torch.empty(1 << 20, dtype=torch.uint8, device=DEV))


def test_two_runs_a_side_stream_and_a_replayed_graph_give_the_same_bytes():
    from attwarp_amd import jpeg
    files = C.pillow()[1:41:4] + [(n, f) for n, f, _ in C.transcoded()[:7]]
    jf = jpeg.JpegFiles([f for _, f in files], device=DEV, progressive=True)
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


def test_upload_image_files_with_a_png_in_the_list(tmp_path):
    from attwarp_amd import pipeline
    a = C.noise(21, 30, 3, 3)
    png = io.BytesIO()
    Image.fromarray(a).save(png, "PNG")
    files = [C.pillow()[10][1], png.getvalue(), C._colour_source(), C.pillow()[30][1]]
    up = pipeline.upload_image_files(files, device=DEV, progressive=True)
    for f, v in zip(files, up):
        assert np.array_equal(v.cpu().numpy(), pil(f, "RGB"))
    with pytest.raises(ValueError, match="progressive"):
        pipeline.upload_image_files(files, device=DEV)


def test_without_the_keyword_progressive_files_are_still_refused():
    from attwarp_amd import jpeg
    with pytest.raises(ValueError, match="progressive"):
        jpeg.decode_jpeg([f for _, f in C.pillow()[:3]], device=DEV)


def test_eob_run_of_32767_in_a_first_pass_and_in_a_refinement():
    from attwarp_amd import jpeg
    f, p, planes = C.eob_run_case()
    jf = jpeg.JpegFiles([f], "L", device=DEV, progressive=True)
    views, status = jf.run()
    assert status.cpu().tolist() == [0]
    assert np.array_equal(jf.coefficients()[0].cpu().numpy(), planes[0].reshape(-1, 64))
    assert np.array_equal(views[0].cpu().numpy(), pil(f, "L"))
