"""GPU tests of the PNG encoder's match="lz" route (csrc/png.hip png_encode_lz_kernel) on the corpus of
tests/pnglz_cases.py, which test_pnglz_ref_cpu.py proves on the CPU: ONE PngBatch with `match` per image, "rle" and "lz"
mixed.  Equality everywhere: every file is the restatement's byte for byte, the "rle" images are png_ref's, the files decode
with Pillow and with the project's own decoder (unit route) to the source pixels, routes() is the restatement's choice per
segment, nothing outside the files is written, and a captured run re-encodes what the sources hold at replay."""
import numpy as np
import pytest
import torch

import png_ref as R
import pnglz_cases as C
import pnglz_ref as Z
from test_png_gpu import decode, same_bytes
from test_png_limits_gpu import place

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64


@pytest.fixture(scope="module")
def corpus():
    from attwarp_amd import png
    cases = C.cases()
    tens = {c.name: place(c.image, bool(c.expect.get("odd_placement"))) for c in cases}
    b = png.PngBatch([tens[c.name] for c in cases], filter=[c.filter for c in cases], order=[c.order for c in cases],
                     match=[c.match for c in cases])
    files = png.download(*b.run())
    return cases, tens, b, files


def batch_of(names, tens, out=None):
    from attwarp_amd import png
    cs = [C.case(n) for n in names]
    return png.PngBatch([tens[n] for n in names], filter=[c.filter for c in cs], order=[c.order for c in cs],
                        match=[c.match for c in cs], out=out)


def test_whole_corpus_equals_the_restatement_and_decodes(corpus):
    cases, tens, b, files = corpus
    assert {c.match for c in cases} == {"rle", "lz"}
    assert sum(not tens[c.name].is_contiguous() for c in cases if c.name.startswith("tail_")) >= 7
    offs = b.offsets.cpu().numpy()
    assert offs[0] == 0 and (np.diff(offs) == [len(f) for f in files]).all() and offs[-1] <= b.bound
    assert b.bound == sum(R.bound(*c.image.shape) for c in cases)
    routes = b.routes()
    assert len(routes) == b.segments == sum(len(C.reference(c.name)[1]) for c in cases)
    at = 0
    for c, f in zip(cases, files):
        want, wroutes, _ = C.reference(c.name)
        same_bytes(f, want, c.name)
        if c.match == "rle":
            assert f == R.encode(c.image, c.filter, c.order), c.name
        pix = c.image[:, :, ::-1] if c.order == "bgr" and c.image.shape[2] == 3 else c.image
        assert np.array_equal(decode(f).reshape(pix.shape), pix), c.name
        assert routes[at:at + len(wroutes)] == wroutes, c.name
        if c.name.startswith("glyph_") and c.match == "lz":
            assert Z.ROUTE_LZ in wroutes
        at += len(wroutes)


def test_round_trip_through_the_projects_decoder(corpus):
    from attwarp_amd import png
    cases, tens, b, files = corpus
    pf = png.PngFiles(files, "keep", device=DEV)
    views, status = pf.run()
    assert status.cpu().tolist() == [0] * len(cases)
    for c, v, r in zip(cases, views, pf.routes()):
        want = c.image[:, :, ::-1] if c.order == "bgr" and c.image.shape[2] == 3 else c.image
        assert tuple(v.shape) == want.shape and np.array_equal(v.cpu().numpy(), want), c.name
        if c.match == "lz" and len(C.reference(c.name)[1]) > 1:
            assert r[0] == 0, (c.name, r)                   # the unit route: every segment decodes on its own


def test_the_same_image_alone_and_at_every_place(corpus):
    from attwarp_amd import png
    cases, tens, b, files = corpus
    names = [c.name for c in cases]
    want = C.reference("small_first")[0]
    assert names[0] == "small_first" and names[-1] == "small_last" and 0 < names.index("small_middle") < len(names) - 1
    assert files[0] == files[names.index("small_middle")] == files[-1] == want
    alone = png.encode_png([tens["small_first"]], "sub", match="lz")
    assert alone == [want]
    assert png.encode_png([tens["small_first"]], "sub") == [R.encode(C.case("small_first").image, "sub")]


def test_guard_bytes_and_every_output_alignment(corpus):
    cases, tens, _, _ = corpus
    names = C.guard_batch()
    want = [C.reference(n)[0] for n in names]
    seen = []
    for k in range(4):
        bound = sum(R.bound(*C.case(n).image.shape) for n in names)
        out = torch.full((GUARD + k + bound + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        b = batch_of(names, tens, out=out[GUARD + k:GUARD + k + bound])
        assert b.bound == bound and out.data_ptr() % 4 == 0
        n = b.scratch.numel()
        scr = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        b.scratch = scr[GUARD:GUARD + n]
        assert b.scratch.data_ptr() % 16 == 0
        buf, offsets = b.run()
        torch.cuda.synchronize()
        offs = offsets.cpu().tolist()
        assert offs == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        assert bool((out[:GUARD + k] == 0xA5).all()) and bool((out[GUARD + k + offs[-1]:] == 0xA5).all()), k
        assert bool((scr[:GUARD] == 0xA5).all()) and bool((scr[-GUARD:] == 0xA5).all()), k
        data = buf[:offs[-1]].cpu().numpy().tobytes()
        files = [data[a:e] for a, e in zip(offs[:-1], offs[1:])]
        for name, f, w in zip(names, files, want):
            same_bytes(f, w, (name, k))
        seen.append(files)
    assert all(s == seen[0] for s in seen[1:])


def test_graph_replay_encodes_the_content_of_the_replay(corpus):
    from attwarp_amd import png
    a, z = C.case("small_first"), C.case("glyph_sub_bgr")
    other = C.glyph_page(77, *a.image.shape[:2], 1)
    src = [torch.from_numpy(a.image).to(DEV), torch.from_numpy(z.image).to(DEV)]
    b = png.PngBatch(src, filter=["sub", "sub"], order=["rgb", "bgr"], match=["lz", "lz"])
    b.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.run()
    src[0].copy_(torch.from_numpy(other))
    b.buffer.zero_()
    g.replay()
    torch.cuda.synchronize()
    files = png.download(b.buffer, b.offsets)
    same_bytes(files[0], Z.encode(other, "sub")[0], "replayed with new content")
    same_bytes(files[1], C.reference("glyph_sub_bgr")[0], "unchanged neighbour")
    assert files[0] != C.reference("small_first")[0]


def test_keyword_is_refused_before_any_launch():
    from attwarp_amd import png
    t = torch.zeros(4, 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        png.PngBatch([t], match="lazy")
    with pytest.raises(ValueError):
        png.PngBatch([t, t], match=["lz"])
