"""GPU tests of the PNG encoder at its limits (tests/png_limit_cases.py, proved on the CPU by test_png_limits_ref_cpu.py):
15-bit codes, two and three limiter rounds, one run filling a segment, every match length, all 286 symbols, the stored /
dynamic tie, full segments down both paths, 600 segments in one image, 1024 rows in one segment, adaptive ties, and every
filter at every row tail in both channel orders.  Equality everywhere: each file is the restatement's byte for byte, decodes
with Pillow and with the project's own decoder to the source pixels, and nothing outside the files is written."""
import numpy as np
import pytest
import torch

import png_limit_cases as L
import png_ref as R
from test_png_gpu import check_file, same_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64


def place(img, odd):
    """The image on the device; `odd`: at an odd byte address with a row pitch that is no multiple of 4."""
    t = torch.from_numpy(np.ascontiguousarray(img)).to(DEV)
    if not odd:
        return t
    H, W, C = img.shape
    pitch = W * C + 5
    pitch += pitch % 4 == 0
    flat = torch.zeros(3 + H * pitch, dtype=torch.uint8, device=DEV)
    view = flat[3:].as_strided((H, W, C), (pitch, C, 1))
    view.copy_(t)
    assert view.data_ptr() % 2 == 1 and pitch % 4 != 0
    return view


@pytest.fixture(scope="module")
def corpus():
    """Every case on the device (the tails marked so at odd addresses), one PngBatch, one run."""
    from attwarp_amd import png
    cases = L.cases()
    tens = {c.name: place(c.image, bool(c.expect.get("odd_placement"))) for c in cases}
    b = png.PngBatch([tens[c.name] for c in cases], filter=[c.filter for c in cases], order=[c.order for c in cases])
    files = png.download(*b.run())
    return cases, tens, b, files


def batch_of(names, tens, out=None):
    from attwarp_amd import png
    cs = [L.case(n) for n in names]
    return png.PngBatch([tens[n] for n in names], filter=[c.filter for c in cs], order=[c.order for c in cs], out=out)


def test_whole_corpus_equals_the_restatement_and_decodes(corpus):
    cases, tens, b, files = corpus
    assert 3 * sum(not tens[c.name].is_contiguous() for c in cases if c.name.startswith("tail_")) >= sum(c.name.startswith("tail_") for c in cases)
    offs = b.offsets.cpu().numpy()
    assert offs[0] == 0 and (np.diff(offs) == [len(f) for f in files]).all() and offs[-1] <= b.bound
    assert b.bound == sum(R.bound(*c.image.shape) for c in cases)
    assert b.segments == sum(len(L.facts(c.name)) for c in cases)
    for c, f in zip(cases, files):
        check_file(f, c.image, c.filter, c.order, c.name, L.reference(c.name))


def test_round_trip_through_the_projects_decoder(corpus):
    from attwarp_amd import png
    cases, tens, b, files = corpus
    pf = png.PngFiles(files, "keep", device=DEV)
    views, status = pf.run()
    assert status.cpu().tolist() == [0] * len(cases)
    for c, v in zip(cases, views):
        want = c.image[:, :, ::-1] if c.order == "bgr" and c.image.shape[2] == 3 else c.image       # the file's order
        assert tuple(v.shape) == want.shape and np.array_equal(v.cpu().numpy(), want), c.name


def test_guard_bytes_and_every_output_alignment(corpus):
    """The sub-batch of png_limit_cases.guard_batch() into a buffer that starts at each residue mod 4, buffer and scratch
    between guard bytes: the guards and the buffer's bytes behind the last file keep their 0xA5, the files are the same."""
    cases, tens, _, _ = corpus
    names = L.guard_batch()
    want = [L.reference(n) for n in names]
    addr = np.array(L.segment_addresses(names))
    seen = []
    for k in range(4):
        assert set(((addr + k) % 4).tolist()) == {0, 1, 2, 3}
        bound = sum(R.bound(*L.case(n).image.shape) for n in names)
        out = torch.full((GUARD + k + bound + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        b = batch_of(names, tens, out=out[GUARD + k:GUARD + k + bound])
        assert b.bound == bound and b.buffer.data_ptr() % 4 == (out.data_ptr() + k) % 4 and out.data_ptr() % 4 == 0
        n = b.scratch.numel()
        scr = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        b.scratch = scr[GUARD:GUARD + n]
        assert b.scratch.data_ptr() % 16 == 0
        buf, offsets = b.run()
        torch.cuda.synchronize()
        offs = offsets.cpu().tolist()
        assert offs == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        assert bool((out[:GUARD + k] == 0xA5).all()) and bool((out[GUARD + k + bound:] == 0xA5).all()), k
        assert bool((out[GUARD + k + offs[-1]:] == 0xA5).all()), k                 # nothing behind the last file
        assert bool((scr[:GUARD] == 0xA5).all()) and bool((scr[-GUARD:] == 0xA5).all()), k
        data = buf[:offs[-1]].cpu().numpy().tobytes()
        files = [data[a:e] for a, e in zip(offs[:-1], offs[1:])]
        for name, f, w in zip(names, files, want):
            same_bytes(f, w, (name, k))
        seen.append(files)
    assert all(s == seen[0] for s in seen[1:])


def test_neighbours_do_not_matter(corpus):
    """600 segments take three passes of the assemble kernel's carry loop; the images behind them have seg0 > 600."""
    from attwarp_amd import png
    cases, tens, _, _ = corpus
    big, small, after = "many_segments", "code15_exact", "every_match_length"
    want = {n: L.reference(n) for n in (big, small, after)}
    for names in ([big], [big, small, after], [small, after, big], [small, big, after]):
        b = batch_of(names, tens)
        files = png.download(*b.run())
        for n, f in zip(names, files):
            same_bytes(f, want[n], (n, names))
    assert png.download(*batch_of([after], tens).run())[0] == want[after]


def test_graph_replay_of_the_limit_batch(corpus):
    from attwarp_amd import png
    cases, tens, b, files = corpus                           # (the fixture's eager run came first)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.run()
    b.buffer.zero_()
    b.offsets.zero_()
    g.replay()
    torch.cuda.synchronize()
    again = png.download(b.buffer, b.offsets)
    for c, f in zip(cases, again):
        same_bytes(f, L.reference(c.name), c.name)
