"""GPU tests of the JPEG encoder's progressive files (``progressive=True``; the jpegprogenc_* kernels of jpegenc.hip, DESIGN.md
3.27): every file equals the restatement of tests/jpegprogenc_ref.py byte for byte (which tests/test_jpegprogenc_ref_cpu.py
proves equal to Pillow's ``progressive=True`` files); plain, optimised and progressive images share a batch; this project's
own decoder reads the files to Pillow's pixels."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpegopt_ref as O
import jpegprogenc_cases as C
import jpegprogenc_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALSO = {"dummy_both_420": "plain", "restart_1": "optimize", "dummy_h40_grey": "plain", "worst_422": "optimize", "grey_1x1": "optimize"}
MODES = {"progressive": dict(optimize=False, progressive=True), "optimize": dict(optimize=True, progressive=False),
         "plain": dict(optimize=False, progressive=False)}


def same_bytes(got: bytes, want: bytes, what):
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(f"{what}: {len(got)} bytes against the restatement's {len(want)}, first difference at byte {first}")


def keywords(items):
    """items: [(case, mode)]"""
    return dict(quality=[c[2].get("quality", 75) for c, _ in items], subsampling=[c[2].get("subsampling", "4:2:0") for c, _ in items],
                restart_rows=[c[2].get("restart_rows", 0) for c, _ in items], order=[c[2].get("order", "rgb") for c, _ in items],
                optimize=[MODES[m]["optimize"] for _, m in items], progressive=[MODES[m]["progressive"] for _, m in items])


def want_file(item):
    c, mode = item
    return C.reference(c[0]) if mode == "progressive" else O.encode(c[1], optimize=mode == "optimize", **c[2])


@pytest.fixture(scope="module")
def corpus():
    """The small cases progressive, and the ALSO cases once more plain or optimised in between, in ONE JpegBatch."""
    from attwarp_amd import jpeg, png
    items = []
    for name in C.small_names():
        items.append((C.case(name), "progressive"))
        if name in ALSO:
            items.append((C.case(name), ALSO[name]))
    tens = [torch.from_numpy(c[1]).to(DEV) for c, _ in items]
    b = jpeg.JpegBatch(tens, **keywords(items))
    files = png.download(*b.run())
    return items, tens, b, files


def test_mixed_batch_equals_the_restatement(corpus):
    items, tens, b, files = corpus
    offs = b.offsets.cpu().numpy()
    assert offs[0] == 0 and (np.diff(offs) == [len(f) for f in files]).all() and offs[-1] <= b.bound
    assert sorted({m for _, m in items}) == ["optimize", "plain", "progressive"]
    total = 0
    for it, f in zip(items, files):
        same_bytes(f, want_file(it), (it[0][0], it[1]))
        H, W, nc, q, sub, rr = C.args_of(it[0][0])
        bd = P.bound(H, W, nc, q, sub, rr) if it[1] == "progressive" else O.bound(H, W, nc, q, sub, rr, optimize=it[1] == "optimize")
        assert len(f) <= bd
        total += bd
    assert b.bound == total


def test_progressive_implies_optimised_tables(corpus):
    from attwarp_amd import jpeg
    items, tens, b, files = corpus
    i = [c[0] for c, _ in items].index("restart_1")
    kw = {k: [v[i]] for k, v in keywords(items).items()}
    kw["optimize"] = [True]
    assert jpeg.encode_jpeg([tens[i]], **kw) == [files[i]]


def test_own_decoder_reads_every_file_to_pillows_pixels(corpus):
    from attwarp_amd import jpeg
    items, tens, b, files = corpus
    for (c, mode), f, t in zip(items, files, jpeg.decode_jpeg(files, "RGB", device=DEV, progressive=True)):
        a = c[1][:, :, ::-1] if (c[1].ndim == 3 and c[2].get("order") == "bgr") else c[1]
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(a)).save(buf, "JPEG", **{**C.pillow_keywords(c[2]), "progressive": mode == "progressive",
                                                                        "optimize": mode == "optimize"})
        assert np.array_equal(t.cpu().numpy(), np.asarray(Image.open(buf).convert("RGB"))), (c[0], mode)


@pytest.mark.parametrize("name", [n for n, _, _, e in C.cases() if e.get("big")])
def test_big_cases_in_batches_of_their_own(name):
    from attwarp_amd import jpeg
    c = C.case(name)
    got = jpeg.encode_jpeg([torch.from_numpy(c[1]).to(DEV)], progressive=True, **c[2])
    same_bytes(got[0], C.reference(name), name)
    m = C.measure(name)
    assert m["flush_7fff"] + m["flush_be"] >= 1 or m["max_depth"] > 16


def test_more_segments_than_one_chunk_of_the_place_scan():
    """A grey image 8 wide and 352 high with a restart per block row: 44 intervals in each of the six scans, 264 segments, so
    the prefix sums of jpegprogenc_place_kernel carry from their first chunk of 256 into a second."""
    from attwarp_amd import jpeg
    import jpegenc_cases as K
    img = K.noise(352, 8, 1, 77)
    assert sum(g[2] for g in P.scan_geometry(352, 8, 1, "4:2:0", 1)) == 264
    got = jpeg.encode_jpeg([torch.from_numpy(img).to(DEV)], progressive=True, restart_rows=1)
    same_bytes(got[0], P.encode(img, restart_rows=1), "264 segments")


def test_a_case_alone_first_last_and_in_the_middle(corpus):
    from attwarp_amd import jpeg
    items, tens, b, files = corpus
    names = [(c[0], m) for c, m in items]
    others = [names.index(n) for n in (("rgb", "progressive"), ("dummy_both_420", "plain"), ("grey_1x1", "optimize"))]
    for name in (("restart_1", "progressive"), ("refine_runs", "progressive"), ("worst_422", "optimize")):
        i = names.index(name)
        for idx in ([i], [i] + others, others + [i], others[:2] + [i] + others[2:]):
            got = jpeg.encode_jpeg([tens[k] for k in idx], **keywords([items[k] for k in idx]))
            for k, g in zip(idx, got):
                same_bytes(g, files[k], (name, idx))


def test_out_and_scratch_between_guards_at_every_residue(corpus):
    from attwarp_amd import jpeg, png
    items, tens, b, files = corpus
    names = [(c[0], m) for c, m in items]
    pick = [names.index(n) for n in (("rgb_1x1", "progressive"), ("dummy_both_420", "plain"), ("restart_1", "progressive"),
                                     ("worst_422", "optimize"), ("worst_420", "progressive"), ("rstn_wraps", "progressive"))]
    sub = [items[i] for i in pick]
    G = 64
    for r in range(4):
        probe = jpeg.JpegBatch([tens[i] for i in pick], **keywords(sub))
        store = torch.full((G + r + probe.bound + G,), 0xA5, dtype=torch.uint8, device=DEV)
        jb = jpeg.JpegBatch([tens[i] for i in pick], out=store[G + r:G + r + probe.bound], **keywords(sub))
        n = jb.scratch.numel()
        guarded = torch.full((256 + n + 256,), 0x5A, dtype=torch.uint8, device=DEV)
        jb.scratch = guarded[256:256 + n]
        assert jb.scratch.data_ptr() % 16 == 0
        got = png.download(*jb.run())
        for i, g in zip(pick, got):
            same_bytes(g, files[i], (names[i], r))
        used = int(jb.offsets[-1])
        host = store.cpu().numpy()
        assert (host[:G + r] == 0xA5).all() and (host[G + r + used:] == 0xA5).all()
        gh = guarded.cpu().numpy()
        assert (gh[:256] == 0x5A).all() and (gh[256 + n:] == 0x5A).all()


def test_run_twice_then_graph_replay_also_after_the_content_changed(corpus):
    from attwarp_amd import jpeg, png
    items, tens, whole, files = corpus
    whole.buffer.zero_()
    assert png.download(*whole.run()) == files                # the histograms are cleared by every run
    assert png.download(*whole.run()) == files
    names = [(c[0], m) for c, m in items]
    pick = [names.index(n) for n in (("rgb", "progressive"), ("restart_1", "optimize"), ("dummy_right_420", "progressive"),
                                     ("dummy_both_420", "plain"), ("restart_2", "progressive"))]
    mine = [tens[i].clone() for i in pick]
    sub = [items[i] for i in pick]
    b = jpeg.JpegBatch(mine, **keywords(sub))
    b.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.run()
    for _ in range(2):
        b.buffer.zero_()
        b.offsets.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert png.download(b.buffer, b.offsets) == [files[i] for i in pick]
    flipped = np.ascontiguousarray(items[pick[2]][0][1][::-1])                  # the sources are read, and counted, at every replay
    mine[2].copy_(torch.from_numpy(flipped))
    g.replay()
    torch.cuda.synchronize()
    got = png.download(b.buffer, b.offsets)
    assert got[2] == P.encode(flipped, **sub[2][0][2]) and got[2] != files[pick[2]]
    assert got[:2] == [files[i] for i in pick[:2]] and got[3:] == [files[i] for i in pick[3:]]


def test_keyword_forms_and_limits():
    from attwarp_amd import jpeg
    a = C.case("dummy_both_422")
    t = torch.from_numpy(a[1]).to(DEV)
    want = C.reference("dummy_both_422")
    kw = dict(a[2])
    assert jpeg.encode_jpeg([t, t], progressive=True, **kw) == [want, want]                      # one value for all
    assert jpeg.encode_jpeg(torch.stack([t, t]), progressive=[False, np.True_], **kw) == [O.encode(a[1], optimize=False, **kw), want]
    assert jpeg.JpegBatch([t], **kw).header.reserved == 0 and jpeg.JpegBatch([t], progressive=False, **kw).progressive == [False]
    for bad in (dict(progressive=1), dict(progressive="yes"), dict(progressive=[True, False]), dict(progressive=None)):
        with pytest.raises(ValueError):
            jpeg.JpegBatch([t], **bad)
    wide = torch.zeros((16, 65500, 3), dtype=torch.uint8, device=DEV)
    jpeg.JpegBatch([wide], restart_rows=9)
    with pytest.raises(ValueError, match="65535"):
        jpeg.JpegBatch([wide], restart_rows=9, progressive=True)


def test_write_jpeg_and_save_jpeg_ragged_take_the_keyword(tmp_path):
    from attwarp_amd import jpeg, pipeline
    import jpegenc_cases as K
    rng = np.random.default_rng(33)
    sizes = [(40, 50), (33, 61), (64, 48)]
    imgs = [K.photo(h, w, 3, 60 + i) for i, (h, w) in enumerate(sizes)]
    dimgs = pipeline.upload_images(imgs, DEV)
    m24 = torch.from_numpy((rng.random((3, 24, 24), dtype=np.float32) ** 3)).to(DEV)
    out, rb = pipeline.warp_from_masks_ragged(dimgs, m24, (32, 44), return_batch=True)
    for what, kw in (("warped", dict(progressive=True)), ("mota", dict(quality=90, restart_rows=1, progressive=True)),
                     ("warped", dict(subsampling="4:4:4", order="bgr", progressive=[True, False, True]))):
        paths = [str(tmp_path / f"{what}_{i}.jpg") for i in range(3)]
        pipeline.save_jpeg_ragged(rb, paths, what, **kw)
        flags = kw["progressive"] if isinstance(kw["progressive"], list) else [kw["progressive"]] * 3
        rest = {k: v for k, v in kw.items() if k != "progressive"}
        for i, p in enumerate(paths):
            want = out[i].cpu().numpy() if what == "warped" else rb.mota_of(i).cpu().numpy()
            same_bytes(open(p, "rb").read(), P.encode(want, **rest) if flags[i] else O.encode(want, optimize=False, **rest), p)
    p = str(tmp_path / "one.jpg")
    jpeg.write_jpeg([p], [dimgs[0]], restart_rows=1, progressive=True)
    same_bytes(open(p, "rb").read(), P.encode(imgs[0], restart_rows=1), p)
