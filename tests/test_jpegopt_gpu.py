"""GPU tests of the JPEG encoder's optimised Huffman tables (``optimize=True``; the jpegopt_* kernels of jpegenc.hip, DESIGN.md
3.26): every file equals the restatement of tests/jpegopt_ref.py byte for byte (which tests/test_jpegopt_ref_cpu.py proves equal
to Pillow's ``optimize=True`` files), images with and without the keyword share a batch, and the clear of the histograms is
part of every run."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpegopt_cases as C
import jpegopt_ref as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PLAIN = ("dummy_both", "restart_2", "symbols_chroma_q100", "worst_420", "grey_1x1")      # cases the mixed batch also holds WITHOUT the keyword


def same_bytes(got: bytes, want: bytes, what):
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(f"{what}: {len(got)} bytes against the restatement's {len(want)}, first difference at byte {first}")


def keywords(items):
    """items: [(case, optimize)]"""
    return dict(quality=[c[2].get("quality", 75) for c, _ in items], subsampling=[c[2].get("subsampling", "4:2:0") for c, _ in items],
                restart_rows=[c[2].get("restart_rows", 0) for c, _ in items], order=[c[2].get("order", "rgb") for c, _ in items],
                optimize=[o for _, o in items])


def want_file(item):
    return C.reference(item[0][0], item[1])


@pytest.fixture(scope="module")
def corpus():
    """The whole corpus optimised, and the PLAIN cases once more without the keyword in between, in ONE JpegBatch."""
    from attwarp_amd import jpeg, png
    items = []
    for c in C.cases():
        items.append((c, True))
        if c[0] in PLAIN:
            items.append((c, False))
    tens = [torch.from_numpy(c[1]).to(DEV) for c, _ in items]
    b = jpeg.JpegBatch(tens, **keywords(items))
    files = png.download(*b.run())
    return items, tens, b, files


def test_mixed_batch_equals_the_restatement(corpus):
    items, tens, b, files = corpus
    offs = b.offsets.cpu().numpy()
    assert offs[0] == 0 and (np.diff(offs) == [len(f) for f in files]).all() and offs[-1] <= b.bound
    bounds = [O.bound(*(c[1].shape[:2]), 1 if c[1].ndim == 2 else 3, c[2].get("quality", 75), c[2].get("subsampling", "4:2:0"),
                      c[2].get("restart_rows", 0), optimize=o) for c, o in items]
    assert b.bound == sum(bounds) and max(tuple(c[1].shape[:2]) for c, _ in items) == (3584, 512)
    for it, f, bd in zip(items, files, bounds):
        same_bytes(f, want_file(it), (it[0][0], it[1]))
        assert len(f) <= bd


def test_plain_files_of_the_mixed_batch_equal_a_batch_without_the_keyword(corpus):
    from attwarp_amd import jpeg
    items, tens, b, files = corpus
    idx = [i for i, (_, o) in enumerate(items) if not o]
    assert [items[i][0][0] for i in idx] == [c[0] for c in C.cases() if c[0] in PLAIN]
    kw = keywords([items[i] for i in idx])
    del kw["optimize"]
    assert jpeg.encode_jpeg([tens[i] for i in idx], **kw) == [files[i] for i in idx]
    assert jpeg.encode_jpeg([tens[i] for i in idx], optimize=False, **kw) == [files[i] for i in idx]
    plain = jpeg.JpegBatch([tens[i] for i in idx], **kw)
    assert plain.header.off_optimize == 0 and plain.optimize == [False] * len(idx)


def test_own_decoder_reads_every_file_to_pillows_pixels(corpus):
    from attwarp_amd import jpeg
    items, tens, b, files = corpus
    for f, t in zip(files, jpeg.decode_jpeg(files, "RGB", device=DEV)):
        assert np.array_equal(t.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB")))


def test_a_case_alone_first_last_and_in_the_middle(corpus):
    from attwarp_amd import jpeg
    items, tens, b, files = corpus
    names = [(c[0], o) for c, o in items]
    others = [names.index(n) for n in (("rgb", True), ("dummy_both", False), ("grey_1x1", True))]
    for name in (("restart_1", True), ("limiter_18", True), ("worst_420", False), ("flat_rgb_16", True)):
        i = names.index(name)
        for idx in ([i], [i] + others, others + [i], others[:2] + [i] + others[2:]):
            got = jpeg.encode_jpeg([tens[k] for k in idx], **keywords([items[k] for k in idx]))
            for k, g in zip(idx, got):
                same_bytes(g, files[k], (name, idx))


def test_out_and_scratch_between_guards_at_every_residue(corpus):
    from attwarp_amd import jpeg, png
    items, tens, b, files = corpus
    names = [(c[0], o) for c, o in items]
    pick = [names.index(n) for n in (("column_17x1", True), ("dummy_both", False), ("restart_1", True), ("symbols_luma_q100", True), ("worst_422", True))]
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


def test_run_twice_gives_the_same_bytes(corpus):
    """The histograms are cleared by every run: a second run does not add to the first one's counts."""
    from attwarp_amd import png
    items, tens, b, files = corpus
    b.buffer.zero_()
    assert png.download(*b.run()) == files
    assert png.download(*b.run()) == files


def test_graph_replay_also_after_the_content_changed(corpus):
    from attwarp_amd import jpeg, png
    items, tens, _, files = corpus
    names = [(c[0], o) for c, o in items]
    pick = [names.index(n) for n in (("rgb", True), ("restart_2", False), ("dummy_right", True), ("restart_2", True), ("tie", True))]
    mine = [tens[i].clone() for i in pick]
    sub = [items[i] for i in pick]
    b = jpeg.JpegBatch(mine, **keywords(sub))
    b.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.run()
    for _ in range(2):                                        # a replay that added to the last run's counts would differ
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
    assert got[2] == O.encode(flipped, **sub[2][0][2]) and got[2] != files[pick[2]]
    assert got[:2] == [files[i] for i in pick[:2]] and got[3:] == [files[i] for i in pick[3:]]


def test_keyword_forms_and_limits():
    from attwarp_amd import jpeg
    a = C.case("dummy_422")
    t = torch.from_numpy(a[1]).to(DEV)
    want = C.reference("dummy_422")
    kw = {k: v for k, v in a[2].items()}
    assert jpeg.encode_jpeg([t, t], optimize=True, **kw) == [want, want]                         # one value for all
    assert jpeg.encode_jpeg(torch.stack([t, t]), optimize=[False, np.True_], **kw) == [C.reference("dummy_422", False), want]
    for bad in (dict(optimize=1), dict(optimize="yes"), dict(optimize=[True, False]), dict(optimize=None)):
        with pytest.raises(ValueError):
            jpeg.JpegBatch([t], **bad)


def test_save_jpeg_ragged_optimize(tmp_path):
    from attwarp_amd import pipeline
    import jpegenc_cases as K
    rng = np.random.default_rng(32)
    sizes = [(40, 50), (33, 61), (64, 48)]
    imgs = [K.photo(h, w, 3, 50 + i) for i, (h, w) in enumerate(sizes)]
    dimgs = pipeline.upload_images(imgs, DEV)
    m24 = torch.from_numpy((rng.random((3, 24, 24), dtype=np.float32) ** 3)).to(DEV)
    out, rb = pipeline.warp_from_masks_ragged(dimgs, m24, (32, 44), return_batch=True)
    for what, kw in (("warped", dict(optimize=True)), ("mota", dict(quality=90, restart_rows=1, optimize=True)),
                     ("warped", dict(subsampling="4:4:4", order="bgr", optimize=[True, False, True]))):
        paths = [str(tmp_path / f"{what}_{i}.jpg") for i in range(3)]
        pipeline.save_jpeg_ragged(rb, paths, what, **kw)
        flags = kw["optimize"] if isinstance(kw["optimize"], list) else [kw["optimize"]] * 3
        rest = {k: v for k, v in kw.items() if k != "optimize"}
        for i, p in enumerate(paths):
            want = out[i].cpu().numpy() if what == "warped" else rb.mota_of(i).cpu().numpy()
            same_bytes(open(p, "rb").read(), O.encode(want, optimize=flags[i], **rest), p)


def test_table_kernel_on_given_histograms():
    """jpegopt_tables_kernel alone over the host test's histograms, the one 39 levels deep included: the tuning flavour's
    ``jpegopt_given_hist`` makes attwarp_jpegenc_encode skip the clear and the count, so the tables come from the counts this
    test leaves in the scratch buffer (two per grey image).  The files of such a run mean nothing and are not looked at."""
    from attwarp_amd import _lib, jpeg
    hists = C.table_histograms()
    assert len(hists) % 2 == 0
    nimg = len(hists) // 2
    tens = [torch.full((8, 8), 128, dtype=torch.uint8, device=DEV) for _ in range(nimg)]
    b = jpeg.JpegBatch(tens, optimize=True)
    plan = b.table_host[int(b.header.off_optimize):]
    assert plan[:8].view(np.int32).tolist() == [nimg, nimg]
    off_hist, off_out = (int(v) for v in plan[8:24].view(np.uint64))
    given = np.zeros((nimg, 4, 256), np.uint32)
    given[:, :2] = np.stack([h for _, h, _ in hists]).reshape(nimg, 2, 256)
    b.scratch[off_hist:off_hist + given.nbytes].copy_(torch.from_numpy(given.view(np.uint8).reshape(-1)))
    with _lib.debug_override(jpegopt_given_hist=1):
        b.run()
        torch.cuda.synchronize()
    rec = b.scratch[off_out:off_out + nimg * 5928].cpu().numpy().reshape(nimg, 5928)
    for i, (name, hist, _) in enumerate(hists):
        t = rec[i // 2, 1320 * (i % 2):1320 * (i % 2 + 1)]
        info = {}
        bits, vals = O.optimal_table(hist, info=info)
        dht_len, depth, nsym = t[1024 + 280:1024 + 292].view(np.int32).tolist()
        assert (dht_len, depth, nsym) == (21 + len(vals), info["depth"], len(vals)), name
        assert t[1024:1024 + dht_len].tobytes() == O.dht_segment((i % 2) << 4, bits, vals), name
        assert t[:1024].view(np.uint32).tolist() == O.code_words(bits, vals), name
        assert O.kraft_gap(bits) == 1 and info["depth"] == (39 if name == "depth_39" else info["depth"])
    assert ctypes.sizeof(_lib.JpegEncHeader) == 80
