"""GPU tests of the JPEG encoder's assembly at its limits (tests/jpegenc_limit_cases.py, each case proved on the CPU by
test_jpegenc_limits_ref_cpu.py): units shorter than a byte, images of more than 256 units, batches of more than 256 files,
the extreme shapes with noise, a full unit of every sampling at near-worst content, rows that start more than 2 GiB behind
the first.  Every file equals the restatement's byte for byte (which equals Pillow's), ``offsets`` are the files' lengths
summed, and this project's own decoder reads every file back to Pillow's pixels.  There is no tolerance anywhere."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpegenc_limit_cases as L
from test_jpegenc_gpu import DEV, keywords, same_bytes

pytestmark = pytest.mark.gpu

G = 64


def check_files(b, files, want, names):
    """Lengths against ``offsets``, the batch's bound and units against the restatement's, every file's bytes."""
    offs = b.offsets.cpu().numpy()
    assert offs[0] == 0 and (np.diff(offs) == [len(f) for f in want]).all() and offs[-1] <= b.bound
    for name, f, w in zip(names, files, want):
        same_bytes(f, w, name)


def check_decodes(files):
    from attwarp_amd import jpeg
    for f, t in zip(files, jpeg.decode_jpeg(files, "RGB", device=DEV)):
        assert np.array_equal(t.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB")))


def small_cases():
    return L.group("sub_byte") + L.group("scan_chunks") + L.group("near_worst")


@pytest.fixture(scope="module")
def small():
    """The sub-byte, scan-chunk and near-worst cases in ONE mixed JpegBatch."""
    from attwarp_amd import jpeg, png
    cases = small_cases()
    tens = [torch.from_numpy(c[1]).to(DEV) for c in cases]
    b = jpeg.JpegBatch(tens, **keywords(cases))
    files = png.download(*b.run())
    return cases, tens, b, files


def test_small_cases_in_one_batch_equal_the_restatement(small):
    cases, tens, b, files = small
    assert b.units == sum(L.measure(c[0])["units"] for c in cases) and b.bound == sum(L.plan(c[0])["bound"] for c in cases)
    check_files(b, files, [L.reference(c[0]) for c in cases], [c[0] for c in cases])


def test_own_decoder_reads_the_small_cases_to_pillows_pixels(small):
    check_decodes(small[3])


def test_sub_byte_cases_alone_first_last_and_in_the_middle(small):
    from attwarp_amd import jpeg
    cases, tens, b, files = small
    names = [c[0] for c in cases]
    others = [names.index(n) for n in ("chunk_257_420", "worst_444_48_blocks", "flat444_8x136")]
    for c in L.group("sub_byte"):
        i = names.index(c[0])
        for idx in ([i], [i] + others, others + [i], others[:2] + [i] + others[2:]):
            sub = [cases[k] for k in idx]
            got = jpeg.encode_jpeg([tens[k] for k in idx], **keywords(sub))
            for k, g in zip(idx, got):
                same_bytes(g, L.reference(names[k]), (c[0], idx))


@pytest.mark.parametrize("name", [c[0] for c in L.extreme()])
def test_extreme_shape_with_noise_in_a_batch_of_its_own(name):
    from attwarp_amd import jpeg, png
    case = L.case(name)
    b = jpeg.JpegBatch([torch.from_numpy(case[1]).to(DEV)], **keywords([case]))
    files = png.download(*b.run())
    assert b.units == L.measure(name)["units"] and b.bound == L.plan(name)["bound"]
    check_files(b, files, [L.reference(name)], [name])
    check_decodes(files)


@pytest.mark.parametrize("name", [c[0] for c in L.far_rows()])
def test_rows_that_start_above_two_gib(name):
    """A view of 60000 rows, 36000 bytes apart, inside one uninitialised device buffer: only the view is written."""
    from attwarp_amd import jpeg, png
    case = L.case(name)
    img = case[1]
    row = img.shape[1] * (3 if img.ndim == 3 else 1)
    store = torch.empty((L.FAR_H - 1) * L.FAR_PITCH + row, dtype=torch.uint8, device=DEV)
    assert store.numel() < 3 << 30
    view = store.as_strided(img.shape, (L.FAR_PITCH, 1) if img.ndim == 2 else (L.FAR_PITCH, 3, 1))
    view.copy_(torch.from_numpy(img).to(DEV))
    assert view[-1].data_ptr() - view.data_ptr() == (L.FAR_H - 1) * L.FAR_PITCH > 1 << 31
    b = jpeg.JpegBatch([view], **keywords([case]))
    files = png.download(*b.run())
    assert b.units == L.measure(name)["units"]
    check_files(b, files, [L.reference(name)], [name])
    check_decodes(files)


@pytest.mark.parametrize("n", L.BATCH_SIZES)
def test_batches_around_and_beyond_one_chunk_of_files(n):
    """255, 256, 257 and 600 files; the two that need a carry also with ``out`` and the scratch buffer between guard bytes."""
    from attwarp_amd import jpeg, png
    batch = L.batch(n)
    cases = [c for c, _ in batch]
    want = [p["file"] for _, p in batch]
    tens = [torch.from_numpy(c[1]).to(DEV) for c in cases]
    b = jpeg.JpegBatch(tens, **keywords(cases))
    files = png.download(*b.run())
    assert b.bound == sum(p["bound"] for _, p in batch) and b.units == sum(len(p["units"]) for _, p in batch)
    check_files(b, files, want, [c[0] for c in cases])
    check_decodes(files)
    if n > 256:
        store = torch.full((G + 1 + b.bound + G,), 0xA5, dtype=torch.uint8, device=DEV)
        jb = jpeg.JpegBatch(tens, out=store[G + 1:G + 1 + b.bound], **keywords(cases))
        ns = jb.scratch.numel()
        guarded = torch.full((256 + ns + 256,), 0x5A, dtype=torch.uint8, device=DEV)
        jb.scratch = guarded[256:256 + ns]
        got = png.download(*jb.run())
        check_files(jb, got, want, [c[0] for c in cases])
        used = int(jb.offsets[-1])
        assert used == sum(len(f) for f in want)
        assert bool((store[:G + 1] == 0xA5).all()) and bool((store[G + 1 + used:] == 0xA5).all())
        assert bool((guarded[:256] == 0x5A).all()) and bool((guarded[256 + ns:] == 0x5A).all())
