"""The JPEG encoder's restatement (tests/jpegenc_ref.py) against Pillow, without a GPU: for every case of
tests/jpegenc_cases.py the whole file equals ``Image.save``'s, Pillow's pixels of it equal the project's reference decoder's
(tests/jpegdec_ref.py), its length is within the bound, and every ``expect`` of the case holds."""
import io

import numpy as np
import pytest
from PIL import Image

import jpegdec_ref as D
import jpegenc_cases as K
import jpegenc_ref as R

NAMES = [c[0] for c in K.cases()]


def pillow_file(img, quality=75, subsampling="4:2:0", restart_rows=0, order="rgb"):
    a = np.asarray(img)
    if a.ndim == 3 and order == "bgr":
        a = a[:, :, ::-1]
    f = io.BytesIO()
    # a grey image has no chroma to sub-sample: the keyword stays unset, as in a bare save (given one, Pillow writes the
    # factors into the single component's SOF0 entry; the scan data is the same)
    sub = dict(subsampling=R.SUBSAMPLING_IDS[subsampling]) if a.ndim == 3 else {}
    Image.fromarray(np.ascontiguousarray(a)).save(f, "JPEG", quality=quality, restart_marker_rows=restart_rows, **sub)
    return f.getvalue()


def case(name):
    return next(c for c in K.cases() if c[0] == name)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pillow_whole_file(name):
    _, img, kw, expect = case(name)
    want, got = pillow_file(img, **kw), K.reference(name)
    assert got == want, (len(got), len(want), next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), -1))
    a = np.asarray(img)
    ncomp = 1 if a.ndim == 2 else a.shape[2]
    assert len(got) <= R.bound(a.shape[0], a.shape[1], ncomp, kw.get("quality", 75), kw.get("subsampling", "4:2:0"), kw.get("restart_rows", 0))
    m = K.measure(name)
    for k, v in expect.items():
        assert m[k] == v, (k, m[k], v)


@pytest.mark.parametrize("name", NAMES)
def test_pillow_and_the_reference_decoder_agree_on_the_file(name):
    data = K.reference(name)
    pil = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    status, pixels, _ = D.decode(data, "RGB")
    assert status == 0 and np.array_equal(pixels, pil)


def test_bare_save_is_quality_75_420_no_restarts():
    for seed, (h, w) in enumerate(((20, 20), (33, 47), (8, 8))):
        img = K.photo(h, w, 3, seed)
        f = io.BytesIO()
        Image.fromarray(img).save(f, "JPEG")
        assert f.getvalue() == R.encode(img) == R.encode(img, 75, "4:2:0", 0)
        g = io.BytesIO()
        Image.fromarray(img[:, :, 0]).save(g, "JPEG")
        assert g.getvalue() == R.encode(img[:, :, 0])


def test_corpus_reaches_what_it_claims():
    names = set(NAMES)
    for (h, w) in K.SIZES:
        for layout in K.LAYOUTS:
            assert f"{h}x{w}_{layout}" in names
    kws = [c[2] for c in K.cases()]
    assert {k.get("quality", 75) for k in kws} >= {1, 30, 75, 95, 100} and {k.get("restart_rows", 0) for k in kws} == {0, 1, 2}
    assert {k.get("order", "rgb") for k in kws} == {"rgb", "bgr"}
    used = K.symbols_used()
    # every symbol of all four tables: the DC categories 0 .. 11, and all 162 AC symbols of each table (the symbol grids of
    # the corpus supply the long runs before large values that photo-like content and noise do not reach)
    for t in range(4):
        assert {s for tt, s in used if tt == t} == set(R.TABLES[t][1]), (t, sorted(set(R.TABLES[t][1]) - {s for tt, s in used if tt == t}))
    assert (len(R.AC_LUMA[1]), len(R.AC_CHROMA[1])) == K.AC_SYMBOLS_USED == (162, 162)


def test_refusals_of_the_restatement():
    with pytest.raises(ValueError):
        R.encode(np.zeros((1, 65500), np.uint8), restart_rows=9)           # 9 x 8188 MCUs > 65535
    assert R.encode(np.zeros((1, 65500), np.uint8), restart_rows=8)[:2] == b"\xff\xd8"
    for bad in (dict(quality=0), dict(quality=101), dict(subsampling="4:1:1")):
        with pytest.raises(ValueError):
            R.encode(np.zeros((8, 8, 3), np.uint8), **bad)
    with pytest.raises(ValueError):
        R.encode(np.zeros((8, 8, 2), np.uint8))
    with pytest.raises(ValueError):
        R.encode(np.zeros((8, 65501), np.uint8))
