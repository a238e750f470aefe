"""The restatement of the optimised Huffman tables (tests/jpegopt_ref.py) against Pillow, and what the case list
(tests/jpegopt_cases.py) claims, on the CPU: the GPU test then only compares the kernels with the restatement."""
import io

import numpy as np
import pytest
from PIL import Image

import jpegenc_ref as R
import jpegopt_cases as C
import jpegopt_ref as O

NAMES = [c[0] for c in C.cases()]


def pillow(img, kw, optimize):
    a = np.asarray(img)
    if a.ndim == 3 and kw.get("order") == "bgr":
        a = np.ascontiguousarray(a[:, :, ::-1])
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", optimize=optimize, **C.pillow_keywords(kw))
    return f.getvalue()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pillow_and_the_expectations_hold(name):
    _, img, kw, expect = C.case(name)
    want = pillow(img, kw, True)
    got = C.reference(name)
    assert got == want, (name, len(got), len(want))
    m = C.measure(name)
    for key, value in expect.items():
        if key == "not_longer":
            assert len(want) <= len(pillow(img, kw, False)), name
        elif key == "noticed_by":
            assert set(value) <= set(m[key]), (name, value, m[key])
        else:
            assert m[key] == value, (name, key, m[key], value)
    a = np.asarray(img)
    H, W = a.shape[:2]
    args = (H, W, 1 if a.ndim == 2 else 3, kw.get("quality", 75), kw.get("subsampling", "4:2:0"), kw.get("restart_rows", 0))
    assert len(got) <= O.bound(*args), name
    assert 0 <= O.bound(*args) - R.bound(*args) - 2 * (m["blocks"] // 8) <= 2           # one more bit per block, every byte stuffed
    assert m["header_bytes"] <= len(R.header(H, W, args[2], args[3], args[4], 1 if args[5] else 0))
    assert O.encode(img, optimize=False, **kw) == pillow(img, kw, False)


def test_every_defect_is_noticed_by_a_named_case():
    noticed = {d for _, _, _, e in C.cases() for d in e.get("noticed_by", [])}
    assert noticed == set(O.DEFECTS)
    for name, _, _, e in C.cases():                           # (the expectations themselves are proven above)
        for d in e.get("noticed_by", []):
            assert C.defect_file(name, d) != C.reference(name), (name, d)


def test_limiter_images_are_the_documented_ones():
    assert C.limiter_copies(19) == [1, 2, 4, 7, 12, 20, 33, 54, 88, 143, 232, 376, 609, 986, 1596, 2583, 4180, 6764, 10945]
    assert sum(C.limiter_copies(17)) == 10926 and len(C.limiter_symbols()) >= 19
    for n in (17, 18, 19):
        info = {}
        bits, vals = O.optimal_table(np.bincount([0] * (sum(C.limiter_copies(n)) + (-sum(C.limiter_copies(n)) % 64)) +
                                                 [s for (s, _), k in zip(C.limiter_symbols(), C.limiter_copies(n)) for _ in range(k)],
                                                 minlength=256), info=info)
        assert info["depth"] == n + 1 and max(k + 1 for k in range(16) if bits[k]) == 16 and len(vals) == n + 1
        assert O.kraft_gap(bits) == 1                         # complete but for the reserved code


def test_tables_are_valid_prefix_codes_beyond_libjpeg():
    """The table builder's own histograms: every one gives a complete code (but for the reserved all-ones code) of at most 16
    bits that lists every counted symbol once; the deepest, 39 levels (libjpeg's bits[33] overflows there), included."""
    depths = {}
    for name, hist, _ in C.table_histograms():
        info = {}
        bits, vals = O.optimal_table(hist, info=info)
        depths[name] = info["depth"]
        assert sorted(vals) == np.flatnonzero(hist).tolist() and sum(bits) == len(vals), name
        assert O.kraft_gap(bits) == 1, name
    assert depths["depth_20"] == 20 and depths["depth_39"] == 39 and depths["one_symbol"] == 1 and depths["equal_256"] == 9
