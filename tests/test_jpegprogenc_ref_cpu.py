"""The restatement of the progressive files (tests/jpegprogenc_ref.py) against Pillow, and what the case list
(tests/jpegprogenc_cases.py) claims, on the CPU: the GPU test then only compares the kernels with the restatement."""
import io

import numpy as np
import pytest
from PIL import Image

import jpegprogenc_cases as C
import jpegprogenc_ref as P

NAMES = [c[0] for c in C.cases()]


def pillow(img, kw, **more):
    a = np.asarray(img)
    if a.ndim == 3 and kw.get("order") == "bgr":
        a = np.ascontiguousarray(a[:, :, ::-1])
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", **{**C.pillow_keywords(kw), **more})
    return f.getvalue()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pillow_and_the_expectations_hold(name):
    _, img, kw, expect = C.case(name)
    want = pillow(img, kw)
    got = C.reference(name)
    assert got == want, (name, len(got), len(want))
    assert pillow(img, kw, optimize=True) == want             # progressive forces the optimised tables
    m = C.measure(name)
    for key, value in expect.items():
        if key == "big":
            continue
        if key == "noticed_by":
            assert set(value) <= set(m[key]), (name, value, m[key])
        elif key.startswith("min_"):
            assert m[key[4:]] >= value, (name, key, m[key[4:]], value)
        else:
            assert m[key] == value, (name, key, m[key], value)
    H, W, nc, q, sub, rr = C.args_of(name)
    assert len(got) <= P.bound(H, W, nc, q, sub, rr), name
    interval, whole = C.bound_use(name)
    print(f"{name}: {len(got)} bytes, {whole:.3f} of the bound, the fullest interval {interval:.3f} of its own")
    assert interval <= 1.0, name
    ours, theirs = Image.open(io.BytesIO(got)), Image.open(io.BytesIO(want))
    assert np.array_equal(np.asarray(ours), np.asarray(theirs))


def test_every_defect_is_noticed_by_a_named_case():
    noticed = {d for _, _, _, e in C.cases() for d in e.get("noticed_by", [])}
    assert noticed == set(P.DEFECTS)
    for name, _, _, e in C.cases():
        for d in e.get("noticed_by", []):
            assert C.defect_file(name, d) != C.reference(name), (name, d)


def test_the_script_is_the_documented_one():
    assert len(P.script(3)) == 10 and len(P.script(1)) == 6
    assert [sc[0] for sc in P.script(3)][2:4] == [(2,), (1,)]     # Cr before Cb
    tables = lambda n: sum(len(P.scan_slots(sc, i)) for i, sc in enumerate(P.script(n)))
    assert tables(3) == 10 and tables(1) == 5
    info = C.info("restart_1")
    assert info["intervals"] == [4, 7, 4, 4, 7, 7, 4, 4, 4, 7] and info["dri"] == [4, 7, 4, 7, 4, 7]
    data = C.reference("restart_1")
    assert data.count(b"\xff\xc4") >= 10 and data[:2] == b"\xff\xd8" and b"\xff\xc2" in data and b"\xff\xc0" not in data[:600]


def test_the_bound_holds_for_the_near_worst_units():
    """How close the corpus comes to the bound, from the restatement (DESIGN.md 3.27 quotes the figures): the bound prices
    every symbol at 16 bits and every byte as stuffed, so random content stays far below it."""
    use = {n: C.bound_use(n) for n in NAMES if n.startswith("worst_")}
    print(use)
    assert all(0.0 < whole <= 1.0 and 0.0 < interval <= 1.0 for interval, whole in use.values()), use
