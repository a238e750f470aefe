"""The restatement of the JPEG decoder's layout family (tests/jpegfmt_ref.py) pinned to Pillow, bit for bit, on every file of
tests/jpegfmt_cases.py, before any GPU test leans on it: RGB, L and the file's own channels (Pillow's CMYK bytes for four
components).  Also what the corpus must contain for the other tests to mean anything."""
import numpy as np
import pytest

import jpegdec_cases as C
import jpegdec_ref as D
import jpegfmt_cases as F
import jpegfmt_ref as R

GOOD = F.good()


@pytest.mark.parametrize("name,f", GOOD, ids=[n for n, _ in GOOD])
def test_restatement_equals_pillow(name, f):
    for mode in ("RGB", "L", "keep"):
        st, px, _ = R.decode(f, mode)
        assert st == D.OK, (name, D.STATUS_NAMES[st])
        want = R.pillow(f, mode)
        assert px.shape == want.shape and px.dtype == np.uint8, (name, mode, px.shape, want.shape)
        assert np.array_equal(px, want), (name, mode, int((px != want).sum()))
    st, bgr, _ = R.decode(f, "RGB", "bgr")
    assert np.array_equal(bgr, R.pillow(f, "RGB")[:, :, ::-1])


def test_the_restatement_agrees_with_the_baseline_one_on_plain_files():
    for name in ("noise_17x33_s2", "blocky_40x31_s1", "grey_17x15", "ri_1", "edge_1x2_s1"):
        f = C.good_file(name)
        for mode in ("RGB", "L", "keep"):
            a, b = R.decode(f, mode), D.decode(f, mode)
            assert a[0] == b[0] == D.OK and np.array_equal(a[1], b[1]) and a[2]["crc"] == b[2]["crc"], (name, mode)


def test_corpus_covers_every_up_sampler_colour_rule_and_edge():
    seen, colors, slots = set(), set(), set()
    for name, f in GOOD:
        p = R.parse(f)
        g = R.geometry(p)
        colors.add(p["color"])
        slots.add(len(g["slots"]))
        for (h, v), (dw, dh) in zip(p["samp"], g["true"]):
            rx, ry = g["hmax"] // h, g["vmax"] // v
            seen.add((R.upsampler(rx, ry, dw), min(dw, 3), min(dh, 3)))
    assert colors == {"ycc", "rgb", "cmyk", "ycck"}          # (grey files are the baseline family's)
    assert 10 in slots and {(8 * max(h for h, _ in s), 8 * max(v for _, v in s)) for _, s, _ in F.LAYOUTS} >= {(32, 16), (8, 32)}
    for how in ("h2v1", "h2v2"):                              # only wider than two samples; one and two are replicated
        assert {(how, 3, 1), (how, 3, 2)} <= seen and not any(s[0] == how and s[1] < 3 for s in seen)
    for dh in (1, 2, 3):                                      # the vertical filter's edges are rows; no width switches it
        assert any(s[0] == "h1v2" and s[2] == dh for s in seen), dh
        for dw in (1, 2, 3):
            assert ("box", dw, dh) in seen, (dw, dh)


def test_malformed_files_carry_every_status():
    got = {R.decode(f)[0] for _, f in F.malformed()}
    assert got >= {D.E_TRUNCATED, D.E_HUFFMAN, D.E_RESTART, D.E_NO_EOI}, got
    assert all(R.decode(f)[0] != D.OK for _, f in F.malformed())


def test_long_files_span_several_segments_without_markers():
    for name, f in F.long_plain():
        p = R.parse(f)
        assert p["ri"] == 0 and 4 * 256 <= len(p["stream"]) <= 48 << 10, (name, len(p["stream"]))
