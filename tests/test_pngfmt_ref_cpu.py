"""The restatement of the PNG decoder's formats path (tests/pngfmt_ref.py) against Pillow, and the corpus
(tests/pngfmt_cases.py) against itself: every case provably reaches the branch it is there for."""
import zlib

import numpy as np
import pytest

import pngdec_ref as D
import pngfmt_cases as C
import pngfmt_ref as F


@pytest.fixture(scope="module")
def decoded():
    """{name: {mode: (status, image)}} of every good file, computed once."""
    return {k.name: {m: F.decode(k.file, m)[:2] for m in ("RGB", "L", "keep")} for k in C.good()}


def test_restatement_equals_pillow_on_every_good_file(decoded):
    for k in C.good():
        for mode in ("RGB", "L"):
            st, img = decoded[k.name][mode]
            want = C.pillow(k.file, mode)
            assert st == D.OK and img.shape == want.shape and np.array_equal(img, want), (k.name, mode)


def test_keep_is_the_mode_with_the_files_channel_count(decoded):
    for k in C.good():
        same = "L" if k.ctype in (0, 4) else "RGB"                          # (a palette file gives its palette's three)
        assert np.array_equal(decoded[k.name]["keep"][1], decoded[k.name][same][1]), k.name
        assert np.array_equal(decoded[k.name]["keep"][1], C.pillow(k.file, "keep")), k.name
    k = next(k for k in C.good() if k.name == "palette_boundary")
    assert np.array_equal(F.decode(k.file, "RGB", "bgr")[1], C.pillow(k.file, "RGB")[:, :, ::-1])


def test_zlib_inflates_every_good_file_to_the_builders_bytes():
    for k in C.good():
        p = F.parse(k.file)
        got = zlib.decompress(p["stream"])
        assert len(got) == F.filt_bytes(k.W, k.H, k.ch, k.depth, k.lace), k.name
        if k.filtered is not None:
            assert got == k.filtered, k.name


def test_adam7_sizes_reach_empty_and_one_line_passes():
    assert F.passes(1, 1, 1) == [(0, 0, 8, 8, 1, 1)] + [(x, y, dx, dy, 0 if x else 1, 0 if y else 1) for x, y, dx, dy in F.ADAM7[1:]]
    assert [g[4:] for g in F.passes(9, 9, 1)] == [(2, 2), (1, 2), (3, 1), (2, 3), (5, 2), (4, 5), (9, 4)]
    assert [g[4:] for g in F.passes(8, 8, 1)] == [(1, 1), (1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (8, 4)]
    cases = C.adam7_sizes()
    assert len(cases) == 3 * 81 and {(k.W, k.H) for k in cases} == {(w, h) for w in range(1, 10) for h in range(1, 10)}
    empty = one_row = one_col = 0
    for k in cases:
        sizes = F.pass_sizes(k.W, k.H, k.ch, k.depth, 1)
        geo = F.passes(k.W, k.H, 1)
        for p, (x0, y0, dx, dy, w, h) in enumerate(geo):
            assert w == len(range(x0, k.W, dx)) and h == len(range(y0, k.H, dy))
            assert sizes[p] == (h * (1 + -(-w * k.ch * k.depth // 8)) if w and h else 0)
            empty += not (w and h)
            one_row += h == 1 and w > 0
            one_col += w == 1 and h > 0
        assert sum(sizes) == len(k.filtered)
        assert sum(w * h for *_, w, h in geo) == k.W * k.H                  # the passes tile the image
    assert empty > 300 and one_row > 300 and one_col > 300
    for p in range(1, 7):                                                  # every later pass is empty somewhere, present elsewhere
        sizes = [F.pass_sizes(k.W, k.H, k.ch, k.depth, 1)[p] for k in cases]
        assert min(sizes) == 0 and max(sizes) > 0


def test_subbyte_rows_have_tail_bits_of_ones_and_all_five_filters():
    cases = C.subbyte_tails()
    assert {(k.depth, k.ctype, k.W) for k in cases} == {(d, c, w) for d, n in ((1, 17), (2, 9), (4, 5)) for c in (0, 3) for w in range(1, n + 1)}
    tails = 0
    for k in cases:
        assert [k.types[(0, r)] for r in range(5)] == [0, 1, 2, 3, 4]
        spare = -k.W * k.depth % 8
        rows = C.pack(k.samples, k.depth)
        if spare:
            assert (rows[:, -1] & ((1 << spare) - 1) == (1 << spare) - 1).all(), k.name
            tails += 1
        assert np.array_equal(F.unpack(rows, k.W, 1, k.depth), k.samples)
    assert tails >= 2 * (15 + 6 + 2)


def test_filter_units_and_carry_rows():
    assert {F.unit_bytes(k.ch, k.depth) for k in C.filter_units()} == {2, 3, 4, 6, 8}
    assert {F.unit_bytes(F.CHANNELS[t], d) for t in F.DEPTHS for d in F.DEPTHS[t]} == {1, 2, 3, 4, 6, 8}
    for k in C.filter_units():
        assert {k.types[(0, r)] for r in range(6)} == {1, 3, 4} and k.W in (1, 2, 3)
    big = next(k for k in C.carries() if k.name == "carry_adam7_9x521")
    geo = F.passes(9, 521, 1)
    assert all(h >= 65 for *_, h in geo)
    for row in (63, 64, 65):
        assert {big.types[(p, row)] for p in range(7) if (p, row) in big.types} == {0, 1, 2, 3, 4}
    plain = [k for k in C.carries() if not k.lace]
    assert sorted({k.H for k in plain}) == [63, 64, 65, 129] and {(k.ctype, k.depth) for k in plain} == {(0, 1), (6, 16)}
    for row in (63, 64):
        assert len({k.types[(0, row)] for k in plain if k.H > row}) >= 4


def test_grey16_saturates_and_the_others_take_the_high_byte(decoded):
    v = np.array(C.GREY16).reshape(2, 5)
    assert np.array_equal(decoded["grey16_values"]["L"][1][:, :, 0], np.minimum(v, 255))
    assert decoded["grey16_values"]["L"][1][0, 4, 0] == 255 and decoded["grey16_values"]["L"][1][1, 2, 0] == 255      # 256, 0x8000
    assert np.array_equal(decoded["grey16_values_adam7"]["RGB"][1], np.repeat(np.minimum(v, 255)[:, :, None], 3, 2))
    assert np.array_equal(decoded["grey_alpha16_values"]["L"][1][:, :, 0], v >> 8)
    assert np.array_equal(decoded["grey2_ramp"]["L"][1].reshape(-1), np.arange(12) % 4 * 85)
    assert np.array_equal(decoded["grey4_ramp"]["L"][1].reshape(-1), np.arange(32) % 16 * 17)


def test_palette_cases(decoded):
    k = next(k for k in C.values() if k.name == "palette_short")
    img = decoded["palette_short"]["RGB"][1]
    assert (img[k.samples[:, :, 0] >= 3] == 0).all() and (k.samples >= 3).sum() == 4 and img[0, 1].any()
    pal = C.boundary_palette()
    assert np.array_equal(decoded["palette_boundary"]["RGB"][1].reshape(256, 3), pal)
    assert np.array_equal(decoded["palette_boundary"]["L"][1].reshape(256), D.luma(pal))
    assert b"tRNS" in next(k for k in C.values() if k.name == "palette_trns").file
    assert b"PLTE" in next(k for k in C.values() if k.name == "rgb_suggested_plte").file


def test_row_limit_files_stand_on_the_limit():
    for k in C.row_limits():
        assert F.row_bytes(k.W, k.ch, k.depth) == (D.MAX_ROW_BYTES if k.depth == 1 else D.MAX_ROW_BYTES - 7), k.name   # the widest
        assert F.row_bytes(k.W + 1, k.ch, k.depth) > D.MAX_ROW_BYTES and k.H == 2


def test_malformed_files_have_their_statuses():
    got = {n: D.STATUS_NAMES[F.decode(f)[0]] for n, f in C.malformed()}
    assert got == {"filter5_pass1": "E_FILTER", "filter5_pass4": "E_FILTER", "filter5_pass7": "E_FILTER",
                   "plain_stream_in_adam7_header": "E_UNDERFLOW", "adam7_stream_in_plain_header": "E_OVERFLOW",
                   "cut_in_pass6": "E_TRUNCATED", "filter7_grey1": "E_FILTER"}


def test_refusals_raise_by_their_words():
    from attwarp_amd import png
    for name, f, word in C.refused():
        with pytest.raises(ValueError, match=word):
            F.parse(f)
        with pytest.raises(ValueError, match=word):
            png.parse_png(f, 0, all_formats=True)


def test_parse_png_agrees_with_the_restatement_and_keeps_its_plain_result():
    from attwarp_amd import png
    for k in C.good():
        p = F.parse(k.file)
        W, H, ctype, spans, depth, lace, pal = png.parse_png(k.file, 3, all_formats=True)
        assert (W, H, ctype, depth, lace, pal) == (p["W"], p["H"], p["color_type"], p["depth"], p["interlace"], p["palette"]), k.name
        assert [bytes(k.file[o:o + n]) for o, n, _ in spans] == [c for c, _ in p["chunks"]]
        assert png.filtered_bytes(W, H, F.CHANNELS[ctype], depth, lace) == F.filt_bytes(W, H, F.CHANNELS[ctype], depth, lace)
        if (depth, lace) != (8, 0) or ctype == 3:
            word = "colour type" if depth == 8 and ctype == 3 else "interlace" if depth == 8 else "depth"
            with pytest.raises(ValueError, match=word):
                png.parse_png(k.file, 3)
        else:
            assert png.parse_png(k.file, 3) == (W, H, ctype, spans)
