"""The restatement of the scans-of-any-layout family (tests/jpegscan_ref.py) pinned to Pillow on the whole corpus of
tests/jpegscan_cases.py, the transcoder pinned to Pillow's reading of the one-scan source, the expected status of every
malformed file, and every refusal by its word, in the restatement and in ``parse_jpeg(..., all_scans=True)``.  No device."""
import numpy as np
import pytest

import jpegfmt_ref as F
import jpegscan_cases as C
import jpegscan_ref as R
from jpegdec_ref import STATUS_NAMES


def test_the_corpus_is_a_few_hundred_files_of_both_kinds_and_every_layout():
    good = C.good()
    assert 250 <= len(good) <= 500
    parsed = [R.parse(f) for _, f in good]
    assert sum(p["sequential"] for p in parsed) >= 100 and sum(not p["sequential"] for p in parsed) >= 150
    assert {p["color"] for p in parsed} == {"ycc", "rgb", "cmyk", "ycck"}
    assert max(sum(h * v for h, v in p["samp"]) for p in parsed) == 10 and max(len(p["scans"]) for p in parsed) == 64
    assert {tuple(map(tuple, p["samp"])) for p in parsed} >= {tuple(s) for _, s, _ in C.L.LAYOUTS}
    assert any(len(s["comps"]) not in (1, p["ncomp"]) for p in parsed for s in p["scans"])          # an interleaved subset
    assert any(len({s["ri"] for s in p["scans"]}) > 2 for p in parsed)                               # DRI changed and removed


@pytest.mark.parametrize("mode,order", [("RGB", "rgb"), ("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr")])
def test_restatement_equals_pillow_on_every_good_file(mode, order):
    for name, f in C.good():
        st, got, _ = R.decode(f, mode, order)
        assert st == 0, (name, STATUS_NAMES[st])
        want = F.pillow(f, mode)
        if order == "bgr":
            want = want[:, :, ::-1]
        assert got.shape == want.shape and np.array_equal(got, want), (name, mode, order)


def test_pillow_reads_a_transcoded_file_as_its_one_scan_source():
    for name, f, src in C.transcoded() + C.limits():
        assert np.array_equal(F.pillow(f, "keep"), F.pillow(src, "keep")), name


def test_the_restatement_finds_the_sources_coefficients_in_a_transcoded_file():
    """In the blocks that cover each component's true size: a scan of one component does not carry the padded ones."""
    for name, f, src in C.transcoded()[::7] + C.limits():
        want = R.source_planes(src)[1]
        p = R.parse(f)
        got = R.decode(f)[2]["planes"]
        for a, b, (dw, dh) in zip(got, want, F.geometry(p)["true"]):
            assert np.array_equal(a[:-(-dh // 8), :-(-dw // 8)], b[:-(-dh // 8), :-(-dw // 8)]), name


EXPECT = {"prog_dc_cut_0": "E_TRUNCATED", "prog_dc_cut_50": "E_TRUNCATED", "prog_dc_cut_90": "E_TRUNCATED", "prog_ac_cut_0": "E_TRUNCATED",
          "prog_ac_cut_50": "E_TRUNCATED", "prog_ac_cut_90": "E_TRUNCATED", "seq_cut_0": "E_TRUNCATED", "seq_cut_50": "E_TRUNCATED",
          "seq_cut_90": "E_TRUNCATED", "prog_bad_code_dc": "E_HUFFMAN", "prog_bad_code_ac": "E_HUFFMAN", "seq_bad_code": "E_HUFFMAN",
          "prog_rst_missing_in_scan_1": "E_RESTART", "prog_rst_wrong_index_in_scan_1": "E_RESTART", "seq_rst_missing_in_scan_1": "E_RESTART",
          "seq_rst_wrong_index_in_scan_1": "E_RESTART", "prog_run_past_se": "E_COEFF", "prog_refinement_of_size_2": "E_COEFF",
          "prog_no_eoi": "E_NO_EOI", "seq_no_eoi": "E_NO_EOI", "seq_ends_inside_scan_1_of_3": "E_TRUNCATED"}


def test_every_malformed_file_has_its_expected_status():
    got = {name: STATUS_NAMES[R.decode(f)[0]] for name, f in C.malformed()}
    assert got == EXPECT


def test_every_refusal_by_its_word_in_the_restatement_and_in_parse_jpeg():
    from attwarp_amd import jpeg
    for name, f, word in C.refused():
        with pytest.raises(ValueError, match=word):
            R.parse(f)
        with pytest.raises(ValueError, match=word):
            jpeg.parse_jpeg(f, all_scans=True)
