"""The wave route's restatement (tests/pngwave_ref.py) and its corpus (tests/pngwave_cases.py) on the CPU: every case named
in the corpus is there and is what its name says, from the file's own bytes; the restatement's bytes equal the serial
decode of tests/pngdec_ref.py on every accepted file; and at the defaults it accepts EVERY good file of both limit corpora
and of the new cases -- convergence within 64 rounds is proved, so no good file may fall back."""
import functools
import zlib

import pytest

import pngdec_cases as C
import pngdec_limit_cases as L
import pngdec_ref as D
import pngwave_cases as WC
import pngwave_ref as W


@functools.lru_cache(maxsize=None)
def restated(f, seg=W.SEGMENT_BYTES, mr=W.MAX_ROUNDS):
    return W.decode_file(f, seg, mr, force_serial=True)


@functools.lru_cache(maxsize=None)
def serial(f):
    p = D.parse(f)
    return D.decode_stream(p["stream"], p["H"] * (1 + p["W"] * D.CHANNELS[p["color_type"]]), force_serial=True)


def test_the_corpus_holds_every_named_case_and_each_decodes_to_its_bytes():
    cases = WC.good_cases()
    assert [k.name for k in cases] == WC.NAMES and len(set(WC.NAMES)) == len(WC.NAMES) == 46
    for k in cases:
        st, filt, _ = serial(k.file)
        assert st == D.OK and filt == k.filtered, k.name
        assert zlib.decompress(D.parse(k.file)["stream"]) == k.filtered, k.name
    assert {len(WC.case(f"size_mod16_{r}").filtered) % 16 for r in range(16)} == set(range(16))
    assert len(WC.case("ring_wraps_twice").filtered) > 2 * W.RING
    assert [n for n, _, _ in WC.malformed()] == WC.MALFORMED_NAMES
    (_, f, want), = WC.malformed()
    assert D.decode(f)[0] == want == D.E_DISTANCE and restated(f, 16)[1][2] == 0


def test_the_named_edges_are_where_the_names_say():
    info = lambda name, seg=16, mr=64: restated(WC.case(name).file, seg, mr)
    assert info("short_block")[1] == (1, 1, 1)
    assert info("blocks_70")[1][0] == 70                                  # a window per block: more blocks than lanes
    assert info("windows_2")[1][0] == 2 and info("windows_3")[1][0] == 3
    assert info("eob_ends_segment")[1][0] == 2 and info("eob_starts_segment")[1][0] == 2
    # segment k is right only after k rounds: rounds = segments = 64, and one round less must fall back
    assert info("out_of_phase_64")[1] == (1, 64, 1)
    out, i3, _ = info("out_of_phase_64", 16, 63)
    assert out is None and i3 == (1, 63, 0)
    # one match per lane, each copying the one before: resolution rounds = matches
    assert info("match_chain_64")[2] == 64 and info("match_chain_64")[1][2] == 1
    # a 256-byte segment of 1-bit codes: 2048 tokens per lane, four lanes fill the staging buffer
    out, i3, _ = info("one_bit_literals_256", 256)
    assert i3 == (1, 1, 1) and 20000 > W.STAGE and 2048 * 4 == W.STAGE
    s = D.parse(WC.case("matches_only_window").file)["stream"]
    r = D.inflate(s, 2, 1 << 20)
    assert len(s) > 2 * 1024 + 2 and r.seen == {(4, 1)}                    # more than two windows of stream, matches only
    for name, pair in (("dist32768_len3_wrap", (3, 32768)), ("dist32768_len258_wrap", (258, 32768)), ("stored_65535_then_dist32768", (10, 32768)),
                       ("len258_dist1_edge", (258, 1)), ("len258_dist2_edge", (258, 2)), ("len258_dist3_edge", (258, 3)),
                       ("reach_first_byte", (5, 5)), ("match_half_before_window", (6, 6))):
        s = D.parse(WC.case(name).file)["stream"]
        assert pair in D.inflate(s, 2, 1 << 20).seen, name
    assert "stored_65535" in WC.case("stored_65535_then_dist32768").features and "stored_len0_final" in WC.case("empty_final_stored").features
    assert {f"stored_at_bit{b}" for b in range(8)} <= set().union(*(WC.case(f"empty_stored_at_bit{b}").features for b in range(8)))
    assert any(t.startswith("len2") and t.endswith("_sym284") for t in WC.case("token48_edges").features)


def test_every_good_file_is_accepted_at_the_defaults_and_equals_the_serial_decode():
    files = [(n, f) for n, f, _ in L.limit_good()] + list(C.good()) + WC.good()
    assert len(L.limit_good()) == 263
    fell_back = []
    for name, f in files:
        out, (windows, rounds, accepted), _ = restated(f)
        if not accepted:
            fell_back.append(name)
            continue
        st, filt, _ = serial(f)
        assert st == D.OK and out == filt, name
        assert rounds <= 64 * windows
    assert fell_back == []                                               # the share of good files that may fall back is zero


@pytest.mark.parametrize("seg", [16, 256])
def test_other_segment_sizes_accept_the_new_cases_and_give_the_same_bytes(seg):
    for name, f in WC.good():
        out, i3, _ = restated(f, seg)
        assert i3[2] == 1 and out == WC.case(name).filtered, name


def test_malformed_files_are_never_accepted():
    bad = [(n, f) for n, f, _ in L.limit_malformed()] + [(n, f) for n, f, _ in C.malformed()] + [(n, f) for n, f, _ in WC.malformed()]
    for name, f in bad:
        assert D.decode(f)[0] != D.OK, name
        for seg in (16, 128):
            assert restated(f, seg)[1][2] == 0, (name, seg)
