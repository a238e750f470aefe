"""CPU proofs about the PNG decoder's limit corpus (tests/pngdec_limit_cases.py): from the bytes, every good file inflates
with zlib to the filtered bytes its builder states and decodes in the restatement (tests/pngdec_ref.py) to Pillow's pixels;
every malformed file has its stated status and zlib refuses it too; the corpus holds every named case, every code length
on both trees, every residue of the length and both routes; the marker scan keeps the positions the builders wrote out.

The two row-limit files (65 rows of 49152 and of 49149 bytes) are checked against zlib and Pillow and their sync points are counted;
the restatement's inflate and filters are NOT run over them (3.2 MB each, symbol by symbol in Python)."""
import zlib

import numpy as np
import pytest

import pngdec_cases as C
import pngdec_limit_cases as L
import pngdec_ref as D

REQUIRED = (["lit15", "dist15", "lit_10_11", "dist_8_9", "hlit286_hdist30", "hlit286", "hdist30", "hlit257_hdist1_nodist", "hlit257",
             "hdist1", "nodist", "single_dist", "eob_only_then_block", "eob_only",
             "rep16_3", "rep16_6", "rep17_3", "rep17_10", "rep18_11", "rep18_138", "rep_across_border", "rep16_across_border",
             "rep18_across_border", "len258_sym285", "len258_sym284_31", "len3_dist32768", "len258_dist32768", "overlap_d2",
             "overlap_d3", "overlap_d4", "len258_dist2", "len258_dist3", "len258_dist4", "stored_len0_final", "stored_65535",
             "reach_exact", "reach_one_more", "scan_tail", "scan_tail_k1", "scan_tail_k2", "scan_tail_k3", "scan_cap_second_tile", "idat_empty_first_mid_last",
             "idat_all_empty_but_one", "avg_row64_c3", "rowmax_c1", "rowmax_c4", "seeded"] +
            [f"stored_at_bit{b}" for b in range(8)] + [f"tail_{j}" for j in range(12)] + [f"scan_k{k}" for k in range(8)] +
            [f"scan_tile_{o}" for o in range(2046, 2051)] + [f"scan_tile_true_{o}" for o in range(2046, 2051)] +
            [f"idat_len_{n}" for n in (255, 256, 257, 511, 512, 513)] +
            [f"carry_c{ch}_s{s}" for ch in (1, 2, 4) for s in range(5)] + [f"row64_filter{t}" for t in range(5)] +
            [f"carry_h{H}_w{W}" for H in (63, 64, 65, 127, 128) for W in (1, 2)])
MALFORMED = (["rep_past_total", "rep16_first", "hlit287", "hlit288", "hdist31", "hdist32", "no_eob", "lit_incomplete", "dist_incomplete",
              "hclen4_all_zero", "single_dist_other_bit", "dist_symbol_30", "cut_len_extra", "cut_dist_extra", "cut_code_lengths",
              "cut_stored_header", "cut_stored_payload", "overflow_by_match", "overflow_by_stored", "broken_second_unit", "filter5_row64",
              "filter5_row0_of_h129", "crc_flip_first", "crc_flip_last", "crc_wrong_on_empty_chunk", "scan_trunc_plus1", "scan_trunc_plus0"] +
             [f"adler_short_{j}" for j in range(4)] + [f"adler_byte{j}" for j in range(4)])


@pytest.fixture(scope="module")
def decoded():
    """{name: (status, RGB image, info)} of every good limit file but the row-limit ones, computed once."""
    return {n: D.decode(f, "RGB") for n, f, _ in L.limit_good()}


def test_every_good_file_equals_zlib_and_pillow(decoded):
    files = L.limit_good()
    assert len(files) >= 200 and len({n for n, _, _ in files}) == len(files)
    for name, f, _ in files:
        p = D.parse(f)
        filt = zlib.decompress(p["stream"])
        assert filt == L.filtered_of(name), name
        st, img, info = decoded[name]
        assert st == D.OK, (name, D.STATUS_NAMES[st])
        assert info["adler"] == zlib.adler32(filt), name
        assert np.array_equal(img, C.pillow(f, "RGB")), name
    sample = files[::7] + [x for x in files if x[0] in ("carry_c2_s1", "avg_row64_c3", "carry_c4_s2")]   # (every colour type)
    for name, f, _ in sample:
        for mode, order in (("L", "rgb"), ("keep", "rgb"), ("RGB", "bgr")):
            st, img, _ = D.decode(f, mode, order)
            want = C.pillow(f, mode)
            assert st == D.OK and np.array_equal(img, want[:, :, ::-1] if order == "bgr" else want), (name, mode)
    assert {D.parse(f)["color_type"] for _, f, _ in sample} == {0, 2, 4, 6}


def test_row_limit_files_equal_zlib_and_pillow():
    for k in L.limit_rowmax():
        p = D.parse(k.file)
        rb = 1 + p["W"] * D.CHANNELS[p["color_type"]]
        assert rb == {"rowmax_c1": D.MAX_ROW_BYTES, "rowmax_c4": D.MAX_ROW_BYTES - 3}[k.name] and p["H"] == 65
        assert zlib.decompress(p["stream"]) == k.filtered and len(k.filtered) == 65 * rb
        kept = D.find_markers(p["stream"])
        assert len(kept) == k.expect["nkept"] == k.expect["chain"] == 65
        # every kept position is a true boundary: the rest of the stream inflates from there, one row per sync point
        for i, at in enumerate(kept[1:], 1):
            d = zlib.decompressobj(-15)
            assert d.decompress(p["stream"][at:-4]) == k.filtered[i * rb:], (k.name, i)
        # Pillow reads the image the builder filtered (alpha dropped)
        assert np.array_equal(C.pillow(k.file, "keep"), k.expect["image"][:, :, :3])


def test_every_malformed_file_has_its_status_and_zlib_refuses_it():
    bad = L.limit_malformed()
    assert sorted(n for n, _, _ in bad) == sorted(MALFORMED)
    for name, f, want in bad:
        st, img, info = D.decode(f)
        assert st != D.OK and img is None, name
        if want is not None:
            assert st == want, (name, D.STATUS_NAMES[st])
        p = D.parse(f)
        if st not in (D.E_CRC, D.E_FILTER):                   # zlib itself rejects the rest, or gives another size
            try:
                assert len(zlib.decompress(p["stream"])) != p["H"] * (1 + p["W"] * D.CHANNELS[p["color_type"]]), name
            except zlib.error:
                pass
    info = {n: D.decode(f)[2] for n, f, _ in bad}
    assert info["broken_second_unit"]["route"] == "serial" and info["broken_second_unit"]["nunits"] == 2
    assert info["scan_trunc_plus1"]["nunits"] == info["scan_trunc_plus0"]["nunits"] + 1 == 2
    files = {n: f for n, f, _ in bad}
    # the CRC is all that is wrong with the third file; the two flipped ones are broken behind it as well
    assert D.decode(files["crc_wrong_on_empty_chunk"], check_crc=False)[0] == D.OK
    assert D.decode(files["crc_flip_first"], check_crc=False)[0] == D.E_ZLIB_HEADER
    assert D.decode(files["crc_flip_last"], check_crc=False)[0] != D.OK
    assert [len(c) for c, _ in D.parse(files["crc_flip_last"])["chunks"]][0] == 257
    # the bad filter byte of filter5_row64 stands in the second batch of 64 rows
    for name, row in (("filter5_row64", 64), ("filter5_row0_of_h129", 0)):
        filt = zlib.decompress(D.parse(files[name])["stream"])
        assert [r for r in range(129) if filt[r * 22] > 4] == [row]


def test_the_corpus_holds_every_named_case_and_every_condition(decoded):
    good = L.limit_good()
    tags = set().union(*[t for _, _, t in good], *[k.features for k in L.limit_rowmax()])
    assert not [t for t in REQUIRED if t not in tags]
    seeds = L.seeded()
    assert len(seeds) == L.SEEDED == 160
    lit, dist, mods, routes = set(), set(), set(), {"unit": 0, "serial": 0}
    for name, k, info in seeds:
        p = D.parse(k.file)
        assert 2 <= len(k.filtered) <= 4096 and info["mod16"] == len(k.filtered) % 16
        # what the generator recorded is what the restatement's token walk meets
        r = D.inflate(p["stream"], 2, len(k.filtered))
        assert r.status == D.OK and r.lit_lens == info["lit_used"] and r.dist_lens == info["dist_used"], name
        assert info["lit_max"] == max(r.lit_lens) and info["dist_max"] == max(r.dist_lens, default=0)
        assert p["stream"].count(C.MARKER) >= (info["blocks"] - 1) * info["sync"]
        lit |= r.lit_lens
        dist |= r.dist_lens
        mods.add(info["mod16"])
        routes[decoded[name][2]["route"]] += 1
    assert lit == set(range(1, 16)) and dist == set(range(1, 16))
    assert mods == set(range(16))
    assert routes["unit"] >= 20 and routes["serial"] >= 20, routes


def test_named_cases_hold_what_their_names_promise(decoded):
    walk = lambda n: D.inflate(D.parse(L.case(n).file)["stream"], 2, len(L.filtered_of(n)))
    r = walk("lit15")
    assert 15 in r.lit_lens and (258, 7) in r.seen and r.lit_lens == set(range(1, 13)) | {14, 15}
    r = walk("dist15")
    assert r.dist_lens == set(range(1, 16)) and max(d for _, d in r.seen) >= 24577 and min(d for _, d in r.seen) == 1
    assert {10, 11} <= walk("lit_10_11").lit_lens and walk("dist_8_9").dist_lens == {1, 2, 3, 4, 5, 6, 8, 9}
    assert walk("len258_sym285").seen == {(258, 31)} and walk("len258_sym284_31").seen == {(258, 31), (258, 9)}
    assert L.case("len258_sym285").file != L.case("len258_sym284_31").file
    for d in (2, 3, 4):
        assert walk(f"overlap_d{d}").seen == {(258, d)}
    for first in (3, 258):
        r = walk(f"len{first}_dist32768")
        assert (first, 32768) in r.seen and {d for _, d in r.seen} == {32768}
    # stored blocks at every bit offset; tails: the last Huffman block of tail_j holds j + 1 literals
    for b in range(8):
        s = D.parse(L.case(f"stored_at_bit{b}").file)["stream"]
        assert len(L.filtered_of(f"stored_at_bit{b}")) == 1 + (b - 2) % 8 + 40 and s[2] & 7 == 2
    lens = [len(D.parse(L.case(f"tail_{j}").file)["stream"]) for j in range(12)]
    assert [b - a for a, b in zip(lens, lens[1:])] == [1] * 11
    # the unit border: one distance apart, one route apart
    a, b = decoded["reach_exact"][2], decoded["reach_one_more"][2]
    assert (a["route"], a["chain"], a["nunits"]) == ("unit", 2, 2) and (b["route"], b["chain"], b["nunits"]) == ("serial", 0, 2)
    sa, sb = D.parse(L.case("reach_exact").file)["stream"], D.parse(L.case("reach_one_more").file)["stream"]
    ka = D.find_markers(sa)
    ua, ub = D.inflate(sa, ka[1], 4096, set(ka), write=False), D.inflate(sb, ka[1], 4096, set(ka), write=False)
    assert (ua.dependent, ub.dependent) == (0, 1) and ua.seen == {(40, 9)} and ub.seen == {(40, 10)}
    for k in L.good_cases():
        _, _, info = decoded[k.name]
        for key, got in (("route", info["route"]), ("chain", info["chain"]), ("nkept", info["nunits"])):
            assert k.expect.get(key, got) == got, (k.name, key)
    # chunks: the lengths the names promise, empty ones included
    lens = lambda n: [len(c) for c, _ in D.parse(L.case(n).file)["chunks"]]
    assert lens("idat_empty_first_mid_last")[::2] == [0, 0, 0] and lens("idat_all_empty_but_one").count(0) == 4
    for n in (255, 256, 257, 511, 512, 513):
        assert lens(f"idat_len_{n}")[0] == n and len(lens(f"idat_len_{n}")) == 2
    # carry: taller than one batch of 64 rows, every filter type on rows 63, 64 and 128 for every channel count
    for ch in (1, 2, 4):
        on = {r: set() for r in (63, 64, 128)}
        for s in range(5):
            p = D.parse(L.case(f"carry_c{ch}_s{s}").file)
            assert (p["H"], p["W"], D.CHANNELS[p["color_type"]]) == (129, 7, ch)
            for r in on:
                on[r].add(L.filtered_of(f"carry_c{ch}_s{s}")[r * (1 + 7 * ch)])
        assert all(v == {0, 1, 2, 3, 4} for v in on.values())
    f = L.filtered_of("avg_row64_c3")
    assert {f[r * 22] for r in range(65)} == {3}


def test_marker_scan_keeps_the_positions_the_builders_state():
    want = L.scan_kept()
    assert len(want) == 8 + 5 + 5 + 4 + 1 + 2
    files = {n: f for n, f, _ in L.limit_good()}
    files.update({n: f for n, f, _ in L.limit_malformed()})
    for name, kept in want.items():
        assert D.find_markers(D.parse(files[name])["stream"]) == kept, name
    assert want["scan_k0"] == [2, 46] and want["scan_k7"] == [2, 53] and want["scan_tile_2047"] == [2, 2051]
    cap = want["scan_cap_second_tile"]
    assert len(cap) == D.MAX_UNITS and 2050 < cap[-1] == 4083 < 2 + 2 * 2048
    assert D.parse(files["scan_cap_second_tile"])["stream"].count(C.MARKER) == 275
    for name in ("scan_tail", "scan_tail_k1", "scan_tail_k2", "scan_tail_k3"):
        s = D.parse(files[name])["stream"]
        assert want[name] == [2, len(s) - 4]                      # the Adler-32's first byte
