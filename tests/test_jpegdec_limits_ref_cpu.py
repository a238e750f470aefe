"""CPU tests of the files of tests/jpegdec_limit_cases.py: every file has, by its own bytes, the property its name
promises; the restatement (tests/jpegdec_ref.py) equals Pillow where Pillow is the judge (narrow and extremely long
images); the sub-stream restatement (tests/jpegdec_sync_ref.py) and the planner agree on what is planned.  No device."""
import numpy as np

import jpegdec_cases as C
import jpegdec_limit_cases as L
import jpegdec_ref as D
import jpegdec_sync_cases as SC
import jpegdec_sync_ref as R


def stream(f):
    return D.parse(f)["stream"]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
def equals_pillow(files):
    for name, f in files:
        for mode in ("RGB", "L"):
            st, img, _ = D.decode(f, mode)
            assert st == D.OK, (name, D.STATUS_NAMES[st])
            want = C.pillow(f, mode)
            assert img.shape == want.shape and np.array_equal(img, want), (name, mode)


def test_narrow_files_equal_pillow():
    files = L.narrow()
    seen = {(p["W"], p["H"], p["ncomp"], p["hs"], p["vs"]) for p in (D.parse(f) for _, f in files)}
    for W in L.NARROW_W:
        for H in L.NARROW_H:
            assert {(W, H, 3, 1, 1), (W, H, 3, 2, 1), (W, H, 3, 2, 2)} <= seen
            assert ((W, H, 1, 1, 1) in seen) == (W in L.NARROW_GREY_W)
    assert len(files) == len(seen) == 8 * 8 * 3 + 3 * 8
    equals_pillow(files)


def test_extremely_long_files_equal_pillow():
    files = L.extreme()
    got = [(p["W"], p["H"], p["hs"], p["vs"], D.geometry(p)["nunits"]) for p in (D.parse(f) for _, f in files)]
    assert got == [(65500, 1, 2, 2, 1), (1, 65500, 2, 2, 1), (1, 65500, 2, 2, 4094), (65500, 2, 2, 1, 1)]
    equals_pillow(files)


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
def test_the_longest_block_is_432_raw_bytes():
    data, spans = L.encode([L.ALL_ONES], L.DC_LONG, L.AC_LONG)
    assert spans == [(0, 432)] and len(data) == 432 and len(data.replace(b"\xff\x00", b"\xff")) == 248
    assert D.code_table(*L.DC_LONG)[(16, 0xFFFE)] == 15 and D.code_table(*L.AC_LONG)[(16, 0xFFFE)] == 0x0F


def test_long_streams_hold_what_their_names_promise():
    ring = 2048
    for name, (f, spans, ri) in L.long_streams().items():
        p = D.parse(f)
        assert p["ri"] == ri and D.geometry(p)["nblocks"] == len(spans) == p["W"] // 8, name
        assert max(b - a for a, b in spans) >= 400, name
        st, planes, info = D.entropy(p)
        assert st == D.OK and info["eoi"], (name, D.STATUS_NAMES[st])
        assert [a for a, _ in info["units"]] == [spans[k][0] for k in range(0, len(spans), ri or len(spans))], name
    by = L.long_streams()
    assert len(stream(by["long_8"][0])) > ring + 1024                    # the ring wraps
    phases = {a % 256 for (a, b) in by["long_mixed_12"][1] if b - a >= 400}
    assert len(phases) >= 6                                              # long blocks start at many phases of a 256-byte chunk
    units = [b - a for a, b in D.entropy(D.parse(by["long_ri5_12"][0]))[2]["units"]]
    assert len(units) == 3 and units[0] > ring and units[1] > ring and units[2] < ring
    planes = D.entropy(D.parse(by["long_random"][0]))[1][0]
    assert (planes[0, :, 1:] > 0).any() and (planes[0, :, 1:] < 0).any() and D.parse(by["long_random"][0])["qt"][0] == [255] * 64
    px = D.decode(by["long_random"][0])[1]
    assert px.min() == 0 and px.max() == 255 and len(np.unique(px)) > 2      # the clamp at both ends, and values between


def test_long_streams_are_accepted_by_the_sub_stream_restatement():
    by = dict(L.long_files())
    for name, S in (("long_8", 32), ("long_8", 512), ("long_mixed_12", 32), ("long_random", 64)):
        p = D.parse(by[name])
        accepted, rounds, planes, nseg = R.decode_file(by[name], S, 256)
        want = D.entropy(p)[1]
        assert accepted == 1 and nseg == -(-len(p["stream"]) // S) and all(np.array_equal(a, b) for a, b in zip(planes, want)), (name, S)
        assert rounds <= 256 and (S != 32 or rounds > 64), (name, S, rounds)      # many segments inside one block: slow to fall in step
    assert R.decode_file(by["long_ri5_12"], 32, 256) == (0, 0, None, 0)


def test_cut_long_streams_are_truncated():
    (_, a), (_, b) = L.long_cuts()
    whole = len(stream(dict(L.long_files())["long_8"]))
    assert 432 < len(stream(a)) < 2 * 432 and 4 * 432 < len(stream(b)) <= 4 * 432 + 12 < whole
    for f in (a, b):
        assert D.decode(f)[0] == D.E_TRUNCATED
        for S in (32, 512):
            assert R.decode_file(f, S, 256)[0] == 0


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
def test_restart_markers_sit_where_the_scan_changes_path():
    files = dict(L.restart_files())
    rst = {n: L.scan_offsets(stream(f)) for n, f in files.items()}
    for n, f in files.items():
        p = D.parse(f)
        st, units, eoi = D.scan(p["stream"], D.geometry(p)["nunits"])
        assert st == D.OK and eoi and [a for _, a in units] == rst[n][0] + [rst[n][1]], n
        assert D.decode(f)[0] == D.OK, n
    every = [o for offs, _ in rst.values() for o in offs]
    assert {o % 8 for o in every} == set(range(8))
    tile = 2048
    assert rst[L.RST_AT_2047[0]][0][L.RST_AT_2047[1]] % tile == tile - 1 and rst[L.RST_AT_2048[0]][0][L.RST_AT_2048[1]] % tile == 0
    assert rst["eoi_ff_2047"][1] % tile == tile - 1 and rst["eoi_ff_2048"][1] % tile == 0
    many = D.geometry(D.parse(files["rst_1230_units"]))["nunits"]
    assert 1000 <= many < D.MAX_UNITS and rst["rst_1230_units"][1] > 2 * tile
    for n, fill in (("fill_1", 1), ("fill_3000", 3000)):
        s, term = stream(files[n]), rst[n][1]
        assert s[term:] == b"\xff" * fill + b"\xff\xd9" and s[term - 1] != 0xFF


def test_damaged_restart_files_and_the_fill_byte_in_front_of_a_restart_marker():
    files = L.restart_damaged()
    assert len(files) == 7
    for n, f in files:
        assert D.decode(f)[0] == D.E_RESTART, n
    # one fill byte in front of a restart marker ends the data here; libjpeg skips it, and Pillow decodes the file
    f = dict(files)["fill_before_rst"]
    good = dict(L.restart_files())["fill_1"]
    assert len(f) == len(good) + 1 and b"\xff\xff\xd7" in stream(f)
    assert D.decode(good)[0] == D.OK and C.pillow(f).shape == D.decode(good)[1].shape      # (hostile values: only that it decodes)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
def uend(f):
    return D.scan(stream(f), 1)[1][0][1]


def test_data_ends_on_and_next_to_a_segment_boundary():
    files = L.data_ends()
    assert [uend(f) % 32 for _, f in files] == list(L.END_RESIDUES)
    for name, f in files:
        p = D.parse(f)
        assert D.geometry(p)["nunits"] == 1 and len(p["stream"]) == uend(f) + 2 and uend(f) >= 64
        accepted, rounds, planes, nseg = R.decode_file(f, 32, SC.MAX_ROUNDS)
        assert accepted == 1 and nseg == R.planned_segments(p, 32) == -(-(uend(f) + 2) // 32), name
        assert all(np.array_equal(a, b) for a, b in zip(planes, D.entropy(p)[1])), name
    base = uend(files[0][1]) // 32
    extra = []
    for (name, f), k in zip(L.behind_end(), L.BEHIND):
        s = stream(f)
        assert uend(f) == 32 * base and len(s) == 32 * base + 2 + k
        accepted, _, planes, nseg = R.decode_file(f, 32, SC.MAX_ROUNDS)
        assert accepted == 1 and D.decode(f)[0] == D.OK and all(np.array_equal(a, b) for a, b in zip(planes, D.entropy(D.parse(f))[1])), name
        extra.append(nseg - base)
    assert extra == [1, 2, 4]                                            # segments that lie wholly behind the data's end
    junk = stream(L.behind_end()[2][1])[32 * base + 2:]
    assert b"\xff\xd0" in junk and b"\xff\x00" in junk and b"\x00\x00\x00" in junk


def test_the_smallest_plans():
    from attwarp_amd import jpeg
    for name, f, S, want in L.smallest_plans():
        p = D.parse(f)
        assert len(p["stream"]) in (2 * S, 2 * S - 1) and uend(f) <= 32                   # (a second segment is wholly behind the data)
        assert R.planned_segments(p, S) == want == jpeg.plan([f], segment_bytes=S)[0][0]["segments"], name
        accepted, rounds, planes, nseg = R.decode_file(f, S, SC.MAX_ROUNDS)
        assert nseg == want and accepted == (want != 0), name
        if accepted:
            assert np.array_equal(planes[0], D.entropy(p)[1][0]), name


def test_the_cap_on_segments():
    from attwarp_amd import jpeg
    (_, at), (_, over) = L.cap_files()
    pa, po = D.parse(at), D.parse(over)
    assert len(pa["stream"]) == L.CAP_SEGMENTS * L.CAP_BYTES == len(po["stream"]) - 1 and R.MAX_SEGMENTS == jpeg.MAX_SEGMENTS == L.CAP_SEGMENTS
    assert 15000 * 32 < uend(at) == uend(over) < L.CAP_SEGMENTS * 32
    assert R.planned_segments(pa, 32) == L.CAP_SEGMENTS and R.planned_segments(po, 32) == 0
    parsed, _, hdr = jpeg.plan([at, over], segment_bytes=32, max_rounds=256)
    assert [p["segments"] for p in parsed] == [L.CAP_SEGMENTS, 0] and hdr.reserved == 1
