"""CPU tests of the restatement of the JPEG decoder's sub-streams (tests/jpegdec_sync_ref.py) against the sequential
restatement (tests/jpegdec_ref.py), and of the planning, which touches no device."""
import numpy as np
import pytest

import jpegdec_cases as C
import jpegdec_ref as D
import jpegdec_sync_cases as SC
import jpegdec_sync_ref as R


def same_planes(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("S", SC.SEGMENT_BYTES)
def test_every_one_unit_good_file_is_accepted_with_the_sequential_coefficients(S):
    planned = 0
    for name, f in SC.all_one_unit_good():
        p = D.parse(f)
        accepted, rounds, planes, nseg = R.decode_file(f, S, SC.MAX_ROUNDS)
        assert nseg == R.planned_segments(p, S)
        if nseg == 0:
            assert len(p["stream"]) < 2 * S and (accepted, rounds, planes) == (0, 0, None), name
            continue
        planned += 1
        st, want, _ = D.entropy(p)
        assert st == D.OK and accepted == 1 and same_planes(planes, want), (name, S)
        assert 1 <= rounds <= nseg, (name, S, rounds, nseg)
    assert planned >= 9


def test_the_corpus_holds_what_its_names_promise():
    p = D.parse(SC.good_file(SC.STRADDLE))
    uend = D.scan(p["stream"], 1)[1][0][1]
    for S in (32, 64, 128):
        assert R.straddles(p["stream"], uend, S), S
    large = D.parse(SC.good_file(SC.LARGE))
    assert len(large["stream"]) >= 33 * 1024
    nseg = R.planned_segments(large, 32)
    assert nseg > 256 and nseg % 256 != 0
    assert R.decode_file(SC.good_file(SC.LARGE), 32, SC.MAX_ROUNDS)[1] <= 16                 # it falls in step quickly
    assert len(D.parse(SC.good_file(SC.SHORT))["stream"]) < 64
    assert R.decode_file(SC.good_file(SC.SLOW), 32, SC.MAX_ROUNDS)[1] > 61                   # and this one slowly ...
    assert R.decode_file(SC.good_file(SC.SLOW), 32, 4)[:2] == (0, 4)          # ... so a cap of 4 rejects it


def test_a_segment_that_starts_on_a_stuffed_zero_starts_one_byte_later():
    s = bytes([0x12, 0xFF, 0x00, 0x34, 0xFF, 0x00, 0x00, 0x56])
    assert R.guess(s, 1, 2, 8) == (3, 0, 0, 0)               # byte 2 is the 00 behind an FF
    assert R.guess(s, 1, 4, 8) == (4, 0, 0, 0)               # byte 4 is an FF: data
    assert R.guess(s, 3, 2, 8) == (6, 0, 0, 0)               # byte 6 is a 00 behind a stuffed 00: data
    assert R.guess(s, 1, 5, 8) == (6, 0, 0, 0) and R.guess(s, 2, 4, 8) == (8, 0, 0, 0)


def test_the_position_is_canonical_across_stuffed_bytes():
    """Every bit position of a unit maps to one (byte, bit), never on a stuffed 00, and back."""
    s = bytes([0xFF, 0x00, 0xFF, 0x00, 0x00, 0x81, 0xFF, 0x00])
    un = R.Unit(s, len(s))
    assert un.raw == [0, 2, 4, 5, 6] and un.n == 40
    for u in range(un.n):
        byte, bit = un.to_pos(u)
        assert s[byte] != 0 or byte == 0 or s[byte - 1] != 0xFF or byte == 4
        assert un.to_bit(byte, bit) == u
    assert un.to_pos(un.n) == (len(s), 0) and un.to_bit(len(s), 0) == un.n
    assert un.window(8) >> 8 == 0xFF00 and un.window(12) >> 8 == 0xF008


def test_one_unit_malformed_files_are_rejected_or_exact():
    seen = {0: 0, 1: 0}
    for name, f, _ in C.malformed():
        p = D.parse(f)
        if D.geometry(p)["nunits"] != 1:
            continue
        for S in (32, 128):
            accepted, rounds, planes, nseg = R.decode_file(f, S, SC.MAX_ROUNDS)
            if nseg:
                seen[accepted] += 1
            if accepted:
                st, want, _ = D.entropy(p)
                assert st in (D.OK, D.E_NO_EOI) and same_planes(planes, want), (name, S)
    assert seen[0] >= 5 and seen[1] >= 3


def test_garbage_behind_the_last_mcu_is_tolerated():
    f = SC.good_file("smooth_200x136_q90_s0")
    g = f[:-2] + bytes(range(1, 200)) + f[-2:]
    assert D.decode(g)[0] == D.OK
    accepted, _, planes, _ = R.decode_file(g, 128, SC.MAX_ROUNDS)
    assert accepted == 1 and same_planes(planes, D.entropy(D.parse(g))[1])


def test_planning_touches_no_device_and_substreams_off_is_the_old_plan():
    from attwarp_amd import jpeg
    names = ["ri_wrap", "big_200x136", "noise_64x48_s1", "grey_17x15", "noise_1x1_s0"]
    files = [C.good_file(n) for n in names] + [f for _, f in SC.good()]
    for S in (32, 128, 512):
        parsed, table, hdr = jpeg.plan(files, substreams="auto", segment_bytes=S)
        want = [R.planned_segments(D.parse(f), S) for f in files]
        assert [p["segments"] for p in parsed] == want
        assert hdr.reserved == sum(w != 0 for w in want) and hdr.scratch_bytes % 256 == 0
        assert want[0] == 0 and want[1] == 0 and want[-1] == 0 and (S > 32 or want[2] != 0)
    _, off_table, off = jpeg.plan(files, substreams=False)
    _, on_table, on = jpeg.plan(files)
    assert off.reserved == 0 and off.scratch_bytes % 256 == 0 and off_table.size == on_table.size
    for key in ("B", "total_units", "idct_tiles", "color_tiles", "table_bytes", "out_bytes", "stream_bytes", "off_images"):
        assert getattr(off, key) == getattr(on, key), key
    assert on.scratch_bytes > off.scratch_bytes
    for kw in (dict(segment_bytes=48), dict(segment_bytes=16), dict(segment_bytes=1024), dict(max_rounds=0), dict(substreams="yes")):
        with pytest.raises(ValueError):
            jpeg.plan(files, **kw)
