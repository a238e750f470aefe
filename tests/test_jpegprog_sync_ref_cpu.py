"""The raw-byte restatement of the progressive scans' sub-streams (tests/jpegprog_sync_ref.py) against the sequential walk
of tests/jpegprog_ref.py, for every good file and limit file at 32 and 256 bytes per segment: the entries at the fixed point
of the first passes' rounds and the entries the AC refinement's skim notes equal the block starts read off the walk; the
bits a cut DC refinement sets, segment by segment, are the bits the walk leaves in the coefficients; every cut scan is
accepted; the plan is the planner's (attwarp_amd.jpeg.plan, host only), malformed files included; no scan of a malformed
file is accepted where the walk fails.  Coefficients WRITTEN are compared here for DC refinements only: the other write
passes are not restated in Python; tests/jpegprog_sync_host_main.cpp compares theirs with its own sequential walk after every
scan, and tests/test_jpegprog_sync_host_cpu.py holds that program's CRCs against jpegprog_ref's."""
import pytest

import jpegprog_cases as C
import jpegprog_ref as R
import jpegprog_sync_cases as SC
import jpegprog_sync_ref as Y


def good_files():
    return C.good() + SC.limits() + SC.larger()


@pytest.mark.parametrize("segment_bytes", [32, 256])
def test_dc_refinements_by_segments_equal_the_sequential_walk(segment_bytes):
    seen = 0
    for name, f in good_files() + [("eob_run_textured", SC.eob_run_textured()), ("most_segments", SC.most_segments(0))]:
        p = R.parse(f)
        st, _, info = R.decode(f)
        assert st == 0, name
        for sc, (route, nseg) in zip(p["scans"], Y.plan(p, segment_bytes)):
            if route != 2:
                continue
            accepted, firsts, ones = Y.dc_refine(p, sc, segment_bytes)
            assert accepted and len(firsts) == nseg and firsts == sorted(firsts), name
            blocks = Y.scan_blocks(p, sc, info["planes"])
            want = {n for n, blk in enumerate(blocks) if (int(blk[0]) >> sc["al"]) & 1}
            assert set().union(*ones) == want, name
            for s, mine in enumerate(ones):                 # every segment sets only blocks of its own range
                hi = firsts[s + 1] if s + 1 < nseg else len(blocks)
                assert all(firsts[s] <= n < hi for n in mine), (name, s)
            seen += 1
    assert seen >= (5 if segment_bytes == 32 else 2), seen


def test_a_truncated_dc_refinement_stays_on_one_lane_and_a_padded_one_is_accepted():
    f = SC.smallest(True)
    p = R.parse(f)
    cut = f[:p["scans"][1]["off"] + 63]                      # 504 of 512 bits: the walk reports E_TRUNCATED
    assert R.decode(cut)[0] == R.E_TRUNCATED
    assert Y.plan(R.parse(cut), 32)[1] == (0, 0)             # 63 bytes: not even cut, the one-lane route reports it
    wide = R.parse(SC.smallest(False))                       # 504 blocks in 63 bytes; at 512 blocks the bits would not cover
    short = dict(wide, W=wide["W"] + 8)
    assert Y.dc_refine(wide, wide["scans"][1], 32)[0] and not Y.dc_refine(short, short["scans"][1], 32)[0]
    g = R.parse(SC.most_segments(0))
    assert Y.dc_refine(g, g["scans"][1], 32)[0]              # padded behind the last block: still covered


@pytest.mark.parametrize("segment_bytes", [32, 256])
def test_the_plan_is_the_planners(segment_bytes):
    from attwarp_amd import jpeg
    files = good_files() + C.malformed()
    parsed, _, _ = jpeg.plan([f for _, f in files], progressive=True, scan_substreams=True, segment_bytes=segment_bytes)
    for (name, f), got in zip(files, parsed):
        assert got["scan_segments"] == [n for _, n in Y.plan(R.parse(f), segment_bytes)], name


def check_entries(name, p, sc, route, det, t, S):
    """The entries at the fixed point (first passes) or from the skim equal those read off the sequential walk's block starts."""
    starts, u, expected, ss = t["starts"], det["unit"], det["expected"], sc["ss"]
    assert len(starts) == expected, name
    edge = starts + [None]
    if route in (1, 3):
        nslot = len(R.scan_mcus(p, sc["comps"])[2])
        for s, ((byte, bit, slot, k), n) in enumerate(zip(det["entries"], det["before"])):
            if n >= expected:
                continue
            q = u.q(byte, bit)
            if route == 1:
                assert q == starts[n] and slot == n % nslot and k == 0, (name, s)
            elif k == ss:
                assert q == starts[n], (name, s)
            else:
                assert starts[n] < q and (edge[n + 1] is None or q < edge[n + 1]), (name, s)
            assert byte >= min(s * S, u.n) and (s == 0 or u.q(byte, bit) >= 8 * u.didx[min(s * S, u.n)]), (name, s)
        return
    for s, (q, n, k, run) in enumerate(det["entries"]):
        if n >= expected:
            continue
        assert q >= det["first"][s], (name, s)
        if k == ss:
            assert q == starts[n] and (n == 0 or s == 0 or starts[n - 1] < det["first"][s]), (name, s)
        else:
            assert run == 0 and starts[n] < q and (edge[n + 1] is None or q < edge[n + 1]), (name, s)


@pytest.mark.parametrize("segment_bytes", [32, 256])
def test_entries_of_every_cut_scan_equal_the_sequential_walks(segment_bytes):
    seen = {1: 0, 3: 0, 4: 0}
    # (the large flat picture only at 256 bytes, where its DC first pass is 80 segments: the small files' are too short to cut there)
    for name, f in good_files() + ([("eob_run_textured", SC.eob_run_textured())] if segment_bytes == 256 else []):
        recs, details, _ = Y.records(f, segment_bytes, 4096)
        p, tr = Y.trace(f)
        assert all(t["status"] == 0 for t in tr), name
        for sc, (route, nseg, rounds, acc), det, t in zip(p["scans"], recs, details, tr):
            if route in (1, 3, 4):
                assert acc == 1 and rounds <= nseg, (name, route, nseg, rounds)
                check_entries(name, p, sc, route, det, t, segment_bytes)
                seen[route] += 1
    assert all(v >= (10 if segment_bytes == 32 else 1) for v in seen.values()), seen


def test_no_scan_of_a_malformed_file_is_accepted_where_the_walk_fails():
    fails = 0
    for name, f in C.malformed():
        recs, _, exact = Y.records(f, 32, 4096)
        p, tr = Y.trace(f)
        for (route, nseg, rounds, acc), t, ex in zip(recs, tr, exact):
            if ex and t["status"] != 0:
                assert acc == 0, name
                fails += route != 0
    assert fails >= 1
