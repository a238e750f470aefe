"""The raw-byte restatement of the layout scans' sub-streams (tests/jpegscan_sync_ref.py) against the
sequential walk, for every file of tests/jpegscan_sync_cases.py at 32 and 256 bytes per segment: the entries at the fixed
point of the first passes' rounds (position, slot modulo the PERIOD, blocks and predictors in front) and the entries the AC
refinement's skim notes equal what is read off the walk's block starts; every cut scan of a good file is accepted; the plan
and the period are the planner's (attwarp_amd.jpeg.plan and the C ABI, host only); a sequential scan is never cut; no scan
of a malformed file is accepted where the walk fails.  Each case's own property is asserted by its builder."""
import numpy as np
import pytest

import jpegscan_ref as R
import jpegscan_sync_cases as SC
import jpegscan_sync_ref as Y


def test_every_case_has_the_property_its_name_claims():
    names = [n for n, _ in SC.good()]
    assert len(names) == 20 and len(SC.malformed()) == 21 + 5
    assert [w for _, _, w in SC.table_sequences()] == [4, 5, 2]
    for name, f in SC.good():
        assert R.decode(f)[0] == 0, name


def test_the_period_is_the_table_sequences_by_content():
    for name, f in SC.shared_table():
        p = R.parse(f)
        assert Y.period(p, p["scans"][0]) == 1 and Y.plan(p, 32)[0][2] == 1, name
    for name, f, want in SC.table_sequences():
        p = R.parse(f)
        assert Y.period(p, p["scans"][0]) == want == SC.period(f, 0)[0], name
        assert all(Y.period(p, sc) == 1 for sc in p["scans"][1:] if Y.kind(sc) != 0), name
    p = R.parse(SC.pillow_440())
    assert Y.period(p, p["scans"][0]) == 4
    p = R.parse(SC.ten_blocks())
    assert Y.period(p, p["scans"][0]) == 1 and len(Y.geometry(p, p["scans"][0])[2]) == 10     # one table: ten slots nobody can tell apart


@pytest.mark.parametrize("segment_bytes", [32, 256])
def test_the_plan_is_the_planners(segment_bytes):
    from attwarp_amd import jpeg
    files = SC.good() + SC.malformed()
    for name, f in files:                                    # (one plan per file: a list of this family is one table)
        parsed, table, header = jpeg.plan([f], all_scans=True, scan_substreams=True, segment_bytes=segment_bytes)
        want = Y.plan(R.parse(f), segment_bytes)
        assert parsed[0]["scan_segments"] == [n for _, n, _ in want], name
        auto = jpeg.plan([f], all_scans=True, scan_substreams="auto", segment_bytes=segment_bytes)[0][0]
        kinds = [jpeg.SCAN_KINDS.index(k) for k in jpeg.AUTO_LAYOUT_SCAN_KINDS]
        assert auto["scan_segments"] == [n for _, n, _ in Y.plan(R.parse(f), segment_bytes, kinds)], name
    p = R.parse(SC.sequential())
    assert Y.plan(p, 32) == [(0, 0, 1)] * 3 and all(len(Y.scan_data(p, sc)) >= 64 for sc in p["scans"])


def check_entries(name, p, sc, route, det, t, S):
    """The entries at the fixed point (first passes) or from the skim equal those read off the sequential walk's block starts."""
    starts, u, expected, ss = t["starts"], det["unit"], det["expected"], sc["ss"]
    assert len(starts) == expected, name
    edge = starts + [None]
    if route in (1, 3):
        per = det["period"]
        for s, ((byte, bit, cls, k), n) in enumerate(zip(det["entries"], det["before"])):
            if n >= expected:
                continue
            q = u.q(byte, bit)
            if route == 1:
                assert q == starts[n] and cls == n % per and k == 0 and det["pred"][s] == t["preds"][n], (name, s)
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
    seen = {1: 0, 2: 0, 3: 0, 4: 0}
    for name, f in SC.good():
        recs, details, _ = Y.records(f, segment_bytes, 64)
        p, tr = Y.trace(f)
        assert all(t["status"] == 0 for t in tr), name
        for sc, (route, nseg, rounds, acc), det, t in zip(p["scans"], recs, details, tr):
            assert (route == 0) == (nseg == 0) and (route == 0 or acc == 1), (name, route, nseg, rounds)     # every cut scan is accepted
            if route in (1, 3, 4):
                assert rounds <= nseg and rounds < 64, (name, route, nseg, rounds)
                check_entries(name, p, sc, route, det, t, segment_bytes)
            if route == 2:                                   # the bits cover the blocks, eight per data byte
                acc2, firsts = Y.dc_refine(p, sc, segment_bytes)
                assert acc2 and firsts == sorted(firsts) and firsts[0] == 0, name
            if route:
                seen[route] += 1
    # (at 256 bytes no DC refinement of these small files is two segments long)
    assert all(v >= (6 if segment_bytes == 32 else r != 2) for r, v in seen.items()), seen


def test_one_round_does_not_settle_a_first_pass_of_three_segments():
    p = R.parse(SC.ten_blocks())
    recs = Y.records(SC.ten_blocks(), 32, 1)[0]
    first = [r for r in recs if r[0] in (1, 3) and r[1] > 2]
    assert first and all(r[2] == 1 and r[3] == 0 for r in first)
    assert all(r[3] == 1 for r in recs if r[0] in (2, 4)) and len(recs) == len(p["scans"])


def test_no_scan_of_a_malformed_file_is_accepted_where_the_walk_fails():
    fails = 0
    for name, f in SC.malformed():
        recs, _, exact = Y.records(f, 32, 64)
        p, tr = Y.trace(f)
        for (route, nseg, rounds, acc), t, ex in zip(recs, tr, exact):
            if ex and t["status"] != 0:
                assert acc == 0, name
                fails += route != 0
    assert fails >= 5
