"""Plain-Python restatement, in the raw-byte domain, of the sub-streams of the scans-of-every-layout family (DESIGN.md 3.25,
csrc/jpegscan_sync_blocks.hpp), on top of jpegscan_ref (the family) and jpegprog_sync_ref (the raw-byte machinery): it
decides route, segments, rounds, accepted and the entries of every scan.
  * the plan: which scans are cut (never a sequential one) and into how many segments, and the PERIOD of a cut DC first
    pass's table sequence, tables compared by content;
  * the first passes over the general MCU: one segment's decode from a state that carries the slot modulo the period, the
    ten DC sums by place, the Jacobi rounds, the blocks and predictors in front of every segment, the acceptance rule;
  * the DC refinement route (block n's bit is data bit n) and the AC refinement's exact skim;
  * trace(): the sequential walk with jpegprog_ref's OWN block routines over this family's geometry, noting where every
    block starts and the predictors in front of it.
The WRITE passes are not restated: tests/jpegscan_sync_host_main.cpp compares their coefficients with js_decode_unit's walk
after every scan, and the GPU tests with the keyword-off run."""
from __future__ import annotations

import numpy as np

import jpegdec_ref as D
import jpegfmt_ref as F
import jpegscan_ref as R
from jpegprog_sync_ref import CAP, MAX_SEGMENTS, Unit, data_bytes, scan_data
from jpegscan_ref import P, ZIGZAG


def kind(sc):
    return 4 if sc["seq"] else (2 if sc["ss"] else 0) + (1 if sc["ah"] else 0)


def geometry(p, sc):
    """(MCUs per row, MCUs, [(component, yy, xx, place in the scan)] per block of an MCU)."""
    return R.scan_mcus(p["W"], p["H"], p["samp"], sc["comps"])


def table_key(t):
    return tuple(t[0]), tuple(t[1][:sum(t[0])])


def period(p, sc):
    """A DC first pass: the smallest divisor of the blocks per MCU whose DC tables repeat, by content; else 1."""
    if kind(sc) != 0:
        return 1
    seq = [table_key(sc["dc"][t]) for _, _, _, t in geometry(p, sc)[2]]
    n = len(seq)
    return next(q for q in range(1, n + 1) if n % q == 0 and all(seq[j] == seq[j + q] for j in range(n - q)))


def plan(p, segment_bytes, kinds=(0, 1, 2, 3)):
    """Per scan (route, segments, period): route 0, no segments and period 1 for a scan that stays on one lane."""
    out = []
    for sc in p["scans"]:
        n = len(scan_data(p, sc))
        nseg = -(-n // segment_bytes)
        mcux, nmcu, slots = geometry(p, sc)
        cut = kind(sc) in kinds and sc["units"] == 1 and n >= 2 * segment_bytes and nseg <= MAX_SEGMENTS and nmcu * len(slots) < CAP
        out.append((1 + kind(sc), nseg, period(p, sc)) if cut else (0, 0, 1))
    return out


def scan_blocks(p, sc, planes):
    """The scan's blocks (views into the padded planes) in the order the scan codes them."""
    mcux, nmcu, slots = geometry(p, sc)
    out = []
    for m in range(nmcu):
        mx, my = m % mcux, m // mcux
        for c, yy, xx, _ in slots:
            h, v = p["samp"][c]
            out.append(planes[c][my, mx] if len(sc["comps"]) == 1 else planes[c][my * v + yy, mx * h + xx])
    return out


def dc_refine(p, sc, segment_bytes):
    """A cut DC refinement -> (accepted, [first block of every segment])."""
    d = scan_data(p, sc)
    nseg = -(-len(d) // segment_bytes)
    mcux, nmcu, slots = geometry(p, sc)
    firsts, before = [], 0
    for s in range(nseg):
        firsts.append(before * 8)
        before += data_bytes(d, s * segment_bytes, min((s + 1) * segment_bytes, len(d)))
    return before * 8 >= nmcu * len(slots), firsts


def first_segment(u, sc, tabs, slots, per, entry, seg_end):
    """One segment of a first pass from entry = (byte, bit, slot class, k) -> dict(exit, nend, eclean, dc: the sums by place)."""
    dc = sc["ss"] == 0
    ss, se, nslot = sc["ss"], sc["se"], len(slots)
    byte, bit, cls, k = entry
    q = u.q(byte, bit)
    cls = cls if dc and cls < per else 0
    k = 0 if dc else (k if ss <= k <= se else ss)
    nend, eclean, sums, at_end, b, place = 0, None, [0] * nslot, False, u.bits, 0
    while u.byte(q) < seg_end:
        b.pos = q
        st, ended = R.OK, 0
        if dc:
            st, s = b.symbol(tabs[slots[cls][3]])            # (the table of slot `cls`: equal, by content, to the true slot's)
            if not st:
                st, v = b.value(s & 15)
            if not st:
                sums[place] = (sums[place] + D.extend(v, s & 15)) & 0xFFFFFFFF
                ended = 1
        else:
            st, rs = b.symbol(tabs[0])
            if not st:
                run, s = rs >> 4, rs & 15
                if s == 0:
                    if run == 15:
                        if k + 16 > se + 1:
                            st = P.E_COEFF
                        else:
                            k += 16
                    else:
                        st, v = b.value(run)
                        if not st:
                            ended = (1 << run) + v
                elif k + run > se:
                    st = P.E_COEFF
                else:
                    st, v = b.value(s)
                    if not st:
                        k += run + 1
                if not st and not ended and k > se:
                    ended = 1
        q = b.pos
        if st:
            eclean = nend if eclean is None else eclean
            if st == P.E_TRUNCATED or q >= u.T:
                at_end = True
                break
            q += 1
        elif ended:
            nend = min(nend + ended, CAP)
        if st or ended:
            cls, place = (cls + 1) % per, (place + 1) % nslot
            k = 0 if dc else ss
    ex = (u.n, 0, cls, k) if at_end else (u.byte(q), q & 7, cls, k)
    return dict(exit=ex, nend=nend, eclean=eclean, dc=sums)


def first_pass(p, sc, S, max_rounds):
    """A cut first pass -> dict(rounds, accepted, entries [(byte, bit, slot class, k)], before [blocks in front of every segment],
    pred [the four predictors, by the component's place in the scan, at every segment's start], period)."""
    u = Unit(scan_data(p, sc))
    nseg = -(-u.n // S)
    mcux, nmcu, slots = geometry(p, sc)
    nslot, per = len(slots), period(p, sc)
    tabs = [D.code_table(*t) for t in (sc["dc"] if sc["ss"] == 0 else sc["ac"])]
    expected = nmcu * nslot
    entries = [(u.guess(s, S), 0, 0, sc["ss"]) for s in range(nseg)]
    dirty, res, rounds, converged = [True] * nseg, [None] * nseg, 0, False
    while rounds < max_rounds:
        rounds += 1
        for s in range(nseg):
            if dirty[s]:
                res[s] = first_segment(u, sc, tabs, slots, per, entries[s], min((s + 1) * S, u.n))
        changed = False
        for s in range(nseg - 1, -1, -1):
            dirty[s] = s > 0 and res[s - 1]["exit"] != entries[s]
            if dirty[s]:
                entries[s] = res[s - 1]["exit"]
                changed = True
        if not changed:
            converged = True
            break
    before, preds, done, bad, found, pred = [], [], 0, False, False, [0, 0, 0, 0]
    for s in range(nseg):
        before.append(done)
        preds.append(list(pred))
        r = res[s]
        if done < expected:
            if sc["ss"] == 0 and entries[s][2] != done % per:
                bad = True
            last = expected - 1 - done
            if last < r["nend"]:
                if r["eclean"] is None or r["eclean"] > last:
                    found = True
                else:
                    bad = True
            elif r["eclean"] is not None:
                bad = True
        if sc["ss"] == 0:
            for i, dsum in enumerate(r["dc"]):               # the sums by place -> by component: the true slot follows from `done`
                t = slots[(done + i) % nslot][3]
                pred[t] = (pred[t] + dsum) & 0xFFFFFFFF
        done = min(done + r["nend"], CAP)
    return dict(rounds=rounds, accepted=converged and found and not bad, entries=entries, before=before, pred=preds, unit=u, expected=expected,
                period=per)


def skim(p, sc, S, masks):
    """A cut AC refinement -> dict(accepted, entries [(data bit, block, k, run)]); masks[n]: bit k set where block n's coefficient at
    zigzag k, inside the band, has history (jpegprog_sync_ref.skim over this family's parse)."""
    u = Unit(scan_data(p, sc))
    nseg = -(-u.n // S)
    ss, se = sc["ss"], sc["se"]
    expected = geometry(p, sc)[1]
    table = D.code_table(*sc["ac"][0])
    Pm = [0]
    for m in masks:
        Pm.append(Pm[-1] + bin(m).count("1"))
    first = [8 * u.didx[min(s * S, u.n)] for s in range(nseg)]
    b, entries, n, k, run = u.bits, [], 0, ss, 0
    b.pos = 0

    def skip(nb):
        if b.pos + nb > u.T:
            return False
        b.pos += nb
        return True

    ok = True
    while True:
        while len(entries) < nseg and b.pos >= first[len(entries)]:
            entries.append((b.pos, n, k, run))
        if n >= expected:
            break
        if run > 0:
            rem = min(run, expected - n)
            j = rem
            if len(entries) < nseg:
                target = first[len(entries)] - b.pos
                j = next((x for x in range(1, rem + 1) if Pm[n + x] - Pm[n] >= target), rem)
            if not skip(Pm[n + j] - Pm[n]):
                ok = False
                break
            n, run = n + j, run - j
            continue
        st, rs = b.symbol(table)
        if st:
            ok = False
            break
        r, s = rs >> 4, rs & 15
        m = masks[n]
        if s == 0 and r != 15:
            st, v = b.value(r)
            if st or not skip(bin(m >> k).count("1")):
                ok = False
                break
            run = (1 << r) + v - 1
            n, k = n + 1, ss
            continue
        if s:
            if s != 1 or b.value(1)[0]:
                ok = False
                break
        nb, kk, found = 0, k, False
        while kk <= se:
            if (m >> kk) & 1:
                nb += 1
            else:
                if r == 0:
                    found = True
                    break
                r -= 1
            kk += 1
        if not found or not skip(nb):
            ok = False
            break
        k = kk + 1
        if k > se:
            n, k = n + 1, ss
    if ok:
        entries += [(None, expected, ss, 0)] * (nseg - len(entries))
    return dict(accepted=ok, entries=entries, first=first, unit=u, expected=expected)


_TRACE = {}


def trace(f):
    """The sequential walk over every scan of a file with jpegprog_ref's and jpegdec_ref's own block routines -> (parse, per scan
    dict(status, starts: the data bit at which every block of a ONE-unit scan starts (a block inside a first pass's EOB run:
    where the run left the reader), preds: the predictors, by place in the scan, in front of every block of a DC first pass,
    masks: for an AC refinement the history masks of its blocks BEFORE the scan)).  The walk goes on behind a failing scan, as
    the device's does."""
    key = bytes(f)
    if key in _TRACE:
        return _TRACE[key]
    p = R.parse(key)
    g = F.geometry(p)
    d = p["data"]
    planes = [np.zeros((g["bh"][c], g["bw"][c], 64), np.int16) for c in range(p["ncomp"])]
    out = []
    for sc in p["scans"]:
        st0, units, _ = D.scan(d[sc["off"]:], sc["units"])
        rec = dict(status=R.E_RESTART if st0 else R.OK, starts=[], preds=[], masks=None)
        out.append(rec)
        if st0:
            continue
        blocks = scan_blocks(p, sc, planes)
        mcux, nmcu, slots = geometry(p, sc)
        nslot, ri = len(slots), sc["ri"] or nmcu
        dct, act = [D.code_table(*t) for t in sc["dc"]], [D.code_table(*t) for t in sc["ac"]]
        if kind(sc) == 3:
            rec["masks"] = [sum(1 << k for k in range(sc["ss"], sc["se"] + 1) if blk[ZIGZAG[k]] != 0) for blk in blocks]
        s = d[sc["off"]:]
        for ku, (a, b) in enumerate(units):
            bits = D._Bits(s[a:b])
            pred, run, ust = [0, 0, 0, 0], 0, R.OK
            for o in range(ku * ri * nslot, min((ku + 1) * ri, nmcu) * nslot):
                blk, t = blocks[o], slots[o % nslot][3]
                if len(units) == 1:
                    rec["starts"].append(bits.pos)
                    rec["preds"].append([x & 0xFFFFFFFF for x in pred])
                if sc["seq"]:
                    blk[:] = 0
                    ust, pred[t] = D.decode_block(bits, dct[t], act[t], pred[t], blk)
                elif sc["ss"] == 0 and sc["ah"] == 0:
                    ust, pred[t] = P.dc_first(bits, dct[t], pred[t], sc["al"], blk)
                elif sc["ss"] == 0:
                    ust = P.dc_refine(bits, sc["al"], blk)
                elif sc["ah"] == 0:
                    if run > 0:
                        run -= 1
                    else:
                        ust, run = P.ac_first(bits, act[0], sc["ss"], sc["se"], sc["al"], blk)
                else:
                    ust, run = P.ac_refine(bits, act[0], sc["ss"], sc["se"], sc["al"], run, blk)
                if ust:
                    break
            if ust and not rec["status"]:
                rec["status"] = ust
    _TRACE[key] = (p, out)
    return _TRACE[key]


_RECORDS = {}


def records(f, S, max_rounds, kinds=(0, 1, 2, 3)):
    """Per scan (route, segments, rounds, accepted) as the device leaves them, and the routes' own results (None: not cut).
    exact[i]: the record does not depend on coefficients a failing earlier scan left behind."""
    key = (bytes(f), S, max_rounds, tuple(kinds))
    if key in _RECORDS:
        return _RECORDS[key]
    p, tr = trace(f)
    restart = any(t["status"] == R.E_RESTART for t in tr)
    recs, details, exact, failed = [], [], [], False
    for sc, (route, nseg, _), t in zip(p["scans"], plan(p, S, kinds), tr):
        det = None
        if route == 0 or restart:
            recs.append((route, nseg, 0, 0))
        elif route in (1, 3):
            det = first_pass(p, sc, S, max_rounds)
            recs.append((route, nseg, det["rounds"], int(det["accepted"])))
        elif route == 2:
            recs.append((route, nseg, 0, int(dc_refine(p, sc, S)[0])))
        else:
            det = skim(p, sc, S, t["masks"])
            recs.append((route, nseg, 0, int(det["accepted"])))
        details.append(det)
        exact.append(not (failed and route == 4))
        failed = failed or t["status"] != R.OK
    _RECORDS[key] = (recs, details, exact)
    return _RECORDS[key]
