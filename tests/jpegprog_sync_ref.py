"""Plain-Python restatement, in the raw-byte domain, of the progressive scans' sub-streams (DESIGN.md 3.23,
csrc/jpegprog_sync_blocks.hpp): it decides route, segments, rounds, accepted and the entries of every cut scan.
  * the plan: which scans are cut and into how many segments; the data bytes of every segment (every byte but the 00 behind
    an FF, a pair across a boundary counted once);
  * the DC refinement route whole: block n's bit is data bit n, a segment's first block is eight times the data bytes in
    front of it, accepted when the bits cover the blocks; the bits it sets are compared with the sequential walk's coefficients;
  * the first passes: one segment's decode from a state, the Jacobi rounds over guessed states, the sums and the acceptance rule;
  * the AC refinement's skim over history masks and their prefix sums, with every segment's entry;
  * trace(): the sequential walk with jpegprog_ref's OWN block routines, noting where every block starts, against which
    tests/test_jpegprog_sync_ref_cpu.py holds the entries.
The WRITE passes of the first passes and of the AC refinement are not restated: their coefficients are compared with the
sequential walk by tests/jpegprog_sync_host_main.cpp after every scan (its CRC per scan is then held against jpegprog_ref's)
and with the keyword-off run on the GPU."""
from __future__ import annotations

import jpegdec_ref as D
import jpegprog_ref as R

MAX_SEGMENTS = 16384


def scan_data(p, sc):
    """The scan's entropy data: up to the first FF that neither 00 nor D0..D7 follows."""
    d = p["data"]
    i = sc["off"]
    while i < len(d):
        if d[i] == 0xFF and not (i + 1 < len(d) and (d[i + 1] == 0 or 0xD0 <= d[i + 1] <= 0xD7)):
            break
        i += 2 if d[i] == 0xFF else 1
    return bytes(d[sc["off"]:min(i, len(d))])


def plan(p, segment_bytes):
    """Per scan (route, segments): route 0 and no segments for a scan that stays on one lane."""
    out = []
    for sc in p["scans"]:
        n = len(scan_data(p, sc))
        nseg = -(-n // segment_bytes)
        cut = sc["units"] == 1 and n >= 2 * segment_bytes and nseg <= MAX_SEGMENTS
        out.append((1 + (2 if sc["ss"] else 0) + (1 if sc["ah"] else 0), nseg) if cut else (0, 0))
    return out


def data_bytes(d, a, b):
    return sum(1 for i in range(a, b) if not (d[i] == 0 and i > 0 and d[i - 1] == 0xFF))


def dc_refine(p, sc, segment_bytes):
    """A cut DC refinement -> (accepted, [first block of every segment], {block ordinal: 1} of the bits set, by segment)."""
    d = scan_data(p, sc)
    nseg = -(-len(d) // segment_bytes)
    nblocks = R.scan_mcus(p, sc["comps"])[1] * len(R.scan_mcus(p, sc["comps"])[2])
    firsts, ones, before = [], [], 0
    for s in range(nseg):
        a, b = s * segment_bytes, min((s + 1) * segment_bytes, len(d))
        firsts.append(before * 8)
        mine, n = set(), before * 8
        for i in range(a, b):
            if d[i] == 0 and i > 0 and d[i - 1] == 0xFF:
                continue
            mine |= {n + e for e in range(8) if (d[i] >> (7 - e)) & 1 and n + e < nblocks}
            n += 8
        ones.append(mine)
        before += data_bytes(d, a, b)
    return before * 8 >= nblocks, firsts, ones


def scan_blocks(p, sc, planes):
    """The scan's blocks (views into the padded planes) in the order the scan codes them."""
    g = D.geometry(p)
    mcux, nmcu, slots = R.scan_mcus(p, sc["comps"])
    out = []
    for m in range(nmcu):
        mx, my = m % mcux, m // mcux
        for c, yy, xx, _ in slots:
            if len(slots) == 1:
                out.append(planes[c][my, mx])
            else:
                h, v = g["samp"][c]
                out.append(planes[c][my * v + yy, mx * h + xx])
    return out


# ---- the routes that decode symbols: the first passes' rounds and the AC refinement's skim ------------------------------------------
# Positions are DATA bits (jpegdec_ref._Bits un-stuffs the unit); a state's canonical raw position is (the raw offset of the data
# byte that holds the bit, the bit's index in it), (len, 0) at the unit's end.
CAP = 1 << 24


class Unit:
    def __init__(self, d):
        self.d, self.n = d, len(d)
        self.raw_of, self.didx = [], [0] * (len(d) + 1)
        for i in range(len(d)):
            self.didx[i] = len(self.raw_of)
            if not (d[i] == 0 and i > 0 and d[i - 1] == 0xFF):
                self.raw_of.append(i)
        self.didx[len(d)] = len(self.raw_of)
        self.bits = D._Bits(d)
        self.T = self.bits.n
        assert self.T == 8 * len(self.raw_of)

    def byte(self, q):
        return self.raw_of[q >> 3] if (q >> 3) < len(self.raw_of) else self.n

    def q(self, byte, bit):
        return min(8 * self.didx[min(byte, self.n)] + bit, self.T)

    def guess(self, s, S):
        b = s * S
        if b >= self.n:
            return self.n
        return b + 1 if b > 0 and self.d[b] == 0 and self.d[b - 1] == 0xFF else b


def first_segment(u, sc, tabs, slots, entry, seg_end):
    """One segment of a first pass from entry = (byte, bit, slot, k) -> dict(exit, nend, eclean, dc)."""
    dc = sc["ss"] == 0
    ss, se, nslot = sc["ss"], sc["se"], len(slots)
    byte, bit, slot, k = entry
    q = u.q(byte, bit)
    slot = slot if dc and slot < nslot else 0
    k = 0 if dc else (k if ss <= k <= se else ss)
    nend, eclean, sums, at_end, b = 0, None, [0, 0, 0], False, u.bits
    while u.byte(q) < seg_end:
        b.pos = q
        st, ended = R.OK, 0
        if dc:
            t = slots[slot][3]
            st, s = b.symbol(tabs[t])
            if not st:
                st, v = b.value(s & 15)
            if not st:
                sums[t] = (sums[t] + D.extend(v, s & 15)) & 0xFFFFFFFF
                ended = 1
        else:
            st, rs = b.symbol(tabs[0])
            if not st:
                run, s = rs >> 4, rs & 15
                if s == 0:
                    if run == 15:
                        if k + 16 > se + 1:
                            st = R.E_COEFF
                        else:
                            k += 16
                    else:
                        st, v = b.value(run)
                        if not st:
                            ended = (1 << run) + v
                elif k + run > se:
                    st = R.E_COEFF
                else:
                    st, v = b.value(s)
                    if not st:
                        k += run + 1
                if not st and not ended and k > se:
                    ended = 1
        q = b.pos
        if st:
            eclean = nend if eclean is None else eclean
            if st == R.E_TRUNCATED or q >= u.T:
                at_end = True
                break
            q += 1
        elif ended:
            nend = min(nend + ended, CAP)
        if st or ended:
            slot = (slot + 1) % nslot
            k = 0 if dc else ss
    ex = (u.n, 0, slot, k) if at_end else (u.byte(q), q & 7, slot, k)
    return dict(exit=ex, nend=nend, eclean=eclean, dc=sums)


def first_pass(p, sc, S, max_rounds):
    """A cut first pass -> dict(rounds, accepted, entries [(byte, bit, slot, k)], before [blocks in front of every segment])."""
    u = Unit(scan_data(p, sc))
    nseg = -(-u.n // S)
    mcux, nmcu, slots = R.scan_mcus(p, sc["comps"])
    tabs = [D.code_table(*t) for t in sc["tables"]]
    expected = nmcu * len(slots)
    k0 = 0 if sc["ss"] == 0 else sc["ss"]
    entries = [(u.guess(s, S), 0, 0, k0) for s in range(nseg)]
    dirty, res, rounds, converged = [True] * nseg, [None] * nseg, 0, False
    while rounds < max_rounds:
        rounds += 1
        for s in range(nseg):
            if dirty[s]:
                res[s] = first_segment(u, sc, tabs, slots, entries[s], min((s + 1) * S, u.n))
        changed = False
        for s in range(nseg - 1, -1, -1):
            dirty[s] = s > 0 and res[s - 1]["exit"] != entries[s]
            if dirty[s]:
                entries[s] = res[s - 1]["exit"]
                changed = True
        if not changed:
            converged = True
            break
    before, done, bad, found = [], 0, False, False
    for s in range(nseg):
        before.append(done)
        r = res[s]
        if done < expected:
            if sc["ss"] == 0 and entries[s][2] != done % len(slots):
                bad = True
            last = expected - 1 - done
            if last < r["nend"]:
                if r["eclean"] is None or r["eclean"] > last:
                    found = True
                else:
                    bad = True
            elif r["eclean"] is not None:
                bad = True
        done = min(done + r["nend"], CAP)
    return dict(rounds=rounds, accepted=converged and found and not bad, entries=entries, before=before, unit=u, expected=expected)


def skim(p, sc, S, masks):
    """A cut AC refinement -> dict(accepted, entries [(data bit, block, k, run)]); masks[n]: bit k set where block n's coefficient at
    zigzag k, inside the band, has history."""
    u = Unit(scan_data(p, sc))
    nseg = -(-u.n // S)
    ss, se = sc["ss"], sc["se"]
    expected = R.scan_mcus(p, sc["comps"])[1]
    table = D.code_table(*sc["tables"][0])
    P = [0]
    for m in masks:
        P.append(P[-1] + bin(m).count("1"))
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
                j = next((x for x in range(1, rem + 1) if P[n + x] - P[n] >= target), rem)
            if not skip(P[n + j] - P[n]):
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
    """The sequential walk of jpegprog_ref over every scan of a file, with its own routines -> per scan dict(status, starts: the data
    bit at which every block of a ONE-unit scan starts (a block inside a first pass's EOB run: where the run left the reader),
    masks: for an AC refinement the history masks of its blocks BEFORE the scan).  The walk goes on behind a failing scan, as
    the device's does."""
    key = bytes(f)
    if key in _TRACE:
        return _TRACE[key]
    p = R.parse(key)
    g = D.geometry(p)
    d = p["data"]
    planes = [__import__("numpy").zeros((g["bh"][c], g["bw"][c], 64), "int16") for c in range(p["ncomp"])]
    out = []
    for sc in p["scans"]:
        st0, units, _ = D.scan(d[sc["off"]:], sc["units"])
        rec = dict(status=R.E_RESTART if st0 else R.OK, starts=[], masks=None)
        out.append(rec)
        if st0:
            continue
        blocks = scan_blocks(p, sc, planes)
        nslot = len(R.scan_mcus(p, sc["comps"])[2])
        nmcu = R.scan_mcus(p, sc["comps"])[1]
        ri = sc["ri"] or nmcu
        tabs = [D.code_table(*t) for t in sc["tables"]]
        slots = R.scan_mcus(p, sc["comps"])[2]
        if sc["ss"] and sc["ah"]:
            rec["masks"] = [sum(1 << k for k in range(sc["ss"], sc["se"] + 1) if blk[R.ZIGZAG[k]] != 0) for blk in blocks]
        s = d[sc["off"]:]
        for ku, (a, b) in enumerate(units):
            bits = D._Bits(s[a:b])
            pred, run, ust = [0, 0, 0], 0, R.OK
            for o in range(ku * ri * nslot, min((ku + 1) * ri, nmcu) * nslot):
                blk, t = blocks[o], slots[o % nslot][3]
                if len(units) == 1:
                    rec["starts"].append(bits.pos)
                if sc["ss"] == 0 and sc["ah"] == 0:
                    ust, pred[t] = R.dc_first(bits, tabs[t], pred[t], sc["al"], blk)
                elif sc["ss"] == 0:
                    ust = R.dc_refine(bits, sc["al"], blk)
                elif sc["ah"] == 0:
                    if run > 0:
                        run -= 1
                    else:
                        ust, run = R.ac_first(bits, tabs[0], sc["ss"], sc["se"], sc["al"], blk)
                else:
                    ust, run = R.ac_refine(bits, tabs[0], sc["ss"], sc["se"], sc["al"], run, blk)
                if ust:
                    break
            if ust and not rec["status"]:
                rec["status"] = ust
    _TRACE[key] = (p, out)
    return _TRACE[key]


def records(f, S, max_rounds):
    """Per scan (route, segments, rounds, accepted) as the device leaves them, and the routes' own results (None: not cut).  exact[i]:
    the record does not depend on coefficients a failing earlier scan left behind."""
    p, tr = trace(f)
    restart = any(t["status"] == R.E_RESTART for t in tr)
    recs, details, exact, failed = [], [], [], False
    for sc, (route, nseg), t in zip(p["scans"], plan(p, S), tr):
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
    return recs, details, exact
