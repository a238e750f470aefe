"""Plain-Python restatement of the progressive JPEG decoder (attwarp_amd/jpeg.py, csrc/jpegprog_blocks.hpp, the jpegprog_*
kernels of csrc/jpegdec.hip): the marker walk over all scans with its refusals, scan geometry, the level
rule, the four block routines of T.81 G.1.2 / G.2 with counters of the branches taken, and the statuses.  Coefficients
become pixels through the IDCT, up-sampling and colour of tests/jpegdec_ref.py, imported unchanged.  Also a TRANSCODER:
the coefficients of a baseline file plus a scan script -> a progressive file, with one fixed full-alphabet Huffman table
per class.  Pinned to Pillow by tests/test_jpegprog_ref_cpu.py."""
from __future__ import annotations

import struct

import numpy as np

import jpegdec_ref as D
from jpegdec_ref import OK, E_TRUNCATED, E_HUFFMAN, E_COEFF, E_RESTART, E_NO_EOI, ZIGZAG

MAX_SCANS = 64
MAX_UNITS = D.MAX_UNITS

COUNT = {"corr_zrl": 0, "corr_eob": 0, "corr_place": 0, "max_eobrun": 0, "plus": 0, "minus": 0, "zrl_first": 0, "eob_first": 0,
         "dc_refine_set": 0}


def reset_counters():
    for k in COUNT:
        COUNT[k] = 0


def markers(d):
    """Offsets of every FF followed by neither 00 nor D0..D7 (the last byte: followed by nothing)."""
    return [i for i in range(len(d)) if d[i] == 0xFF and not (i + 1 < len(d) and (d[i + 1] == 0 or 0xD0 <= d[i + 1] <= 0xD7))]


def scan_mcus(p, comps):
    """(MCUs per row, MCUs, [(component, yy, xx, table)] per block of an MCU)."""
    hs, vs = p["hs"], p["vs"]
    if len(comps) == 1:
        c = comps[0]
        h, v = (hs, vs) if c == 0 else (1, 1)
        cw, ch = -(-p["W"] * h // hs), -(-p["H"] * v // vs)
        return -(-cw // 8), -(-cw // 8) * -(-ch // 8), [(c, 0, 0, 0)]
    mcux, mcuy = -(-p["W"] // (8 * hs)), -(-p["H"] // (8 * vs))
    slots = []
    for t, c in enumerate(comps):
        h, v = (hs, vs) if c == 0 else (1, 1)
        slots += [(c, yy, xx, t) for yy in range(v) for xx in range(h)]
    return mcux, mcux * mcuy, slots


def levels(scans):
    lv = []
    for i, a in enumerate(scans):
        dep = [lv[j] for j in range(i) if set(scans[j]["comps"]) & set(a["comps"]) and scans[j]["ss"] <= a["se"] and a["ss"] <= scans[j]["se"]]
        lv.append(max(dep) + 1 if dep else 0)
    return lv


def parse(data):
    """The marker walk over the whole file -> dict(W, H, ncomp, hs, vs, qt, scans, cut, levels, first); every scan is
    dict(comps, ss, se, ah, al, ri, tables, off, units).  ValueError with the word of each refusal."""
    d = bytes(data)
    n = len(d)
    if d[:2] != b"\xff\xd8":
        raise ValueError("jpeg: bad signature")
    pos, qts, dcs, acs, ri = 2, {}, {}, {}, 0
    frame, scans, sent, latched, cut, jfif, adobe = None, [], None, {}, False, False, None
    mk = None
    while True:
        if scans and pos + 1 >= n:
            break
        if pos >= n:
            raise OSError("jpeg: the file ends inside its headers")
        if d[pos] != 0xFF:
            raise ValueError("jpeg: a marker was expected")
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            if scans:
                break
            raise OSError("jpeg: the file ends inside its headers")
        m = d[pos]
        pos += 1
        if scans and m == 0xD9:
            break
        if m != 0xC2 and m in D._FRAMES:
            raise ValueError(f"jpeg: {D._FRAMES[m]} frame")
        if m in (0, 1, 0xD8, 0xD9, 0xCC) or 0xD0 <= m <= 0xD7:
            raise ValueError(f"jpeg: marker {m:02x} in the headers")
        if pos + 2 > n or pos + struct.unpack(">H", d[pos:pos + 2])[0] > n:
            if scans:
                break
            raise OSError("jpeg: the file ends inside its headers")
        L = struct.unpack(">H", d[pos:pos + 2])[0]
        if L < 2:
            raise ValueError("jpeg: segment length below 2")
        seg = d[pos + 2:pos + L]
        pos += L
        if m in (0xC0, 0xC1, 0xC2):
            if frame is not None:
                raise ValueError("jpeg: a second frame (hierarchical)")
            prec, H, W, nf = struct.unpack(">BHHB", seg[:6])
            if prec != 8 or H == 0 or W == 0 or nf not in (1, 3) or len(seg) != 6 + 3 * nf:
                raise ValueError("jpeg: precision, size or components")
            frame = (m, W, H, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)])
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                ns = sum(counts)
                left = 1
                for c in counts:
                    left = 2 * left - c
                    if left < 0:
                        raise ValueError("jpeg: DHT over-subscribed")
                if tc > 1 or th > 3 or len(counts) != 16 or ns > 256 or q + 17 + ns > len(seg):
                    raise ValueError("jpeg: bad DHT")
                syms = list(seg[q + 17:q + 17 + ns])
                if tc == 0 and any(s > 15 for s in syms):
                    raise ValueError("jpeg: DHT with a DC category above 15")
                (acs if tc else dcs)[th] = (counts, syms)
                q += 17 + ns
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq != 0 or tq > 3 or q + 65 > len(seg):
                    raise ValueError("jpeg: bad DQT (8-bit tables only)")
                t = [0] * 64
                for k in range(64):
                    t[ZIGZAG[k]] = seg[q + 1 + k]
                qts[tq] = t
                q += 65
        elif m == 0xDD:
            ri = struct.unpack(">H", seg)[0]
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\0"
        elif m == 0xEE:
            if seg[:5] == b"Adobe" and len(seg) >= 12:
                adobe = seg[11]
        elif m in (0xDC, 0xDE, 0xDF):
            raise ValueError("jpeg: DNL / hierarchical marker")
        elif m == 0xDA:
            if frame is None:
                raise ValueError("jpeg: SOS before the frame header")
            sof, W, H, comps = frame
            if sof != 0xC2:
                raise ValueError("jpeg: not a progressive file (the baseline restatement decodes it)")
            nf = len(comps)
            if sent is None:
                hs = vs = 1
                if nf == 3:
                    if adobe == 0 or (adobe is None and not jfif and bytes(c[0] for c in comps) == b"RGB"):
                        raise ValueError("jpeg: RGB-coded file")
                    samp = [(c[1], c[2]) for c in comps]
                    if samp[1] != (1, 1) or samp[2] != (1, 1) or samp[0] not in ((1, 1), (2, 1), (2, 2)):
                        raise ValueError(f"jpeg: sampling layout {samp}")
                    hs, vs = samp[0]
                sent = [[None] * 64 for _ in range(nf)]
                mk = markers(d)
                first = pos
            if len(scans) >= MAX_SCANS:
                raise ValueError(f"jpeg: more than {MAX_SCANS} scans")
            ns = seg[0]
            if not 1 <= ns <= nf or len(seg) != 4 + 2 * ns:
                raise ValueError("jpeg: bad scan header")
            ids = [c[0] for c in comps]
            ci = [ids.index(seg[1 + 2 * i]) if seg[1 + 2 * i] in ids else -1 for i in range(ns)]
            if -1 in ci or any(b <= a for a, b in zip(ci, ci[1:])):
                raise ValueError("jpeg: the scan's components are not the frame's, in frame order")
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            if ss > se or se > 63 or (ss == 0 and se != 0) or (ss > 0 and ns > 1) or al > 13 or (ah != 0 and al != ah - 1):
                raise ValueError("jpeg: bad progression")
            tables = []
            for i, c in enumerate(ci):
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if ss > 0 and sent[c][0] is None:
                    raise ValueError("jpeg: an AC scan before the component's DC")
                for k in range(ss, se + 1):
                    if ah == 0 and sent[c][k] is not None:
                        raise ValueError("jpeg: a first pass over a coefficient already sent")
                    if ah != 0 and sent[c][k] != ah:
                        raise ValueError("jpeg: a refinement that does not continue the coefficient's precision")
                    sent[c][k] = al
                if c not in latched:
                    if comps[c][3] not in qts:
                        raise ValueError("jpeg: a table never defined")
                    latched[c] = qts[comps[c][3]]
                if ah == 0 or ss > 0:
                    tabs, tid = (acs, ta) if ss > 0 else (dcs, td)
                    if tid not in tabs:
                        raise ValueError("jpeg: a table never defined")
                    tables.append(tabs[tid])
            end = next((x for x in mk if x >= pos), n)
            geo = dict(W=W, H=H, hs=hs, vs=vs)
            nmcu = scan_mcus(geo, ci)[1]
            scans.append(dict(comps=ci, ss=ss, se=se, ah=ah, al=al, ri=ri, tables=tables, off=pos, units=-(-nmcu // ri) if ri else 1))
            cut = end + 1 >= n
            pos = end
    if not cut and any(a != 0 for row in sent for a in row):
        raise ValueError("jpeg: incomplete progressive file")
    units = sum(s["units"] for s in scans)
    p = dict(W=W, H=H, ncomp=nf, hs=hs, vs=vs, ri=0, scans=scans, cut=cut, levels=levels(scans), first=first, units=units,
             qt=[latched.get(c, qts.get(comps[c][3], [0] * 64)) for c in range(nf)], data=d)
    g = D.geometry(p)
    if units > MAX_UNITS or g["nblocks"] >= D.MAX_BLOCKS:
        raise ValueError("jpeg: size limit")
    return p


# ---- the four block routines ---------------------------------------------------------------------------------------------------------
def _w16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def dc_first(bits, table, pred, al, blk):
    st, s = bits.symbol(table)
    if st:
        return st, pred
    st, v = bits.value(s & 15)
    if st:
        return st, pred
    pred = D._wrap32(pred + D.extend(v, s & 15))
    blk[0] = _w16((pred << al) & 0xFFFF)
    return OK, pred


def dc_refine(bits, al, blk):
    st, v = bits.value(1)
    if st:
        return st
    if v:
        COUNT["dc_refine_set"] += 1
        blk[0] = _w16((int(blk[0]) & 0xFFFF) | (1 << al))
    return OK


def ac_first(bits, table, ss, se, al, blk):
    """A block outside any EOB run -> (status, blocks BEHIND this one that the run covers)."""
    k = ss
    while k <= se:
        st, rs = bits.symbol(table)
        if st:
            return st, 0
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r == 15:
                if k + 16 > se + 1:
                    return E_COEFF, 0
                COUNT["zrl_first"] += 1
                k += 16
                continue
            st, v = bits.value(r)
            if st:
                return st, 0
            COUNT["eob_first"] += 1
            COUNT["max_eobrun"] = max(COUNT["max_eobrun"], (1 << r) + v)
            return OK, (1 << r) + v - 1
        k += r
        if k > se:
            return E_COEFF, 0
        st, v = bits.value(s)
        if st:
            return st, 0
        blk[ZIGZAG[k]] = _w16((D.extend(v, s) << al) & 0xFFFF)
        k += 1
    return OK, 0


def _correct(bits, al, blk, at, where):
    st, v = bits.value(1)
    if st:
        return st
    COUNT[where] += 1
    c = int(blk[at])
    if v and not (c & 0xFFFF) & (1 << al):
        blk[at] = _w16(((c & 0xFFFF) + (1 << al if c >= 0 else -(1 << al))) & 0xFFFF)
    return OK


def ac_refine(bits, table, ss, se, al, eobrun, blk):
    """-> (status, the blocks behind this one that the run covers).  eobrun on entry counts this block."""
    k = ss
    if eobrun == 0:
        while k <= se:
            st, rs = bits.symbol(table)
            if st:
                return st, 0
            r, s = rs >> 4, rs & 15
            place = 0
            if s:
                if s != 1:
                    return E_COEFF, 0
                st, v = bits.value(1)
                if st:
                    return st, 0
                COUNT["plus" if v else "minus"] += 1
                place = _w16((1 << al if v else -(1 << al)) & 0xFFFF)
            elif r != 15:
                st, v = bits.value(r)
                if st:
                    return st, 0
                eobrun = (1 << r) + v
                COUNT["max_eobrun"] = max(COUNT["max_eobrun"], eobrun)
                break
            found = False
            while k <= se:
                at = ZIGZAG[k]
                if blk[at] != 0:
                    st = _correct(bits, al, blk, at, "corr_place" if s else "corr_zrl")
                    if st:
                        return st, 0
                else:
                    r -= 1
                    if r < 0:
                        found = True
                        break
                k += 1
            if not found:
                return E_COEFF, 0
            if s:
                blk[ZIGZAG[k]] = place
            k += 1
    if eobrun > 0:
        while k <= se:
            at = ZIGZAG[k]
            if blk[at] != 0:
                st = _correct(bits, al, blk, at, "corr_eob")
                if st:
                    return st, 0
            k += 1
        eobrun -= 1
    return OK, eobrun


def entropy(p):
    """-> (status, coefficient planes int16 [bh, bw, 64] per component (padded, as the device lays them out), info)."""
    g = D.geometry(p)
    d = p["data"]
    planes = [np.zeros((g["bh"][c], g["bw"][c], 64), np.int16) for c in range(p["ncomp"])]
    layout, eoi = [], False
    for i, sc in enumerate(p["scans"]):
        st, units, e = D.scan(d[sc["off"]:], sc["units"])
        if st:
            return E_RESTART, planes, dict(eoi=e)
        layout.append(units)
        eoi = e
    first = OK
    for i, sc in enumerate(p["scans"]):
        mcux, nmcu, slots = scan_mcus(p, sc["comps"])
        ri = sc["ri"] or nmcu
        tabs = [D.code_table(*t) for t in sc["tables"]]
        s = d[sc["off"]:]
        for k, (a, b) in enumerate(layout[i]):
            bits = D._Bits(s[a:b])
            pred = [0, 0, 0]
            run, ust = 0, OK
            for m in range(k * ri, min((k + 1) * ri, nmcu)):
                mx, my = m % mcux, m // mcux
                for c, yy, xx, t in slots:
                    if len(slots) == 1:
                        blk = planes[c][my, mx]
                    else:
                        h, v = g["samp"][c]
                        blk = planes[c][my * v + yy, mx * h + xx]
                    if sc["ss"] == 0 and sc["ah"] == 0:
                        ust, pred[t] = dc_first(bits, tabs[t], pred[t], sc["al"], blk)
                    elif sc["ss"] == 0:
                        ust = dc_refine(bits, sc["al"], blk)
                    elif sc["ah"] == 0:
                        if run > 0:
                            run -= 1
                        else:
                            ust, run = ac_first(bits, tabs[0], sc["ss"], sc["se"], sc["al"], blk)
                    else:
                        ust, run = ac_refine(bits, tabs[0], sc["ss"], sc["se"], sc["al"], run, blk)
                    if ust:
                        break
                if ust:
                    break
            if ust and not first:
                first = ust
        if first:
            break                                     # the lowest failing scan decides
    info = dict(eoi=eoi)
    if first:
        return first, planes, info
    return (OK if eoi else E_NO_EOI), planes, info


_CACHE = {}


def decode(f, mode="RGB", order="rgb"):
    """A file -> (status, pixels [H, W, C] or None, info with crc (of the coefficients; 0 unless OK), units, levels)."""
    key = bytes(f)
    if key not in _CACHE:
        p = parse(key)
        st, planes, info = entropy(p)
        info = dict(info, crc=D.coef_crc(planes) if st == OK else 0, units=p["units"], levels=p["levels"], planes=planes)
        _CACHE[key] = (p, st, D.idct_planes(p, planes) if st == OK else None, info)
    p, st, comp, info = _CACHE[key]
    if st:
        return st, None, info
    return st, D.pixels(p, comp, mode, order), info


# ---- the transcoder ------------------------------------------------------------------------------------------------------------------
DC_TABLE = ([0, 0, 0, 15, 1] + [0] * 11, list(range(16)))
AC_TABLE = ([0] * 7 + [255, 1] + [0] * 7, list(range(256)))


def _codes(table):
    return {sym: (l, code) for (l, code), sym in D.code_table(*table).items()}


class _Writer:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]

    def flush(self):
        self.bits += [1] * (-len(self.bits) % 8)
        raw = np.packbits(np.array(self.bits, np.uint8)).tobytes() if self.bits else b""
        self.bits = []
        return raw.replace(b"\xff", b"\xff\x00")


def _magbits(v):
    a = abs(v)
    n = a.bit_length()
    return n, (v if v >= 0 else v + (1 << n) - 1)


def _encode_scan(p, planes, sc, ri, hack, index):
    """The entropy data of one scan, restart markers included.  hack: {(scan, block ordinal): [(value, bits)]} replaces a
    block's own bits."""
    g = D.geometry(p)
    mcux, nmcu, slots = scan_mcus(p, sc["comps"])
    ss, se, ah, al = sc["ss"], sc["se"], sc["ah"], sc["al"]
    dcc, acc = _codes(DC_TABLE), _codes(AC_TABLE)
    out, w = b"", _Writer()
    per = ri or nmcu
    pred = [0, 0, 0]
    state = dict(run=0, be=[])

    def sym(codes, s):
        l, code = codes[s]
        w.put(code, l)

    def emit_eobrun():
        if state["run"] > 0:
            nb = state["run"].bit_length() - 1
            sym(acc, nb << 4)
            if nb:
                w.put(state["run"] & ((1 << nb) - 1), nb)
            state["run"] = 0
        for b in state["be"]:
            w.put(b, 1)
        state["be"] = []

    ordinal = 0
    for m in range(nmcu):
        if m and m % per == 0:
            emit_eobrun()
            out += w.flush() + bytes([0xFF, 0xD0 + ((m // per - 1) & 7)])
            pred = [0, 0, 0]
        mx, my = m % mcux, m // mcux
        for c, yy, xx, t in slots:
            if len(slots) == 1:
                blk = planes[c][my, mx]
            else:
                h, v = g["samp"][c]
                blk = planes[c][my * v + yy, mx * h + xx]
            key = (index, ordinal)
            ordinal += 1
            if hack and key in hack:
                emit_eobrun()
                for v, n in hack[key]:
                    w.put(v, n)
                continue
            if ss == 0 and ah == 0:
                cur = int(blk[0]) >> al
                n, bits = _magbits(cur - pred[t])
                pred[t] = cur
                sym(dcc, n)
                w.put(bits, n)
            elif ss == 0:
                w.put((int(blk[0]) >> al) & 1, 1)
            elif ah == 0:
                r = 0
                for k in range(ss, se + 1):
                    v = int(blk[ZIGZAG[k]])
                    a = abs(v) >> al
                    if a == 0:
                        r += 1
                        continue
                    emit_eobrun()
                    while r > 15:
                        sym(acc, 0xF0)
                        r -= 16
                    n, bits = _magbits(a if v >= 0 else -a)
                    sym(acc, r << 4 | n)
                    w.put(bits, n)
                    r = 0
                if r > 0:
                    state["run"] += 1
                    if state["run"] == 0x7FFF:
                        emit_eobrun()
            else:
                absv = [abs(int(blk[ZIGZAG[k]])) >> al for k in range(64)]
                eob = max([k for k in range(ss, se + 1) if absv[k] == 1], default=0)
                r, br = 0, []
                for k in range(ss, se + 1):
                    a = absv[k]
                    if a == 0:
                        r += 1
                        continue
                    while r > 15 and k <= eob:
                        emit_eobrun()
                        sym(acc, 0xF0)
                        r -= 16
                        for b in br:
                            w.put(b, 1)
                        br = []
                    if a > 1:
                        br.append(a & 1)
                        continue
                    emit_eobrun()
                    sym(acc, r << 4 | 1)
                    w.put(0 if int(blk[ZIGZAG[k]]) < 0 else 1, 1)
                    for b in br:
                        w.put(b, 1)
                    br, r = [], 0
                if r > 0 or br:
                    state["run"] += 1
                    state["be"] += br
                    if state["run"] == 0x7FFF:
                        emit_eobrun()
    emit_eobrun()
    return out + w.flush()


def _dht(tc, th, table):
    body = bytes([tc << 4 | th]) + bytes(table[0]) + bytes(table[1])
    return b"\xff\xc4" + struct.pack(">H", 2 + len(body)) + body


def transcode(p, planes, script, ri=None, table_ids=None, hack=None, eoi=True, encode=True):
    """Frame ``p`` (W, H, ncomp, hs, vs, qt: a parse of jpegdec_ref) with coefficient planes and a scan script
    [(comps, ss, se, ah, al)] -> a progressive file.  ri: restart interval per scan (None / 0: none; a DRI is written
    whenever it changes); table_ids: per scan the Huffman table id it defines in front of itself and names (default 0);
    encode=False leaves every scan's data empty (for files the marker walk refuses)."""
    nf = p["ncomp"]
    out = b"\xff\xd8" + b"\xff\xe0" + struct.pack(">H", 16) + b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
    for c in range(nf):
        out += b"\xff\xdb" + struct.pack(">H", 67) + bytes([c]) + bytes(p["qt"][c][ZIGZAG[k]] for k in range(64))
    out += b"\xff\xc2" + struct.pack(">HBHHB", 8 + 3 * nf, 8, p["H"], p["W"], nf)
    for c in range(nf):
        h, v = (p["hs"], p["vs"]) if c == 0 else (1, 1)
        out += bytes([c + 1, h << 4 | v, c])
    cur_ri = 0
    for i, (comps, ss, se, ah, al) in enumerate(script):
        r = (ri[i] if ri else 0) or 0
        if r != cur_ri:
            out += b"\xff\xdd" + struct.pack(">HH", 4, r)
            cur_ri = r
        th = table_ids[i] if table_ids else 0
        if ss == 0 and ah == 0:
            out += _dht(0, th, DC_TABLE)
        elif ss > 0:
            out += _dht(1, th, AC_TABLE)
        out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * len(comps), len(comps))
        for c in comps:
            out += bytes([c + 1, th << 4 | th])
        out += bytes([ss, se, ah << 4 | al])
        if encode:
            out += _encode_scan(p, planes, dict(comps=comps, ss=ss, se=se, ah=ah, al=al), r, hack, i)
    return out + (b"\xff\xd9" if eoi else b"")


def baseline_planes(f):
    """A baseline file -> (its parse, its coefficient planes) by the baseline restatement."""
    p = D.parse(f)
    st, planes, _ = D.entropy(p)
    assert st == OK
    return p, planes
