"""numpy restatement of the JPEG decoder's scans-of-any-layout family (attwarp_amd/jpeg.py with ``all_scans=True``,
csrc/jpegscan_blocks.hpp, the jpegscan_* kernels of jpegdec.hip): the marker walk over all scans of a
progressive file of any layout or of a sequential file of several scans, with its refusals; the geometry of a scan over
the general MCU; the level rule; the entropy walk per scan with the four routines of jpegprog_ref and the sequential block
of jpegdec_ref; the statuses.  Coefficient planes become pixels through jpegfmt_ref, unchanged.  Also a TRANSCODER:
coefficient planes of a frame of any layout plus a scan script -> an SOF2 file, or an SOF0 file with full-band scans of
component subsets, with one fixed full-alphabet Huffman table per class.  Pinned to Pillow by test_jpegscan_ref_cpu.py."""
from __future__ import annotations

import struct

import numpy as np

import jpegdec_ref as D
import jpegfmt_ref as F
import jpegprog_ref as P
from jpegdec_ref import OK, E_RESTART, E_NO_EOI, ZIGZAG

MAX_SCANS = 64
MAX_UNITS = D.MAX_UNITS
MAX_SLOTS = 10


def scan_mcus(W, H, samp, comps):
    """(MCUs per row, MCUs, [(component, yy, xx, place in the scan)] per block of an MCU) of a scan over ``comps``: several
    components walk the FRAME's MCUs, one walks the blocks that cover its true size."""
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    if len(comps) == 1:
        h, v = samp[comps[0]]
        cw, ch = -(-W * h // hmax), -(-H * v // vmax)
        return -(-cw // 8), -(-cw // 8) * -(-ch // 8), [(comps[0], 0, 0, 0)]
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    return mcux, mcux * mcuy, [(c, yy, xx, t) for t, c in enumerate(comps) for yy in range(samp[c][1]) for xx in range(samp[c][0])]


def _segments(d):
    """The marker walk: yields (marker, payload, offset behind the segment); the caller sends back the offset to go on from
    behind a scan's data.  Ends at EOI or at the file's end behind a scan."""
    n, pos, scans = len(d), 2, False
    while True:
        if scans and pos + 1 >= n:
            return
        if pos >= n:
            raise OSError("jpeg: the file ends inside its headers")
        if d[pos] != 0xFF:
            raise ValueError("jpeg: a marker was expected")
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            if scans:
                return
            raise OSError("jpeg: the file ends inside its headers")
        m = d[pos]
        pos += 1
        if scans and m == 0xD9:
            return
        if m != 0xC2 and m in D._FRAMES:
            raise ValueError(f"jpeg: {D._FRAMES[m]} frame")
        if m in (0, 1, 0xD8, 0xD9, 0xCC) or 0xD0 <= m <= 0xD7:
            raise ValueError(f"jpeg: marker {m:02x} in the headers")
        if pos + 2 > n or pos + struct.unpack(">H", d[pos:pos + 2])[0] > n:
            if scans:
                return
            raise OSError("jpeg: the file ends inside its headers")
        L = struct.unpack(">H", d[pos:pos + 2])[0]
        if L < 2:
            raise ValueError("jpeg: segment length below 2")
        back = yield m, d[pos + 2:pos + L], pos + L
        pos = back if back is not None else pos + L
        scans = scans or m == 0xDA


def parse(data):
    """The walk over the whole file -> dict(W, H, ncomp, samp, color, qt, sequential, scans, cut, levels, first, units, data);
    every scan is dict(comps, ss, se, ah, al, seq, ri, dc, ac, off, units).  ValueError with the word of each refusal."""
    d = bytes(data)
    if d[:2] != b"\xff\xd8":
        raise ValueError("jpeg: bad signature")
    qts, dcs, acs, ri, jfif, adobe, frame = {}, {}, {}, 0, False, None, None
    scans, sent, latched, cut, mk, first = [], None, {}, False, None, None
    walk = _segments(d)
    back = None
    while True:
        try:
            m, seg, pos = walk.send(back) if back is not None else next(walk)
        except StopIteration:
            break
        back = None
        if m in (0xC0, 0xC1, 0xC2):
            if frame is not None:
                raise ValueError("jpeg: a second frame (hierarchical)")
            prec, H, W, nf = struct.unpack(">BHHB", seg[:6])
            if prec != 8:
                raise ValueError(f"jpeg: precision {prec}")
            if H == 0 or W == 0 or nf not in (1, 3, 4) or len(seg) != 6 + 3 * nf:
                raise ValueError("jpeg: size or components")
            frame = (m, W, H, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)])
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                counts = list(seg[q + 1:q + 17])
                (acs if seg[q] >> 4 else dcs)[seg[q] & 15] = (counts, list(seg[q + 17:q + 17 + sum(counts)]))
                q += 17 + sum(counts)
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                if seg[q] >> 4:
                    raise ValueError("jpeg: 16-bit quantisation table")
                t = [0] * 64
                for k in range(64):
                    t[ZIGZAG[k]] = seg[q + 1 + k]
                qts[seg[q] & 15] = t
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
            nf = len(comps)
            if sent is None:
                samp = [(c[1], c[2]) for c in comps] if nf > 1 else [(1, 1)]
                if any(not 1 <= f <= 4 for hv in samp for f in hv):
                    raise ValueError("jpeg: sampling factors outside 1..4")
                if sum(h * v for h, v in samp) > MAX_SLOTS:
                    raise ValueError(f"jpeg: {sum(h * v for h, v in samp)} blocks per MCU (at most {MAX_SLOTS})")
                hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
                if any(hmax % h or vmax % v for h, v in samp):
                    raise ValueError("jpeg: fractional up-sampling")
                if nf == 1:
                    color = "grey"
                elif nf == 3:
                    rgb = not jfif and (adobe == 0 if adobe is not None else bytes(c[0] for c in comps) == b"RGB")
                    color = "rgb" if rgb else "ycc"
                else:
                    color = "cmyk" if adobe in (None, 0) else "ycck"
                sent = [[None] * 64 for _ in range(nf)]
                mk = P.markers(d)
                first = pos
            if len(scans) >= MAX_SCANS:
                raise ValueError(f"jpeg: more than {MAX_SCANS} scans")
            ns = seg[0] if seg else 0
            if not 1 <= ns <= nf or len(seg) != 4 + 2 * ns:
                raise ValueError("jpeg: bad scan header")
            ids = [c[0] for c in comps]
            if any(seg[1 + 2 * i] not in ids for i in range(ns)):
                raise ValueError("jpeg: the scan names a component the frame does not have")
            ci = [ids.index(seg[1 + 2 * i]) for i in range(ns)]
            if any(b <= a for a, b in zip(ci, ci[1:])):
                raise ValueError("jpeg: the scan's components are not in frame order")
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            seq = sof != 0xC2
            if seq and (ss, se, ah, al) != (0, 63, 0, 0):
                raise ValueError("jpeg: spectral selection / successive approximation in a sequential file")
            if not seq and (ss > se or se > 63 or (ss == 0 and se != 0) or (ss > 0 and ns > 1) or al > 13 or (ah != 0 and al != ah - 1)):
                raise ValueError(f"jpeg: bad progression in a scan of {ns} component(s)")
            dc, ac = [], []
            for i, c in enumerate(ci):
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if seq:
                    if sent[c][0] is not None:
                        raise ValueError(f"jpeg: component {c} of a sequential file was already sent")
                    sent[c] = [0] * 64
                else:
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
                if seq or (ss == 0 and ah == 0):
                    if td not in dcs:
                        raise ValueError("jpeg: a table never defined")
                    dc.append(dcs[td])
                if seq or ss > 0:
                    if ta not in acs:
                        raise ValueError("jpeg: a table never defined")
                    ac.append(acs[ta])
            end = next((x for x in mk if x >= pos), len(d))
            nmcu = scan_mcus(W, H, samp, ci)[1]
            scans.append(dict(comps=ci, ss=ss, se=se, ah=ah, al=al, seq=seq, ri=ri, dc=dc, ac=ac, off=pos, units=-(-nmcu // ri) if ri else 1))
            cut = end + 1 >= len(d)
            back = end
    if not scans:
        raise OSError("jpeg: the file ends inside its headers")
    if not cut and any(a != 0 for row in sent for a in row):
        raise ValueError("jpeg: incomplete file: a component or coefficient never sent, or never down to Al = 0")
    units = sum(s["units"] for s in scans)
    p = dict(W=W, H=H, ncomp=nf, samp=samp, color=color, sequential=frame[0] != 0xC2, scans=scans, cut=cut, levels=P.levels(scans), first=first,
             units=units, ri=0, qt=[latched.get(c, qts.get(comps[c][3], [0] * 64)) for c in range(nf)], data=d)
    if units > MAX_UNITS or F.geometry(p)["nblocks"] >= D.MAX_BLOCKS:
        raise ValueError("jpeg: size limit")
    return p


def entropy(p):
    """-> (status, coefficient planes int16 [bh, bw, 64] per component (padded, as the device lays them out), info).
    E_RESTART from any scan first, then the status of the lowest failing (scan, unit), then E_NO_EOI."""
    g = F.geometry(p)
    d = p["data"]
    planes = [np.zeros((g["bh"][c], g["bw"][c], 64), np.int16) for c in range(p["ncomp"])]
    layout, eoi = [], False
    for sc in p["scans"]:
        st, units, e = D.scan(d[sc["off"]:], sc["units"])
        if st:
            return E_RESTART, planes, dict(eoi=e)
        layout.append(units)
        eoi = e
    first = OK
    for i, sc in enumerate(p["scans"]):
        mcux, nmcu, slots = scan_mcus(p["W"], p["H"], p["samp"], sc["comps"])
        ri = sc["ri"] or nmcu
        dct, act = [D.code_table(*t) for t in sc["dc"]], [D.code_table(*t) for t in sc["ac"]]
        s = d[sc["off"]:]
        for k, (a, b) in enumerate(layout[i]):
            bits = D._Bits(s[a:b])
            pred, run, ust = [0] * 4, 0, OK
            for m in range(k * ri, min((k + 1) * ri, nmcu)):
                mx, my = m % mcux, m // mcux
                for c, yy, xx, t in slots:
                    h, v = p["samp"][c]
                    blk = planes[c][my, mx] if len(sc["comps"]) == 1 else planes[c][my * v + yy, mx * h + xx]
                    if sc["seq"]:
                        blk[:] = 0                               # (the whole row is the scan's)
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
                if ust:
                    break
            if ust and not first:
                first = ust
        if first:
            break                                             # the lowest failing scan decides
    if first:
        return first, planes, dict(eoi=eoi)
    return (OK if eoi else E_NO_EOI), planes, dict(eoi=eoi)


_CACHE = {}


def decode(f, mode="RGB", order="rgb"):
    """A file -> (status, pixels [H, W, C] or None, info with crc (of the coefficients; 0 unless OK), units, levels, planes)."""
    key = bytes(f)
    if key not in _CACHE:
        p = parse(key)
        st, planes, info = entropy(p)
        info = dict(info, crc=D.coef_crc(planes) if st == OK else 0, units=p["units"], levels=p["levels"], planes=planes)
        _CACHE[key] = (p, st, F.idct_planes(p, planes) if st == OK else None, info)
    p, st, comp, info = _CACHE[key]
    if st:
        return st, None, info
    return st, F.pixels(p, comp, mode, order), info


# ---- the transcoder ------------------------------------------------------------------------------------------------------------------
IDS = {"grey": [1], "ycc": [1, 2, 3], "rgb": list(b"RGB"), "cmyk": list(b"CMYK"), "ycck": list(b"CMYK")}


def _encode_block_seq(w, blk, pred, dcc, acc):
    n, bits = P._magbits(int(blk[0]) - pred)
    w.put(dcc[n][1], dcc[n][0])
    w.put(bits, n)
    r = 0
    last = max([k for k in range(1, 64) if blk[ZIGZAG[k]]], default=0)
    for k in range(1, last + 1):
        v = int(blk[ZIGZAG[k]])
        if v == 0:
            r += 1
            continue
        while r > 15:
            w.put(acc[0xF0][1], acc[0xF0][0])
            r -= 16
        n, bits = P._magbits(v)
        w.put(acc[r << 4 | n][1], acc[r << 4 | n][0])
        w.put(bits, n)
        r = 0
    if last < 63:
        w.put(acc[0][1], acc[0][0])
    return int(blk[0])


def encode_scan(frame, planes, sc, ri, hack=None, index=0):
    """The entropy data of one scan (comps, ss, se, ah, al, seq) over the general MCU, restart markers included: the
    encoder of jpegprog_ref._encode_scan with this module's geometry and the sequential block.  hack: {(scan, block
    ordinal): [(value, bits)]} replaces a block's own bits."""
    W, H, samp = frame["W"], frame["H"], frame["samp"]
    comps, ss, se, ah, al, seq = sc
    mcux, nmcu, slots = scan_mcus(W, H, samp, comps)
    dcc, acc = P._codes(P.DC_TABLE), P._codes(P.AC_TABLE)
    out, w = b"", P._Writer()
    per = ri or nmcu
    pred = [0] * 4
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
            pred = [0] * 4
        mx, my = m % mcux, m // mcux
        for c, yy, xx, t in slots:
            h, v = samp[c]
            blk = planes[c][my, mx] if len(comps) == 1 else planes[c][my * v + yy, mx * h + xx]
            key = (index, ordinal)
            ordinal += 1
            if hack and key in hack:
                emit_eobrun()
                for val, n in hack[key]:
                    w.put(val, n)
                continue
            if seq:
                pred[t] = _encode_block_seq(w, blk, pred[t], dcc, acc)
            elif ss == 0 and ah == 0:
                cur = int(blk[0]) >> al
                n, bits = P._magbits(cur - pred[t])
                pred[t] = cur
                sym(dcc, n)
                w.put(bits, n)
            elif ss == 0:
                w.put((int(blk[0]) >> al) & 1, 1)
            elif ah == 0:
                r = 0
                for k in range(ss, se + 1):
                    val = int(blk[ZIGZAG[k]])
                    a = abs(val) >> al
                    if a == 0:
                        r += 1
                        continue
                    emit_eobrun()
                    while r > 15:
                        sym(acc, 0xF0)
                        r -= 16
                    n, bits = P._magbits(a if val >= 0 else -a)
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


def transcode(frame, planes, script, sequential=False, ri=None, table_ids=None, hack=None, eoi=True, cut=None):
    """``frame`` (W, H, samp, color, qt per component) with coefficient planes and a scan script -> a file.  Progressive
    (SOF2): script entries (comps, ss, se, ah, al).  ``sequential`` (SOF0): entries are component lists, each a full-band
    scan.  ri: restart interval per scan (None / 0: none; a DRI is written whenever it changes); table_ids: per scan the
    Huffman table id it defines in front of itself and names (default 0); cut = (scan, fraction): the file ends inside that
    scan's data."""
    nf, color = len(frame["samp"]), frame["color"]
    ids = IDS[color]
    out = b"\xff\xd8"
    if color in ("grey", "ycc"):
        out += b"\xff\xe0" + struct.pack(">H", 16) + b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
    else:
        out += b"\xff\xee" + struct.pack(">H", 14) + b"Adobe\0\x64\0\0\0\0" + bytes([2 if color == "ycck" else 0])
    for c in range(nf):
        out += b"\xff\xdb" + struct.pack(">H", 67) + bytes([c]) + bytes(frame["qt"][c][ZIGZAG[k]] for k in range(64))
    out += (b"\xff\xc0" if sequential else b"\xff\xc2") + struct.pack(">HBHHB", 8 + 3 * nf, 8, frame["H"], frame["W"], nf)
    for c, (h, v) in enumerate(frame["samp"]):
        out += bytes([ids[c], h << 4 | v, c])
    cur_ri = 0
    for i, entry in enumerate(script):
        comps, ss, se, ah, al = (list(entry), 0, 63, 0, 0) if sequential else entry
        r = (ri[i] if ri else 0) or 0
        if r != cur_ri:
            out += b"\xff\xdd" + struct.pack(">HH", 4, r)
            cur_ri = r
        th = table_ids[i] if table_ids else 0
        if sequential or (ss == 0 and ah == 0):
            out += P._dht(0, th, P.DC_TABLE)
        if sequential or ss > 0:
            out += P._dht(1, th, P.AC_TABLE)
        out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * len(comps), len(comps))
        for c in comps:
            out += bytes([ids[c], th << 4 | th])
        out += bytes([ss, se, ah << 4 | al])
        data = encode_scan(frame, planes, (comps, ss, se, ah, al, sequential), r, hack, i)
        if cut and cut[0] == i:
            at = int(len(data) * cut[1])
            while at and data[at - 1] == 0xFF:                # (never between an FF and what follows it)
                at -= 1
            return out + data[:at]
        out += data
    return out + (b"\xff\xd9" if eoi else b"")


def source_planes(f):
    """A one-scan sequential file of any layout -> (frame, coefficient planes) by the layout restatement."""
    p = F.parse(f)
    st, planes, _ = F.entropy(p)
    assert st == OK
    return dict(W=p["W"], H=p["H"], samp=p["samp"], color=p["color"], qt=p["qt"]), planes
