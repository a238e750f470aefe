"""numpy restatement of the progressive JPEG files of the encoder (attwarp_amd/csrc/jpegprogenc_blocks.hpp, the jpegprogenc_*
kernels of jpegenc.hip): the bytes of ``Image.save(f, "JPEG", ..., progressive=True)``, which are
jpeg_simple_progression's script, the four block coders of the IJG library's published jcphuff.c, one optimal table per scan
(jpegopt_ref.optimal_table) and a DHT / DRI / SOS in front of every scan.  No Pillow in here;
tests/test_jpegprogenc_ref_cpu.py proves it against Pillow, the host and GPU tests prove the coders and the kernels against it.

A scan is coded into TOKENS first: ``("s", slot, symbol)`` is a Huffman symbol of table slot ``slot``, ``("b", value, n)``
are n raw bits, ``("r",)`` is the end of a restart interval.  The statistics pass counts the first kind, the second pass
turns all of them into bits: both see the same symbols, the ones a forced flush of the end-of-band run makes included.
``defect`` seeds exactly one wrong reading of the procedure, in this file only: the case list must notice each.
"""
import numpy as np

import jpegenc_ref as R
import jpegopt_ref as O

MAX_CORR_BITS = 1000
BE_LIMIT = MAX_CORR_BITS - 64 + 1     # 937: the run is flushed when more correction bits than this are pending
EOBRUN_MAX = 0x7fff
# (components, Ss, Se, Ah, Al); component 2 (Cr) comes before component 1 (Cb)
SCRIPT_COLOUR = (((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                 ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0))
SCRIPT_GREY = (((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0),
               ((0,), 1, 63, 1, 0))
DC1_SLOT = 10                         # table slots: slot i is scan i's table (scan 0: DC table 0), slot 10 the DC table of Cb / Cr
SLOTS = 11
# bits one block adds to a scan at most (jpegprogenc_blocks.hpp pe_block_bits)
EOBRUN_BITS = 16 + 14
DC_FIRST_BITS = 16 + 12
AC_FIRST_COEF_BITS = 16 + 10
AC_REFINE_BLOCK_BITS = EOBRUN_BITS + 63 * 17

DEFECTS = {
    "cb_before_cr": "the chroma scans come in the order Cb, Cr",
    "ac_dummy_blocks": "an AC scan walks the component's blocks padded to whole MCUs",
    "no_be_flush": "the run is not flushed when more than 937 correction bits are pending",
    "no_7fff_split": "the run is not flushed when it reaches 0x7FFF",
    "zrl_past_eob": "a refinement writes ZRL for sixteen zeros behind the last newly non-zero coefficient too",
    "corr_before_sign": "a refinement writes the buffered correction bits before the sign bit",
    "dri_repeated": "every scan gets a DRI",
    "dri_omitted": "only the first scan gets a DRI",
    "eobrun_across_restart": "the run is not flushed at a restart but carried into the next interval",
    "dc_shift_magnitude": "the DC first pass shifts the magnitude (rounds towards zero) instead of arithmetically",
}


def script(ncomp, defect=None):
    s = list(SCRIPT_COLOUR if ncomp == 3 else SCRIPT_GREY)
    if defect == "cb_before_cr" and ncomp == 3:
        s[2], s[3], s[7], s[8] = s[3], s[2], s[8], s[7]
    return s


def coefficients(a, quality, sub):
    """Per component [block rows, block columns, 64] zigzag coefficients, padded to whole MCUs (the padding blocks of luma
    are the dummy blocks of jpegenc_ref.scan_blocks: the DC of the block they repeat, no AC)."""
    ncomp = 1 if a.ndim == 2 else 3
    mcus, (hmax, vmax, mx, my) = R.scan_blocks(a, quality, sub)
    comps = [np.zeros((my * (vmax if c == 0 else 1), mx * (hmax if c == 0 else 1), 64), np.int64) for c in range(ncomp)]
    for m, mcu in enumerate(mcus):
        r, c = divmod(m, mx)
        for s, (ci, _, z) in enumerate(mcu):
            if ci == 0:
                comps[0][r * vmax + s // hmax, c * hmax + s % hmax] = z
            else:
                comps[ci][r, c] = z
    return comps, (hmax, vmax, mx, my)


def _nbits(v):
    return int(v).bit_length()


class _Run:
    """EOBRUN and the correction bits pending behind it (jcphuff.c's EOBRUN, BE and bit_buffer)."""

    def __init__(self, slot, tokens, defect, stats):
        self.slot, self.tokens, self.defect, self.stats = slot, tokens, defect, stats
        self.n, self.bits = 0, []

    def emit(self):
        if self.n > 0:
            nb = _nbits(self.n) - 1
            self.tokens.append(("s", self.slot, (nb << 4) & 0xff))
            if nb:
                self.tokens.append(("b", self.n & ((1 << nb) - 1), nb))
            self.n = 0
            self.tokens.extend(("b", b, 1) for b in self.bits)
            self.bits = []
            self.stats["eobruns"] += 1

    def end_block(self, own_bits=()):
        self.n += 1
        self.bits.extend(own_bits)
        if self.n == EOBRUN_MAX and self.defect != "no_7fff_split":
            self.stats["flush_7fff"] += 1
            self.emit()
        elif len(self.bits) > BE_LIMIT and self.defect != "no_be_flush":
            self.stats["flush_be"] += 1
            self.emit()


def _dc_first(blocks, al, tokens, defect):
    """blocks: [(component, DC slot, coefficient 0)] of one interval"""
    last = {}
    for ci, slot, v in blocks:
        v = int(v)
        t = (abs(v) >> al) * (1 if v >= 0 else -1) if defect == "dc_shift_magnitude" else v >> al
        d = t - last.get(ci, 0)
        last[ci] = t
        n = _nbits(abs(d))
        tokens.append(("s", slot, n))
        if n:
            tokens.append(("b", (d if d >= 0 else d - 1) & ((1 << n) - 1), n))


def _ac_first(z, ss, se, al, run, tokens):
    r = 0
    for k in range(ss, se + 1):
        v = int(z[k])
        t = abs(v) >> al
        if t == 0:
            r += 1
            continue
        run.emit()
        while r > 15:
            tokens.append(("s", run.slot, 0xf0))
            r -= 16
        n = _nbits(t)
        tokens.append(("s", run.slot, r << 4 | n))
        tokens.append(("b", (t if v >= 0 else ~t) & ((1 << n) - 1), n))
        r = 0
    if r > 0:
        run.end_block()


def _ac_refine(z, ss, se, al, run, tokens, defect):
    stats = run.stats
    absv = [abs(int(z[k])) >> al for k in range(64)]
    eob = 0
    for k in range(ss, se + 1):
        if absv[k] == 1:
            eob = k
    r, br = 0, []
    for k in range(ss, se + 1):
        t = absv[k]
        if t == 0:
            r += 1
            continue
        while r > 15 and (k <= eob or defect == "zrl_past_eob"):
            run.emit()
            tokens.append(("s", run.slot, 0xf0))
            r -= 16
            tokens.extend(("b", b, 1) for b in br)
            br = []
            stats["zrl_refine"] += 1
        if r > 15:
            stats["zrl_skipped"] += 1                         # sixteen zeros behind the last newly non-zero coefficient
        if t > 1:
            br.append(t & 1)
            continue
        run.emit()
        tokens.append(("s", run.slot, r << 4 | 1))
        sign = ("b", 0 if int(z[k]) < 0 else 1, 1)
        if defect != "corr_before_sign":
            tokens.append(sign)
        tokens.extend(("b", b, 1) for b in br)
        if defect == "corr_before_sign":
            tokens.append(sign)
        br, r = [], 0
    if r > 0 or br:
        run.end_block(br)


def component_blocks(H, W, ncomp, geom, ci):
    """(block columns, block rows) a single-component scan of component ci walks: its own, no dummy blocks."""
    hmax, vmax = geom[:2]
    fh, fv = (1, 1) if (ci == 0 or ncomp == 1) else (hmax, vmax)
    return -(-(-(-W // fh)) // 8), -(-(-(-H // fv)) // 8)


def scan_tokens(comps, geom, size, sc, index, restart_rows, defect=None, stats=None):
    """The tokens of scan ``index`` = ``sc`` and its restart interval in MCUs of the scan (0: none)."""
    H, W = size
    hmax, vmax, mx, my = geom
    cs, ss, se, ah, al = sc
    stats = stats if stats is not None else {}
    for key in ("eobruns", "flush_7fff", "flush_be", "zrl_refine", "zrl_skipped"):
        stats.setdefault(key, 0)
    tokens = []
    if len(cs) > 1:                                           # interleaved: MCUs, dummy blocks included
        per_row = mx
        walk = []
        for m in range(mx * my):
            r, c = divmod(m, mx)
            mcu = [(0, index, comps[0][r * vmax + by, c * hmax + bx]) for by in range(vmax) for bx in range(hmax)]
            mcu += [(ci, DC1_SLOT, comps[ci][r, c]) for ci in cs[1:]]
            walk.append(mcu)
    else:                                                     # the component's own blocks in raster order, one per "MCU"
        ci = cs[0]
        wc, hc = component_blocks(H, W, len(comps), geom, ci)
        if defect == "ac_dummy_blocks" and ss > 0:
            hc, wc = comps[ci].shape[:2]
        per_row = wc
        walk = [[(ci, index, comps[ci][r, c])] for r in range(hc) for c in range(wc)]
    interval = restart_rows * per_row
    if interval > 65535:
        raise ValueError(f"restart interval {interval} of scan {index} (at most 65535; libjpeg would clamp it there)")
    step = interval or len(walk)
    run = _Run(index, tokens, defect, stats)
    for m0 in range(0, len(walk), step):
        part = walk[m0:m0 + step]
        if ss == 0 and ah == 0:
            _dc_first([(ci, slot, z[0]) for mcu in part for ci, slot, z in mcu], al, tokens, defect)
        elif ss == 0:
            tokens.extend(("b", (int(z[0]) >> al) & 1, 1) for mcu in part for _, _, z in mcu)
        else:
            # blocks whose band holds nothing at this precision take a short cut (large flat images)
            band = np.abs(np.stack([mcu[0][2][ss:se + 1] for mcu in part])) >> al
            busy = band.any(axis=1)
            for mcu, b in zip(part, busy):
                z = mcu[0][2]
                if not b:
                    run.end_block()
                elif ah == 0:
                    _ac_first(z, ss, se, al, run, tokens)
                else:
                    _ac_refine(z, ss, se, al, run, tokens, defect)
        if defect != "eobrun_across_restart" or m0 + step >= len(walk):
            run.emit()
        tokens.append(("r",))
    return tokens, interval


def _dht_class(slot, sc):
    if slot == DC1_SLOT:
        return 0x01
    cs, ss = sc[0], sc[1]
    if ss == 0:
        return 0x00
    return 0x10 if cs[0] == 0 else 0x11


def frame_header(H, W, ncomp, quality, sub):
    """SOI .. SOF2: jpegenc_ref.header's without the tables and the scan, the frame marked progressive."""
    h = R.header(H, W, ncomp, quality, sub, 0)
    at = h.index(b"\xff\xc0")
    end = at + 2 + int.from_bytes(h[at + 2:at + 4], "big")
    return h[:at] + b"\xff\xc2" + h[at + 2:end]


def scan_slots(sc, index):
    """The table slots whose DHT goes in front of the scan."""
    cs, ss, se, ah, al = sc
    if ss == 0 and ah:
        return []
    return [index, DC1_SLOT] if len(cs) > 1 else [index]


def sos_segment(sc):
    cs, ss, se, ah, al = sc
    out = b"\xff\xda" + (6 + 2 * len(cs)).to_bytes(2, "big") + bytes([len(cs)])
    for ci in cs:
        td = min(ci, 1) if (ss == 0 and ah == 0) else 0
        ta = min(ci, 1) if ss > 0 else 0
        out += bytes([ci + 1, td << 4 | ta])
    return out + bytes([ss, se, ah << 4 | al])


def encode(img, quality=75, subsampling="4:2:0", restart_rows=0, order="rgb", defect=None, info=None):
    """uint8 [H,W] / [H,W,1] / [H,W,3] -> the progressive file's bytes.  ``info`` receives ``hist`` (slot -> counts),
    ``tables``, ``intervals`` (per scan), ``dri`` (the values written), ``scan_bytes``, the run statistics ``eobruns`` /
    ``flush_7fff`` / ``flush_be`` / ``zrl_refine`` / ``zrl_skipped``, ``depths`` (slot -> depth before limiting), ``tokens``, ``comps`` and ``interval_bits`` (per scan the unpadded bits of its intervals)."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or 0 in a.shape:
        raise ValueError(f"uint8 [H,W] / [H,W,1] / [H,W,3] expected, got {a.dtype} {a.shape}")
    if subsampling not in R.SUBSAMPLINGS:
        raise ValueError(f"unknown subsampling {subsampling!r}")
    a = O._prepared(a, order)
    H, W = a.shape[:2]
    ncomp = 1 if a.ndim == 2 else 3
    comps, geom = coefficients(a, quality, subsampling)
    sc_list = script(ncomp, defect)
    stats = {}
    scans = [scan_tokens(comps, geom, (H, W), sc, i, restart_rows, defect, stats) for i, sc in enumerate(sc_list)]
    hist = np.zeros((SLOTS, 256), np.int64)
    for tokens, _ in scans:
        for t in tokens:
            if t[0] == "s":
                hist[t[1], t[2]] += 1
    tables, codes, depths = {}, {}, {}
    for i, sc in enumerate(sc_list):
        for slot in scan_slots(sc, i):
            extra = {}
            tables[slot] = O.optimal_table(hist[slot], info=extra)
            depths[slot] = extra["depth"]
            codes[slot] = R.huffman_codes(*tables[slot])
    out = bytearray(frame_header(H, W, ncomp, quality, subsampling))
    last_dri, dris, scan_bytes, interval_bits = 0, [], [], []
    for i, (sc, (tokens, interval)) in enumerate(zip(sc_list, scans)):
        start = len(out)
        for slot in scan_slots(sc, i):
            out += O.dht_segment(_dht_class(slot, sc), *tables[slot])
        write_dri = interval != last_dri
        if defect == "dri_repeated":
            write_dri = interval != 0
        if defect == "dri_omitted":
            write_dri = interval != 0 and i == 0
        if write_dri:
            out += b"\xff\xdd\x00\x04" + interval.to_bytes(2, "big")
            last_dri = interval
            dris.append(interval)
        out += sos_segment(sc)
        bits, nint, lens = [], 0, []
        for t in tokens:
            if t[0] == "s":
                c, n = codes[t[1]][t[2]]
                bits.append(format(c, f"0{n}b"))
            elif t[0] == "b":
                bits.append(format(t[1], f"0{t[2]}b"))
            else:
                s = "".join(bits)
                lens.append(len(s))
                s += "1" * (-len(s) % 8)
                data = int(s, 2).to_bytes(len(s) // 8, "big") if s else b""
                if nint:
                    out += bytes([0xff, 0xd0 + (nint - 1) % 8])
                out += data.replace(b"\xff", b"\xff\x00")
                bits = []
                nint += 1
        scan_bytes.append(len(out) - start)
        interval_bits.append(lens)
    out += b"\xff\xd9"
    if info is not None:
        info.update(stats, hist=hist, depths=depths, tables=tables, dri=dris, scan_bytes=scan_bytes, geometry=geom, ncomp=ncomp,
                    intervals=[iv for _, iv in scans], tokens=[t for t, _ in scans], comps=comps, interval_bits=interval_bits)
    return bytes(out)


def scan_geometry(H, W, ncomp, sub, restart_rows):
    """Per scan (blocks, blocks per interval, intervals, bits a block adds at most, DHTs, components): what the planner
    sizes from."""
    geom = R.geometry(H, W, ncomp, sub)
    hmax, vmax, mx, my = geom
    bpm = hmax * vmax + 2 if ncomp == 3 else 1
    out = []
    for i, sc in enumerate(script(ncomp)):
        cs, ss, se, ah, al = sc
        if len(cs) > 1:
            per_row, rows, per_mcu = mx, my, bpm
        else:
            per_row, rows = component_blocks(H, W, ncomp, geom, cs[0])
            per_mcu = 1
        nblk = per_row * rows * per_mcu
        step = restart_rows * per_row * per_mcu or nblk
        if ss == 0:
            bpb = 1 if ah else DC_FIRST_BITS
        elif ah == 0:
            bpb = EOBRUN_BITS + (se - ss + 1) * AC_FIRST_COEF_BITS
        else:
            bpb = AC_REFINE_BLOCK_BITS
        out.append((nblk, step, -(-nblk // step), bpb, len(scan_slots(sc, i)), len(cs)))
    return out


def interval_bound_bits(nblocks, bpb):
    """Bits an interval of nblocks blocks takes at most: every block at its bound and one more run symbol at the end."""
    return nblocks * bpb + EOBRUN_BITS


def bound(H, W, ncomp, quality=75, sub="4:2:0", restart_rows=0):
    """attwarp_jpegenc_bound_prog: SOI .. SOF2; per scan its DHTs at 277 bytes, a DRI, the SOS, every interval at its bound,
    every byte stuffed, a marker behind it; EOI."""
    n = len(frame_header(H, W, ncomp, quality, sub))
    for nblk, step, nint, bpb, ndht, nc in scan_geometry(H, W, ncomp, sub, restart_rows):
        n += 277 * ndht + 6 + 6 + 2 * nc
        full, rest = divmod(nblk, step)
        n += full * (2 * ((interval_bound_bits(step, bpb) + 7) // 8) + 2)
        if rest:
            n += 2 * ((interval_bound_bits(rest, bpb) + 7) // 8) + 2
    return n + 2
