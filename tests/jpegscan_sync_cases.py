"""Files for the sub-streams of the scans-of-every-layout family (test_jpegscan_sync_ref_cpu.py,
test_jpegscan_sync_host_cpu.py, test_jpegscan_sync_gpu.py), built at run time with Pillow and the transcoder of jpegscan_ref.
Files are small (about 96 pixels a side; the two constructions that need 272 and 512 blocks of ONE chroma component are
larger) and busy: their coefficient blocks come from a quality-100 noise picture, so that scans are several 32-byte segments
long, and every cut first pass stays below 63 segments, which the rounds settle for certain (segment k's entry is true
after k rounds; Pillow's own quality-100 files are therefore 48 pixels a side).  Every builder asserts, from the file's own bytes, the property its name claims: a case that stops having
it fails on the CPU."""
from __future__ import annotations

import functools
import struct

import numpy as np

import jpegdec_cases as C
import jpegfmt_cases as L
import jpegscan_cases as SC
import jpegscan_ref as R
from jpegscan_ref import P, ZIGZAG

S = 32                                                    # the segment size every case is built for
MAX_FIRST_SEGMENTS = 62                                   # of a cut first pass: fewer than max_rounds - 1 = 63


def kind(sc):
    """JP_DC_FIRST, JP_DC_REFINE, JP_AC_FIRST, JP_AC_REFINE, JS_SEQUENTIAL."""
    return 4 if sc["seq"] else (2 if sc["ss"] else 0) + (1 if sc["ah"] else 0)


def scan_bytes(f):
    """[(scan of the parse, its entropy data up to the first marker)]."""
    p = R.parse(f)
    mk = P.markers(p["data"])
    return [(sc, bytes(p["data"][sc["off"]:next((x for x in mk if x >= sc["off"]), len(p["data"]))])) for sc in p["scans"]]


def table_key(t):
    return tuple(t[0]), tuple(t[1][:sum(t[0])])


def period(f, scan):
    """The period of scan `scan`'s DC table sequence, from the file: the smallest divisor of the blocks per MCU whose tables repeat."""
    p = R.parse(f)
    sc = p["scans"][scan]
    slots = R.scan_mcus(p["W"], p["H"], p["samp"], sc["comps"])[2]
    seq = [table_key(sc["dc"][t]) for _, _, _, t in slots]
    n = len(seq)
    return next(q for q in range(1, n + 1) if n % q == 0 and all(seq[j] == seq[j + q] for j in range(n - q))), seq


@functools.lru_cache(None)
def _pool():
    """Coefficient blocks of a quality-100 noise picture and the picture's quantisation table."""
    _, frame, planes = SC.source("cmyk_q100", 96, 96, 3)
    return np.concatenate([pl.reshape(-1, 64) for pl in planes]), frame["qt"]


def frame_of(samp, color, W, H, seed=0, fill=True, ac=8):
    """(frame, padded coefficient planes) of a layout, the planes filled with pool blocks (or zero) cut off behind zigzag
    position `ac`: an AC first pass over all 63 coefficients of such blocks would be hundreds of segments, and without
    end-of-block symbols its states do not settle."""
    pool, qt = _pool()
    pool = pool.copy()
    pool[:, [ZIGZAG[k] for k in range(ac + 1, 64)]] = 0
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    planes = []
    for c, (h, v) in enumerate(samp):
        n = mcuy * v * mcux * h
        blocks = np.resize(np.roll(pool, 37 * seed + 11 * c, axis=0), (n, 64)) if fill else np.zeros((n, 64), np.int16)
        planes.append(np.ascontiguousarray(blocks).reshape(mcuy * v, mcux * h, 64).astype(np.int16))
    return dict(W=W, H=H, samp=list(samp), color=color, qt=[qt[c % len(qt)] for c in range(len(samp))]), planes


def approximation(nf, dc=None):
    """DC (the scans `dc`, default one interleaved) with Al = 1, AC with Al = 1 and a refinement each, the DC refined the same way."""
    a = list(range(nf))
    dc = dc or [a]
    return ([(c, 0, 0, 0, 1) for c in dc] + [([c], 1, 63, 0, 1) for c in a] + [([c], 1, 63, 1, 0) for c in a] + [(c, 0, 0, 1, 0) for c in dc])


def _check_good(name, f, want_kinds=()):
    """Every cut first pass (DC or AC: both settle by rounds) below 63 segments; the kinds the case is for are cut."""
    cut = set()
    for sc, d in scan_bytes(f):
        if sc["units"] == 1 and len(d) >= 2 * S and kind(sc) != 4:
            cut.add(kind(sc))
            assert kind(sc) not in (0, 2) or -(-len(d) // S) <= MAX_FIRST_SEGMENTS, (name, kind(sc), len(d))
    assert set(want_kinds) <= cut, (name, cut)
    return f


# ---- the period ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def shared_table():
    """[(name, file)]: Pillow's progressive CMYK (4:4:4 and 4:2:0) and YCCK: all components on ONE DC table, period 1."""
    out = [("pil_cmyk_444", L.write_cmyk(C.noise(48, 40, 4, 5), quality=100, subsampling=0, progressive=True)),
           ("pil_cmyk_420", L.write_cmyk(C.noise(56, 40, 4, 6), quality=100, subsampling=2, progressive=True))]
    ycck = L.write_cmyk(C.noise(40, 56, 4, 7), quality=100, subsampling=2, progressive=True)
    out.append(("pil_ycck_420", C.edit(ycck, lambda s: C.replace(s, 0xEE, lambda pl: pl[:11] + b"\x02"))))
    for name, f in out:
        p = R.parse(f)
        assert len(p["scans"][0]["comps"]) == 4 and kind(p["scans"][0]) == 0 and p["color"] == ("ycck" if "ycck" in name else "cmyk"), name
        assert period(f, 0)[0] == 1 and len(scan_bytes(f)[0][1]) >= 2 * S, name
        _check_good(name, f, (0, 2, 3))
    return out


def dc_tables(n):
    """n DC tables of different content, each a full alphabet: P.DC_TABLE with its symbols rotated."""
    counts, syms = P.DC_TABLE
    return [(list(counts), syms[t:] + syms[:t]) for t in range(n)]


def transcode_dc(frame, planes, script, tables):
    """jpegscan_ref.transcode for a script whose DC first passes take the table `tables[c]` for component c (defined under the
    id c in front of the scan); every other scan is the transcoder's own."""
    whole = R.transcode(frame, planes, script)
    p = R.parse(whole)
    out = bytearray(whole[:whole.index(b"\xff\xc4")])         # everything in front of the first DHT
    ids = R.IDS[frame["color"]]
    own = scan_bytes(whole)
    assert len(p["scans"]) == len(script)
    for i, (comps, ss, se, ah, al) in enumerate(script):
        if not (ss == 0 and ah == 0):
            out += (P._dht(1, 0, P.AC_TABLE) if ss > 0 else b"") + b"\xff\xda" + struct.pack(">HB", 6 + 2 * len(comps), len(comps))
            out += b"".join(bytes([ids[c], 0]) for c in comps) + bytes([ss, se, ah << 4 | al])
            out += own[i][1]
            continue
        for c in comps:
            out += P._dht(0, c, tables[c])
        out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * len(comps), len(comps)) + b"".join(bytes([ids[c], c << 4]) for c in comps) + bytes([0, 0, al])
        codes = [P._codes(tables[c]) for c in range(len(tables))]
        mcux, nmcu, slots = R.scan_mcus(frame["W"], frame["H"], frame["samp"], comps)
        w, pred = P._Writer(), [0] * 4
        for m in range(nmcu):
            mx, my = m % mcux, m // mcux
            for c, yy, xx, t in slots:
                h, v = frame["samp"][c]
                blk = planes[c][my, mx] if len(comps) == 1 else planes[c][my * v + yy, mx * h + xx]
                cur = int(blk[0]) >> al
                n, bits = P._magbits(cur - pred[t])
                pred[t] = cur
                w.put(codes[c][n][1], codes[c][n][0])
                w.put(bits, n)
        out += w.flush()
    return bytes(out) + b"\xff\xd9"


@functools.lru_cache(None)
def table_sequences():
    """[(name, file, period)]: four-component files whose DC tables are all distinct (period = blocks per MCU, also with a 2 x 1
    first component), and repeat as A B A B (period 2)."""
    t = dc_tables(4)
    out = []
    for name, samp, tabs, want in (("distinct_1111", [(1, 1)] * 4, t, 4), ("distinct_2111", [(2, 1), (1, 1), (1, 1), (1, 1)], t, 5),
                                   ("repeating_abab", [(1, 1)] * 4, [t[0], t[1], t[0], t[1]], 2)):
        frame, planes = frame_of(samp, "cmyk", 72, 64, len(out))
        f = transcode_dc(frame, planes, approximation(4), tabs)
        assert period(f, 0)[0] == want and len(period(f, 0)[1]) == sum(h * v for h, v in samp), name
        assert len({table_key(x) for x in R.parse(f)["scans"][0]["dc"]}) == len({table_key(x) for x in tabs}), name
        assert R.decode(f)[2]["crc"] == R.decode(R.transcode(frame, planes, approximation(4)))[2]["crc"], name
        out.append((name, _check_good(name, f, (0, 2, 3)), want))
    return out


@functools.lru_cache(None)
def pillow_440():
    """Pillow's progressive 4:2:2 turned 4:4:0 by its frame header: DC tables 0 0 1 1 over the four blocks of an MCU.  (Quality 97:
    at 100 no size has both a DC scan of two segments and a luma scan below 63.)"""
    f = C.edit(C.write(C.noise(72, 48, 3, 9), quality=97, subsampling=1, progressive=True), SC._resized(48, 72, 0x12))
    p = R.parse(f)
    per, seq = period(f, 0)
    assert p["samp"] == [(1, 2), (1, 1), (1, 1)] and seq[0] == seq[1] != seq[2] == seq[3] and per == 4
    return _check_good("pil_440", f, (0, 2, 3))


# ---- the geometry -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def ten_blocks():
    """Ten blocks per MCU in a four-component frame: an interleaved DC first pass and an interleaved DC refinement, both cut."""
    frame, planes = frame_of([(2, 2), (1, 1), (1, 1), (2, 2)], "ycck", 128, 112, 4, ac=4)
    f = R.transcode(frame, planes, approximation(4))
    p = R.parse(f)
    assert len(R.scan_mcus(p["W"], p["H"], p["samp"], p["scans"][0]["comps"])[2]) == 10
    by = {(kind(sc), len(sc["comps"])): len(d) for sc, d in scan_bytes(f)}
    assert by[(0, 4)] >= 2 * S and by[(1, 4)] >= 2 * S, by
    return _check_good("ten_blocks", f, (0, 1, 2, 3))


@functools.lru_cache(None)
def subsets():
    """[(name, file)]: interleaved DC scans over a subset of the components; the component left out is the one with h v > 1,
    so the scan's MCU is smaller than the frame's and it still walks the frame's MCU grid."""
    out = []
    for name, samp, dc in (("subset_02_of_k2x2", [(1, 1), (1, 1), (1, 1), (2, 2)], [[0, 2], [1], [3]]),
                           ("subset_123_of_c2x2", [(2, 2), (1, 1), (1, 1), (1, 1)], [[1, 2, 3], [0]])):
        frame, planes = frame_of(samp, "cmyk", 96, 88, 7 + len(out))
        f = R.transcode(frame, planes, approximation(4, dc))
        p = R.parse(f)
        sc, d = scan_bytes(f)[0]
        left = [c for c in range(4) if c not in sc["comps"]]
        assert sc["comps"] == dc[0] and any(samp[c][0] * samp[c][1] > 1 for c in left) and all(samp[c] == (1, 1) for c in sc["comps"]), name
        assert R.scan_mcus(p["W"], p["H"], samp, sc["comps"])[1] == 6 * 6 and len(d) >= 2 * S, name
        last = scan_bytes(f)[-len(dc)]
        assert kind(last[0]) == 1 and last[0]["comps"] == dc[0], name
        out.append((name, _check_good(name, f, (0, 2, 3))))
    return out


@functools.lru_cache(None)
def padded_plane():
    """The luma of a 72 x 96 4:1:1 frame alone in its scans: 9 covering blocks per row at the padded plane's pitch of 12.  A DC
    first pass, an AC first pass and an AC refinement of it, all cut."""
    frame, planes = frame_of([(4, 1), (1, 1), (1, 1)], "ycc", 72, 96, 9)
    f = R.transcode(frame, planes, approximation(3, [[0], [1, 2]]))
    p = R.parse(f)
    assert R.scan_mcus(72, 96, p["samp"], [0])[0] == 9 and planes[0].shape[1] == 12
    mine = {kind(sc) for sc, d in scan_bytes(f) if sc["comps"] == [0] and len(d) >= 2 * S}
    assert {0, 2, 3} <= mine, mine
    return _check_good("padded_411", f, (0, 2, 3))


# ---- the boundary constructions of jpegprog_sync_cases on component 1 of a 2 x 2 sub-sampled CMYK frame ---------------------------
CHROMA = [(2, 2), (1, 1), (1, 1), (1, 1)]


def _chroma(bh, bw, qt=1):
    """(frame, planes) of a CMYK frame whose component 1 is bh x bw blocks, all coefficients zero."""
    frame, planes = frame_of(CHROMA, "cmyk", 16 * bw, 16 * bh, fill=False)
    frame["qt"] = [[qt] * 64] * 4
    return frame, planes


def _script(dc_al=0, refine=False):
    """DC interleaved, then component 1's AC (Al = 1 and its refinement with `refine`), then the other components' AC."""
    a = [0, 1, 2, 3]
    one = [([1], 1, 63, 0, 1), ([1], 1, 63, 1, 0)] if refine else [([1], 1, 63, 0, 0)]
    return [(a, 0, 0, 0, dc_al)] + one + [([c], 1, 63, 0, 0) for c in (0, 2, 3)] + ([(a, 0, 0, 1, 0)] if dc_al else [])


@functools.lru_cache(None)
def straddle():
    """Noise of +-1 and a few +-3 in every AC coefficient of component 1: more than 65 bytes of refinement per block, so a
    block touches three 32-byte segments or more."""
    frame, planes = _chroma(4, 4)
    rng = np.random.default_rng(21)
    planes[1][:, :, 1:] = rng.choice(np.array([-1, 1], np.int16), (4, 4, 63))
    planes[1][:, :, 7::13] *= 3
    planes[1][:, :, 0] = 10
    f = R.transcode(frame, planes, _script(refine=True))
    sc, d = scan_bytes(f)[2]
    assert kind(sc) == 3 and sc["comps"] == [1] and len(d) / 16 > 65, len(d)
    return f


@functools.lru_cache(None)
def eob_boundary():
    """Component 1's AC refinement opens with an EOB run of 8 blocks: 8 + 3 bits of symbol, 245 correction bits of blocks 0..3,
    none of blocks 4..7 (no history), so the run ends at bit 256, the first bit of segment 1."""
    frame, planes = _chroma(4, 4)
    a = planes[1].reshape(16, 64)
    a[:, 0] = 16
    for b, n in enumerate((61, 61, 61, 62)):
        a[b, [ZIGZAG[k] for k in range(1, 1 + n)]] = 2        # history, correction bit 0
    for b in range(8, 16):
        a[b, [ZIGZAG[k] for k in range(1, 31)]] = 1           # thirty new coefficients each: the scan runs on
    f = R.transcode(frame, planes, _script(refine=True))
    sc, d = scan_bytes(f)[2]
    assert kind(sc) == 3 and sc["comps"] == [1] and d[:32] == bytes([0x30]) + bytes(31) and len(d) >= 2 * S, d[:34].hex()
    return f


@functools.lru_cache(None)
def ac_first_overshoot():
    """The last block of component 1's AC first pass is an EOB run of 15 blocks: it overshoots the last block by 14."""
    frame, planes = _chroma(6, 6, qt=3)
    rng = np.random.default_rng(5)
    planes[1][:, :, :] = rng.integers(-6, 7, planes[1].shape)
    planes[1][:, :, [ZIGZAG[k] for k in range(21, 64)]] = 0    # (twenty coefficients a block: the scan stays below 63 segments)
    planes[1][-1, -1, 1:] = 0
    f = R.transcode(frame, planes, _script(), hack={(1, 35): [(0x30, 8), (7, 3)]})
    g = R.transcode(frame, planes, _script())
    assert R.decode(f)[0] == 0 and R.decode(g)[2]["crc"] == R.decode(f)[2]["crc"] and f != g
    sc, d = scan_bytes(f)[1]
    assert kind(sc) == 2 and sc["comps"] == [1] and len(d) >= 2 * S
    return f


def _dc_refine_script():
    return [([0, 1, 2, 3], 0, 0, 0, 1), ([1], 0, 0, 1, 0), ([0, 2, 3], 0, 0, 1, 0)] + [([c], 1, 63, 0, 0) for c in range(4)]


@functools.lru_cache(None)
def dc_refine_ones(first_zero):
    """Component 1's DC refinement is all one bits: every data byte an FF 00 pair; 68 raw bytes, the boundary at 32 on the FF of
    a pair.  first_zero: block 0's bit is zero, so the first byte is 7F and the boundary lies on the 00 of a pair."""
    frame, planes = _chroma(17, 16)
    planes[1][:, :, 0] = 5
    if first_zero:
        planes[1][0, 0, 0] = 4
    f = R.transcode(frame, planes, _dc_refine_script())
    sc, d = scan_bytes(f)[1]
    assert kind(sc) == 1 and sc["comps"] == [1] and d == (b"\x7f" + b"\xff\x00" * 33 if first_zero else b"\xff\x00" * 34), d.hex()
    assert (d[32], d[31]) == ((0x00, 0xFF) if first_zero else (0xFF, 0x00))
    return f


@functools.lru_cache(None)
def smallest(cut):
    """Component 1's DC refinement of exactly 64 bytes (two segments: cut) or, cut=False, of 63 (one lane)."""
    frame, planes = _chroma(16, 32) if cut else _chroma(18, 28)
    planes[1][:, :, 0] = 6
    planes[1][::3, ::2, 0] = 7
    f = R.transcode(frame, planes, _dc_refine_script())
    sc, d = scan_bytes(f)[1]
    assert kind(sc) == 1 and sc["comps"] == [1] and len(d) == (64 if cut else 63) and b"\xff" not in d
    return f


@functools.lru_cache(None)
def two_bands():
    """Two AC refinements of different bands (1..5 and 6..63) of component 0 on one level, both several segments long."""
    frame, planes = frame_of(CHROMA, "cmyk", 96, 96, 12)
    a = [0, 1, 2, 3]
    script = ([(a, 0, 0, 0, 0), ([0], 1, 5, 0, 1), ([0], 6, 63, 0, 1), ([0], 1, 5, 1, 0), ([0], 6, 63, 1, 0)] + [([c], 1, 63, 0, 0) for c in (1, 2, 3)])
    f = R.transcode(frame, planes, script)
    q = R.parse(f)
    assert q["levels"][3] == q["levels"][4] == 1 and q["levels"][1] == q["levels"][2] == 0, q["levels"]
    assert all(len(d) >= 2 * S for sc, d in scan_bytes(f) if kind(sc) == 3) and sum(kind(sc) == 3 for sc in q["scans"]) == 2
    return _check_good("two_bands", f, (0, 2, 3))


@functools.lru_cache(None)
def sequential():
    """A sequential file in three scans, every one long enough to be cut if it were progressive: all stay on route 0."""
    frame, planes = frame_of([(1, 1), (1, 1), (1, 1), (2, 2)], "cmyk", 64, 48, 14)
    f = R.transcode(frame, planes, [[3], [0, 1], [2]], sequential=True)
    assert all(kind(sc) == 4 and len(d) >= 2 * S for sc, d in scan_bytes(f))
    return f


def limits():
    """[(name, file)]: the boundary constructions, all with status OK."""
    out = [("straddle", straddle()), ("eob_boundary", eob_boundary()), ("ac_first_overshoot", ac_first_overshoot()),
           ("dc_refine_ones", dc_refine_ones(False)), ("dc_refine_7f_ones", dc_refine_ones(True)), ("smallest_cut", smallest(True)),
           ("one_byte_less", smallest(False))]
    return [(n, _check_good(n, f)) for n, f in out]


@functools.lru_cache(None)
def good():
    """[(name, file)]: every file decodes with Pillow."""
    out = (shared_table() + [(n, f) for n, f, _ in table_sequences()] + [("pil_440", pillow_440()), ("ten_blocks", ten_blocks())] + subsets() +
           [("padded_411", padded_plane())] + limits() + [("two_bands", two_bands()), ("sequential", sequential())])
    assert len({n for n, _ in out}) == len(out)
    return out


@functools.lru_cache(None)
def broken():
    """[(name, file)]: the ten-block file damaged INSIDE a scan that is cut: an invalid code in the DC first pass, the AC first
    pass and the AC refinement of component 0, and the file ending inside the DC first pass and inside that refinement."""
    frame, planes = frame_of([(2, 2), (1, 1), (1, 1), (2, 2)], "ycck", 128, 112, 4, ac=4)
    script = approximation(4)
    ones = [(0xFFFF, 16), (0xFFFF, 16)]                      # no code of the fixed tables is all ones
    out = [("broken_dc_code", R.transcode(frame, planes, script, hack={(0, 300): ones}), 0),
           ("broken_ac_first_code", R.transcode(frame, planes, script, hack={(1, 100): ones}), 1),
           ("broken_ac_refine_code", R.transcode(frame, planes, script, hack={(5, 100): ones}), 5),
           ("broken_dc_cut", R.transcode(frame, planes, script, cut=(0, 0.6)), 0),
           ("broken_ac_refine_cut", R.transcode(frame, planes, script, cut=(5, 0.5)), 5)]
    for name, f, i in out:
        sc, d = scan_bytes(f)[i]
        assert R.decode(f)[0] != 0 and len(d) >= 2 * S and sc["units"] == 1, name
    return [(n, f) for n, f, _ in out]


def malformed():
    """The 21 malformed files of jpegscan_cases (small: their failing scans stay on one lane) and those of broken()."""
    out = SC.malformed()
    assert len(out) == 21
    return out + broken()
