"""Limit files of the progressive scans' sub-streams (test_jpegprog_sync_host_cpu.py, test_jpegprog_sync_gpu.py; DESIGN.md
3.23), on top of the corpus of jpegprog_cases.py.  Every builder asserts, from the file's own bytes, the property its name
claims, so a case that stops hitting its limit fails here, on the CPU."""
from __future__ import annotations

import functools

import numpy as np

import jpegprog_cases as C
import jpegprog_ref as R

S = 32                                                    # the segment size every case is built for


def scan_bytes(f):
    """[(scan of the parse, its entropy data up to the first marker)] of a progressive file."""
    p = R.parse(f)
    out = []
    for sc in p["scans"]:
        end = next((x for x in R.markers(p["data"]) if x >= sc["off"]), len(p["data"]))
        out.append((sc, bytes(p["data"][sc["off"]:end])))
    return out


def kind(sc):
    return (2 if sc["ss"] else 0) + (1 if sc["ah"] else 0)    # JP_DC_FIRST, JP_DC_REFINE, JP_AC_FIRST, JP_AC_REFINE


def _grey(bh, bw, qt=1):
    return dict(W=8 * bw, H=8 * bh, ncomp=1, hs=1, vs=1, ri=0, qt=[[qt] * 64]), [np.zeros((bh, bw, 64), np.int16)]


@functools.lru_cache(None)
def straddle():
    """Noise of +-1 and a few +-3 in every AC coefficient: the refinement places some 58 new coefficients per block at 9 bits
    each and corrects the rest, more than 65 bytes per block on average, so a block touches three 32-byte segments or more."""
    p, planes = _grey(4, 4)
    rng = np.random.default_rng(21)
    planes[0][:, :, 1:] = rng.choice(np.array([-1, 1], np.int16), (4, 4, 63))
    planes[0][:, :, 7::13] *= 3
    planes[0][:, :, 0] = 10
    f = R.transcode(p, planes, C._grey_script(1))
    sc, d = [x for x in scan_bytes(f) if kind(x[0]) == 3][-1]
    assert len(d) / 16 > 65, len(d)
    return f


@functools.lru_cache(None)
def eob_boundary():
    """An AC refinement that opens with an EOB run of 8 blocks: 8 + 3 bits of symbol, 245 correction bits of blocks 0..3,
    none of blocks 4..7 (no history), so the run ends at bit 256, the first byte of segment 1: the zero-bit blocks lie on
    the boundary."""
    p, planes = _grey(4, 4)
    a = planes[0].reshape(16, 64)
    a[:, 0] = 16
    for b, n in enumerate((61, 61, 61, 62)):
        a[b, [R.ZIGZAG[k] for k in range(1, 1 + n)]] = 2     # history, correction bit 0
    for b in range(8, 16):
        a[b, [R.ZIGZAG[k] for k in range(1, 31)]] = 1        # thirty new coefficients each: the scan runs on
    f = R.transcode(p, planes, C._grey_script(1))
    sc, d = [x for x in scan_bytes(f) if kind(x[0]) == 3][0]
    assert d[:32] == bytes([0x30]) + bytes(31) and len(d) >= 2 * S, d[:34].hex()
    return f


@functools.lru_cache(None)
def eob_run_textured(h=1448, w=1456):
    """jpegprog_cases.eob_run_case with a textured corner: the refinement holds an EOB run of 32767 AND two segments or more."""
    bh, bw = h // 8, w // 8
    p, planes = _grey(bh, bw)
    planes[0][:, :, 0] = 8
    for b in range(12):
        planes[0][0, b, [R.ZIGZAG[k] for k in range(1, 64)]] = 2 + (b & 1)     # 63 correction bits each
        planes[0][0, b, R.ZIGZAG[5]] = 1
    planes[0][-1, -1, 1] = 3
    f = R.transcode(p, planes, C._grey_script(1))
    R.reset_counters()
    st, _, _ = R.decode(f)
    sc, d = [x for x in scan_bytes(f) if kind(x[0]) == 3][0]
    assert st == 0 and R.COUNT["max_eobrun"] >= 32767 and len(d) >= 2 * S, (st, R.COUNT["max_eobrun"], len(d))
    return f


@functools.lru_cache(None)
def ac_first_overshoot():
    """The last block of an AC first pass is an EOB run of 15 blocks: it overshoots the last block by 14."""
    p, planes = _grey(6, 6, qt=3)
    rng = np.random.default_rng(5)
    planes[0][:, :, :] = rng.integers(-6, 7, planes[0].shape)
    planes[0][-1, -1, 1:] = 0
    script = [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0)]
    f = R.transcode(p, planes, script, hack={(1, 35): [(0x30, 8), (7, 3)]})
    assert R.decode(f)[0] == 0
    g = R.transcode(p, planes, script)
    assert R.decode(g)[2]["crc"] == R.decode(f)[2]["crc"] and f != g
    assert len([x for x in scan_bytes(f) if kind(x[0]) == 2][0][1]) >= 2 * S
    return f


@functools.lru_cache(None)
def dc_refine_ones(first_zero):
    """A DC refinement of all-one bits: every data byte an FF 00 pair; 68 raw bytes, the boundary at 32 on the FF of a pair.
    first_zero: block 0's bit is zero, so the first byte is 7F and the boundary lies on the 00 of a pair."""
    p, planes = _grey(17, 16)
    planes[0][:, :, 0] = 5
    if first_zero:
        planes[0][0, 0, 0] = 4
    f = R.transcode(p, planes, [([0], 0, 0, 0, 1), ([0], 0, 0, 1, 0), ([0], 1, 63, 0, 0)])
    sc, d = [x for x in scan_bytes(f) if kind(x[0]) == 1][0]
    assert d == (b"\x7f" + b"\xff\x00" * 33 if first_zero else b"\xff\x00" * 34), d.hex()
    assert (d[32], d[31]) == ((0x00, 0xFF) if first_zero else (0xFF, 0x00))
    return f


@functools.lru_cache(None)
def smallest(cut):
    """A DC refinement of exactly 64 bytes (two segments: cut) or, cut=False, of 63 (one lane)."""
    p, planes = _grey(16, 32) if cut else _grey(18, 28)
    planes[0][:, :, 0] = 6
    planes[0][::3, ::2, 0] = 7
    f = R.transcode(p, planes, [([0], 0, 0, 0, 1), ([0], 0, 0, 1, 0), ([0], 1, 63, 0, 0)])
    sc, d = [x for x in scan_bytes(f) if kind(x[0]) == 1][0]
    assert len(d) == (64 if cut else 63) and b"\xff" not in d
    return f


def _pad_scan(f, which, to):
    """The file with scan `which`'s entropy data padded with zero bytes to `to` bytes (bytes behind the last block are
    tolerated)."""
    p = R.parse(f)
    sc = p["scans"][which]
    end = next(x for x in R.markers(p["data"]) if x >= sc["off"])
    at = len(f) - len(p["data"]) + end
    assert f[at] == 0xFF and f[at - 1] != 0xFF
    return f[:at] + bytes(to - (end - sc["off"])) + f[at:]


@functools.lru_cache(None)
def most_segments(extra):
    """The DC refinement of smallest(True) padded to exactly 16384 segments (+ extra bytes: one more, stays on one lane)."""
    f = _pad_scan(smallest(True), 1, 16384 * S + extra)
    assert len(scan_bytes(f)[1][1]) == 16384 * S + extra
    return f


@functools.lru_cache(None)
def two_bands():
    """Two AC refinements of one component on one level with different bands (1..5 and 6..63), both several segments long."""
    src = C.save(C.noise(96, 96, 1, 31), quality=100)
    p, planes = R.baseline_planes(src)
    script = [([0], 0, 0, 0, 1), ([0], 1, 5, 0, 1), ([0], 6, 63, 0, 1), ([0], 1, 5, 1, 0), ([0], 6, 63, 1, 0), ([0], 0, 0, 1, 0)]
    f = R.transcode(p, planes, script)
    q = R.parse(f)
    assert q["levels"][3] == q["levels"][4] == 1
    assert all(len(d) >= 2 * S for sc, d in scan_bytes(f) if kind(sc) == 3)
    return f


@functools.lru_cache(None)
def dc_scripts():
    """[(name, file)]: DC first passes per component and in pairs, refined the same way, every DC scan several segments long."""
    src = C.save(C.noise(120, 160, 3, 33), quality=92, subsampling=2)
    p, planes = R.baseline_planes(src)
    ac = [([c], 1, 63, 0, 0) for c in range(3)]
    sep = [([c], 0, 0, 0, 1) for c in range(3)] + ac + [([c], 0, 0, 1, 0) for c in range(3)]
    pairs = [([0], 0, 0, 0, 1), ([1, 2], 0, 0, 0, 1)] + ac + [([0, 1], 0, 0, 1, 0), ([2], 0, 0, 1, 0)]
    out = [("dc_separate_large", R.transcode(p, planes, sep)), ("dc_pairs_large", R.transcode(p, planes, pairs))]
    for _, f in out:
        assert sum(len(d) >= 2 * S for sc, d in scan_bytes(f) if kind(sc) == 0) >= 2
    return out


def limits():
    """[(name, file)]: the small limit files, all with status OK."""
    return [("straddle", straddle()), ("eob_boundary", eob_boundary()), ("ac_first_overshoot", ac_first_overshoot()),
            ("dc_refine_ones", dc_refine_ones(False)), ("dc_refine_7f_ones", dc_refine_ones(True)), ("smallest_cut", smallest(True)),
            ("one_byte_less", smallest(False)), ("two_bands", two_bands())] + dc_scripts()


@functools.lru_cache(None)
def larger():
    """[(name, file)]: Pillow's own scripts at a size where every scan is several 32-byte segments long."""
    out = []
    for name, h, w, c, sub in (("96x80_420", 80, 96, 3, "420"), ("72x88_444", 88, 72, 3, "444"), ("grey_100x60", 60, 100, 1, None)):
        a = C.noise(h, w, c, 40 + len(out))
        a[: h // 2] //= 8                                    # a quiet half: EOB runs
        kw = {} if sub is None else {"subsampling": C.SUB[sub]}
        for q in (60, 95):
            out.append((f"{name}_q{q}", C.save(a, quality=q, progressive=True, **kw)))
    return out
