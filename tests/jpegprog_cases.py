"""The corpus of the progressive JPEG tests (test_jpegprog_ref_cpu.py, test_jpegprog_host_cpu.py, test_jpegprog_gpu.py): Pillow's
own progressive files at the sizes where a scan's covered blocks differ from the padded plane, scripts only the
transcoder of jpegprog_ref.py can write, hostile and malformed files, and what the marker walk refuses.  Every picture is
as small as its case allows; the one large case is the EOB run of 32767."""
from __future__ import annotations

import functools
import io

import numpy as np
from PIL import Image

import jpegprog_ref as R

SUB = {"444": 0, "422": 1, "420": 2}


def noise(h, w, c, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, c) if c == 3 else (h, w), dtype=np.uint8)


def save(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", **kw)
    return b.getvalue()


_SIZES = [("1x1_420", 1, 1, 3, "420"), ("8x8_444", 8, 8, 3, "444"), ("9x9_420", 9, 9, 3, "420"), ("17x9_422", 9, 17, 3, "422"),
          ("17x33_420", 33, 17, 3, "420"), ("33x20_420", 20, 33, 3, "420"), ("16x16_444", 16, 16, 3, "444"),
          ("grey_40x52", 52, 40, 1, None), ("grey_17x9", 9, 17, 1, None)]


@functools.lru_cache(None)
def pillow():
    """[(name, file)]: Pillow's own scripts (10 scans YCbCr, 6 grey), noise so that the refinements carry correction bits."""
    out = []
    for i, (name, h, w, c, sub) in enumerate(_SIZES):
        a = noise(h, w, c, 100 + i)
        kw = {} if sub is None else {"subsampling": SUB[sub]}
        for q in (75, 100):
            out.append((f"{name}_q{q}", save(a, quality=q, progressive=True, **kw)))
        out.append((f"{name}_opt", save(a, quality=75, progressive=True, optimize=True, **kw)))
        if max(h, w) > 8:
            out.append((f"{name}_rows", save(a, quality=90, progressive=True, restart_marker_rows=1, **kw)))
            out.append((f"{name}_rst3", save(a, quality=90, progressive=True, restart_marker_blocks=3, **kw)))
    return out


def _grey_script(al):
    s = [([0], 0, 0, 0, al), ([0], 1, 63, 0, al)]
    for a in range(al, 0, -1):
        s += [([0], 0, 0, a, a - 1), ([0], 1, 63, a, a - 1)]
    return s


def _colour_source():
    return save(noise(20, 33, 3, 7), quality=92, subsampling=2)


@functools.lru_cache(None)
def transcoded():
    """[(name, file, its baseline source)]: scripts Pillow does not write."""
    out = []
    src = _colour_source()
    p, planes = R.baseline_planes(src)
    spectral = [([0, 1, 2], 0, 0, 0, 0), ([0], 1, 5, 0, 0), ([0], 6, 63, 0, 0), ([1], 1, 63, 0, 0), ([2], 1, 63, 0, 0)]
    out.append(("spectral_only", R.transcode(p, planes, spectral), src))
    three = [([0, 1, 2], 0, 0, 0, 3)] + [([c], 1, 63, 0, 3) for c in range(3)]
    for a in (3, 2, 1):
        three += [([0, 1, 2], 0, 0, a, a - 1)] + [([c], 1, 63, a, a - 1) for c in range(3)]
    out.append(("three_refinements", R.transcode(p, planes, three), src))
    sep = [([c], 0, 0, 0, 1) for c in range(3)] + [([c], 1, 63, 0, 0) for c in range(3)] + [([c], 0, 0, 1, 0) for c in range(3)]
    out.append(("dc_separate", R.transcode(p, planes, sep), src))
    out.append(("dc_pairs", R.transcode(p, planes, [([0], 0, 0, 0, 0), ([1, 2], 0, 0, 0, 0)] + spectral[1:]), src))
    out.append(("dri_changes", R.transcode(p, planes, spectral, ri=[2, 0, 3, 1, 0]), src))
    out.append(("dri_refine", R.transcode(p, planes, three, ri=[(i % 3) + 1 for i in range(len(three))]), src))
    out.append(("table_ids", R.transcode(p, planes, three, table_ids=[i % 4 for i in range(len(three))]), src))
    g8 = save(noise(8, 8, 1, 9), quality=100)
    pg, plg = R.baseline_planes(g8)
    out.append(("one_scan_per_coefficient", R.transcode(pg, plg, [([0], k, k, 0, 0) for k in range(64)]), g8))
    for ss in range(1, 64):
        script = [([0], 0, 0, 0, 1), ([0], 1, 63, 0, 1) if ss == 1 else ([0], 1, ss - 1, 0, 1)]
        if ss > 1:
            script += [([0], ss, 63, 0, 1), ([0], 1, ss - 1, 1, 0)]
            script += [([0], ss, 63, 1, 0), ([0], 0, 0, 1, 0)]
        else:
            script += [([0], 1, 63, 1, 0), ([0], 0, 0, 1, 0)]
        out.append((f"split_at_{ss}", R.transcode(pg, plg, script), g8))
    g = save(noise(23, 19, 1, 11), quality=95)
    pg2, plg2 = R.baseline_planes(g)
    out.append(("grey_three_refinements", R.transcode(pg2, plg2, _grey_script(3), ri=[0, 2, 0, 4, 1, 0, 0, 5]), g))
    return out


def scan_limit(extra=0):
    """A grey 8x8 file of exactly MAX_SCANS (+ extra) scans: coefficient by coefficient, the tail refined bit by bit."""
    g8 = save(noise(8, 8, 1, 9), quality=100)
    pg, plg = R.baseline_planes(g8)
    n = R.MAX_SCANS + extra
    script = [([0], 0, 0, 0, 0)] + [([0], k, k, 0, 0) for k in range(1, 63)]          # 63 scans, coefficient 63 left
    left = n - len(script)                                                              # >= 1 scans for coefficient 63
    script += [([0], 63, 63, 0, left - 1)] + [([0], 63, 63, a, a - 1) for a in range(left - 1, 0, -1)]
    assert len(script) == n
    return R.transcode(pg, plg, script), g8


@functools.lru_cache(None)
def eob_run_case(h=1448, w=1456):
    """A flat grey picture of 32942 blocks with one coefficient in the LAST block: an EOB run of exactly 32767 and then the
    rest, in a first pass and (the coefficient being 3: one refinement with history only in the last block) in a
    refinement pass."""
    bh, bw = h // 8, w // 8
    planes = [np.zeros((bh, bw, 64), np.int16)]
    planes[0][:, :, 0] = 8
    planes[0][-1, -1, 1] = 3
    planes[0][0, 0, 1] = 2
    p = dict(W=w, H=h, ncomp=1, hs=1, vs=1, ri=0, qt=[[1] * 64])
    return R.transcode(p, planes, _grey_script(1)), p, planes


@functools.lru_cache(None)
def hostile():
    """DC Al = 13 with a predictor that wraps 16 bits once shifted (hand-written differences of +9 and +32767 in the first
    two blocks): the pixels are the restatement's alone."""
    planes = [np.zeros((2, 3, 64), np.int16)]
    planes[0][:, :, 0] = np.array([[8191, -8192, 4097], [-1, 1, 8190]], np.int16) << 2    # the first pass sends DC >> 13, thirteen refinements the rest
    planes[0][0, 1, 5] = -3
    p = dict(W=24, H=16, ncomp=1, hs=1, vs=1, ri=0, qt=[[255] * 64])
    script = [([0], 0, 0, 0, 13)] + [([0], 0, 0, a, a - 1) for a in range(13, 0, -1)] + [([0], 1, 63, 0, 0)]
    return [("dc_al13", R.transcode(p, planes, script, hack={(0, 0): [(4, 4), (9, 4)], (0, 1): [(0b11110, 5), (0x7FFF, 15)]}))]


def good():
    """[(name, file)]: every file that decodes with status OK."""
    return pillow() + [(n, f) for n, f, _ in transcoded()] + [("scan_limit", scan_limit()[0])] + hostile()


@functools.lru_cache(None)
def malformed():
    """[(name, file)]: files the marker walk accepts and the decoder gives a status other than OK."""
    out = []
    base = dict(pillow())["17x33_420_q100"]
    p = R.parse(base)
    for i, kind in ((0, "dc_first"), (1, "ac_first"), (5, "ac_refine"), (6, "dc_refine")):
        sc = p["scans"][i]
        end = next(x for x in R.markers(base) if x >= sc["off"])
        out.append((f"cut_in_{kind}", base[:max(sc["off"], end - 2 if kind != "dc_refine" else sc["off"])]))
    out.append(("no_eoi", base[:-2]))
    rows = dict(pillow())["17x33_420_rows"]
    pr = R.parse(rows)
    sc = pr["scans"][2]
    rst = [i for i in range(sc["off"], len(rows) - 1) if rows[i] == 0xFF and 0xD0 <= rows[i + 1] <= 0xD7]
    at = rst[0]
    out.append(("rst_removed", rows[:at] + rows[at + 2:]))
    out.append(("rst_doubled", rows[:at] + rows[at:at + 2] + rows[at:]))
    out.append(("rst_renumbered", rows[:at + 1] + bytes([0xD0 + ((rows[at + 1] + 1) & 7)]) + rows[at + 2:]))
    # hand-written symbols through the transcoder's fixed tables (AC code of symbol s: 8 bits of value s)
    g = save(noise(16, 16, 1, 13), quality=95)
    pg, plg = R.baseline_planes(g)
    script = [([0], 0, 0, 0, 1), ([0], 1, 20, 0, 1), ([0], 21, 63, 0, 1), ([0], 1, 63, 1, 0), ([0], 0, 0, 1, 0)]
    T = lambda hack: R.transcode(pg, plg, script, hack=hack)
    out.append(("no_code_dc", T({(0, 1): [(0xFFFF, 16)]})))
    out.append(("no_code_ac", T({(1, 2): [(0xFFFF, 16)]})))
    out.append(("run_past_se", T({(1, 0): [(0xF1, 8), (1, 1), (0x61, 8), (1, 1)]})))          # 15 zeros + 1, then 6 zeros: k = 22 > 20
    out.append(("zrl_past_se", T({(1, 3): [(0xF0, 8), (0xF0, 8)]})))                             # k = 1 + 16 + 16 > 21
    out.append(("refine_s2", T({(3, 1): [(0x02, 8), (3, 2)]})))
    out.append(("two_scans_fail", T({(2, 0): [(0xFFFF, 16)], (1, 3): [(0xF0, 8), (0xF0, 8)]})))  # the earlier scan decides: E_COEFF
    return out


def refused():
    """[(name, file, word of the ValueError)]."""
    g8 = save(noise(8, 8, 1, 9), quality=100)
    pg, plg = R.baseline_planes(g8)
    T = lambda script: R.transcode(pg, plg, script, encode=False)
    full = [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0)]
    out = [("ss_above_se", T([([0], 0, 0, 0, 0), ([0], 5, 4, 0, 0)]), "progression"),
           ("se_above_63", T([([0], 0, 0, 0, 0), ([0], 1, 64, 0, 0)]), "progression"),
           ("dc_with_ac", T([([0], 0, 5, 0, 0)]), "progression"),
           ("al_14", T([([0], 0, 0, 0, 14)]), "progression"),
           ("ah_al_gap", T([([0], 0, 0, 0, 3), ([0], 0, 0, 3, 1)]), "progression"),
           ("refine_wrong_precision", T([([0], 0, 0, 0, 2), ([0], 0, 0, 1, 0)]), "refinement"),
           ("refine_unsent", T([([0], 0, 0, 0, 0), ([0], 1, 63, 1, 0)]), "refinement"),
           ("first_pass_twice", T(full + [([0], 3, 9, 0, 0)]), "already sent"),
           ("ac_before_dc", T([([0], 1, 63, 0, 0), ([0], 0, 0, 0, 0)]), "DC"),
           ("incomplete_band", T([([0], 0, 0, 0, 0), ([0], 1, 62, 0, 0)]), "incomplete"),
           ("incomplete_precision", T([([0], 0, 0, 0, 1), ([0], 1, 63, 0, 0)]), "incomplete"),
           ("too_many_scans", scan_limit(1)[0], "scans")]
    src = _colour_source()
    p, planes = R.baseline_planes(src)
    out.append(("ac_interleaved", R.transcode(p, planes, [([0, 1, 2], 0, 0, 0, 0), ([0, 1], 1, 63, 0, 0)], encode=False), "progression"))
    return out
