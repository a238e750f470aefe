"""Files of the two JPEG kinds only ``all_scans=True`` decodes (tests of attwarp_amd.jpeg: test_jpegscan_ref_cpu.py,
test_jpegscan_host_cpu.py, test_jpegscan_gpu.py): progressive files of the layouts the baseline records refuse, and
sequential files whose components come in several scans.  Built at run time three ways: Pillow's own progressive writer
(CMYK, keep_rgb), header edits of Pillow's progressive files (4:4:0, YCCK, RGB-coded), and the transcoder of jpegscan_ref
over the coefficient planes of jpegfmt_cases' one-scan files, one scan script per (layout, size) in rotation.  Pillow opens
every file of good(); malformed() files carry the restatement's status; refused() files are turned away by the marker walk
even with the keyword."""
from __future__ import annotations

import functools

import jpegdec_cases as C
import jpegfmt_cases as L
import jpegscan_ref as R


def _sof(fn):
    """An edit of the SOF2 payload (C.sof_edit knows the sequential frames only)."""
    return lambda segs: [(m, fn(bytearray(pl)) if m == 0xC2 else pl) for m, pl in segs]


def _resized(w, h, luma):
    return _sof(lambda b: L.resized(w, h, luma)([(0xC0, bytes(b))])[0][1])


# ---- scan scripts over nf components -----------------------------------------------------------------------------------------------
def spectral(nf):
    """Spectral selection only: one interleaved DC scan, two bands per component."""
    a = list(range(nf))
    return [(a, 0, 0, 0, 0)] + [s for c in a for s in (([c], 1, 5, 0, 0), ([c], 6, 63, 0, 0))]


def approximation(nf):
    """Successive approximation: DC with Al = 1, AC with Al = 2 and two refinements."""
    a = list(range(nf))
    return ([(a, 0, 0, 0, 1)] + [([c], 1, 63, 0, 2) for c in a] + [([c], 1, 63, 2, 1) for c in a] + [(a, 0, 0, 1, 0)]
            + [([c], 1, 63, 1, 0) for c in a])


def dc_subset(nf):
    """DC interleaved over a subset of the components, the others alone."""
    a = list(range(nf))
    dc = [(a[1:], 0, 0, 0, 0), ([0], 0, 0, 0, 0)] if nf > 2 else [([c], 0, 0, 0, 0) for c in a]
    return dc + [([c], 1, 63, 0, 0) for c in reversed(a)]


def dc_each(nf):
    """One DC scan per component, then two coefficient halves per component with a refinement of the upper one."""
    a = list(range(nf))
    return [([c], 0, 0, 0, 0) for c in a] + [s for c in a for s in (([c], 1, 9, 0, 0), ([c], 10, 63, 0, 1), ([c], 10, 63, 1, 0))]


def split_bands(nf):
    """One scan per band split at Ss = 1, 6, 63: every band of every block is a scan of its own level."""
    a = list(range(nf))
    return [(a, 0, 0, 0, 0)] + [([c], lo, hi, 0, 0) for c in a for lo, hi in ((1, 5), (6, 62), (63, 63))]


SCRIPTS = [("spectral", spectral), ("approx", approximation), ("dc_subset", dc_subset), ("dc_each", dc_each), ("split_at", split_bands)]


def sequential_splits(nf):
    """The scan splits of a sequential file of nf components."""
    a = list(range(nf))
    out = [("each", [[c] for c in a]), ("first_rest", [[0], a[1:]]), ("reversed", [[c] for c in reversed(a)])]
    if nf == 4:
        out.append(("k_first", [[3], [0, 1], [2]]))
    return out


def _restarts(frame, script, how, sequential=False):
    """Restart intervals per scan: "mcu" one MCU of the scan, "row" one MCU row, "mixed" changed and removed between scans."""
    out = []
    for i, e in enumerate(script):
        comps = list(e) if sequential else e[0]
        mcux = R.scan_mcus(frame["W"], frame["H"], frame["samp"], comps)[0]
        out.append({"mcu": 1, "row": mcux, "mixed": (0, 1, 0, mcux, 2)[i % 5]}[how])
    return out


@functools.lru_cache(maxsize=None)
def source(name, W, H, seed=0, ri=0):
    """(one-scan sequential file, frame, coefficient planes) of a layout of jpegfmt_cases.LAYOUTS, or "420" / "cmyk_q100"."""
    if name == "420":
        f = C.write(C.noise(W, H, 3, seed), quality=90, subsampling=2)
    elif name == "cmyk_q100":
        f = L.write_cmyk(C.noise(W, H, 4, seed), quality=100, subsampling=2)
    else:
        _, samp, color = next(e for e in L.LAYOUTS if e[0] == name)
        f = L.coef_file(W, H, samp, color, seed, ri)
    return (f,) + R.source_planes(f)


@functools.lru_cache(maxsize=None)
def pillow():
    """(name, file): Pillow's own progressive writer and header edits of its files."""
    out = []
    for sub in (0, 1, 2):
        for W, H in ((1, 1), (5, 3), (17, 15), (33, 20)):
            out.append((f"pil_cmyk_s{sub}_{W}x{H}", L.write_cmyk(C.noise(W, H, 4, 10 * sub + W), quality=85, subsampling=sub, progressive=True)))
        out.append((f"pil_cmyk_s{sub}_ri_row", L.write_cmyk(C.blocky(40, 31, 4, sub), quality=85, subsampling=sub, progressive=True, restart_marker_rows=1)))
        out.append((f"pil_cmyk_s{sub}_ri_1", L.write_cmyk(C.noise(24, 17, 4, 50 + sub), quality=75, subsampling=sub, progressive=True, restart_marker_blocks=1)))
    for W, H in ((1, 1), (16, 16), (23, 19)):
        out.append((f"pil_keep_rgb_{W}x{H}", C.write(C.noise(W, H, 3, W), quality=85, keep_rgb=True, progressive=True)))
    out.append(("pil_keep_rgb_ri_row", C.write(C.blocky(40, 31, 3, 3), quality=85, keep_rgb=True, progressive=True, restart_marker_rows=1)))
    out.append(("pil_keep_rgb_ri_1", C.write(C.noise(24, 17, 3, 4), quality=85, keep_rgb=True, progressive=True, restart_marker_blocks=1)))
    for W, H in ((16, 8), (32, 24), (48, 40), (15, 7)):       # progressive 4:2:2 of W x H -> 4:4:0 of H x W
        out.append((f"edit_440_{H}x{W}", C.edit(C.write(C.noise(W, H, 3, W + H), quality=80, subsampling=1, progressive=True), _resized(H, W, 0x12))))
    out.append(("edit_440_ri_row", C.edit(C.write(C.noise(48, 40, 3, 8), quality=80, subsampling=1, progressive=True, restart_marker_rows=1),
                                          _resized(40, 48, 0x12))))
    cmyk = L.write_cmyk(C.noise(33, 20, 4, 9), quality=85, subsampling=2, progressive=True)
    out.append(("edit_ycck_s2", C.edit(cmyk, lambda s: C.replace(s, 0xEE, lambda pl: pl[:11] + b"\x02"))))
    for sub in (1, 2):                                       # RGB-coded by the Adobe transform on a file stripped of its JFIF marker
        f = C.write(C.noise(33, 20, 3, 12 + sub), quality=85, subsampling=sub, progressive=True)
        out.append((f"edit_adobe_rgb_s{sub}", C.edit(f, lambda s: C.insert_before_sos(L.strip_jfif(s), [L.ADOBE(0)]))))
    return out


@functools.lru_cache(maxsize=None)
def transcoded():
    """(name, file, one-scan source file): progressive and several-scan sequential files of every layout of
    jpegfmt_cases.LAYOUTS.  Every (layout, size) takes one script, in rotation, so every layout meets every script."""
    out, turn = [], 0
    for name, samp, color in L.LAYOUTS:
        nf = len(samp)
        for j, (W, H) in enumerate(L.sizes(samp)):
            f, frame, planes = source(name, W, H, 7 * j)
            sname, make = SCRIPTS[turn % len(SCRIPTS)]
            script = make(nf)
            how = (None, "mcu", None, "row", "mixed")[(turn // len(SCRIPTS)) % 5]
            ri = _restarts(frame, script, how) if how else None
            ids = [i % 4 for i in range(len(script))] if turn % 3 == 0 else None       # table ids redefined between scans
            out.append((f"prog_{name}_{W}x{H}_{sname}" + (f"_ri_{how}" if how else "") + ("_ids" if ids else ""),
                        R.transcode(frame, planes, script, ri=ri, table_ids=ids), f))
            turn += 1
        # several-scan sequential files: every split at a small and a three-MCU-row size, restarts of one MCU, one row, none
        mw, mh = 8 * max(h for h, _ in samp), 8 * max(v for _, v in samp)
        for e, (split, script) in enumerate(sequential_splits(nf)):
            for g, (W, H) in enumerate(((3, 2), (mw + 1, mh + 1), (2 * mw + 3, 2 * mh + 5))):
                f, frame, planes = source(name, W, H, 90 + g)
                how = (None, "mcu", "row")[(e + g) % 3]
                ri = _restarts(frame, script, how, True) if how else None
                out.append((f"seq_{name}_{W}x{H}_{split}" + (f"_ri_{how}" if how else ""), R.transcode(frame, planes, script, sequential=True, ri=ri), f))
    for g, (W, H) in enumerate(((1, 1), (16, 16), (33, 20), (40, 31))):       # a plain 4:2:0 in three scans
        f, frame, planes = source("420", W, H, g)
        how = (None, "mcu", "row", None)[g]
        script = [[0], [1], [2]]
        out.append((f"seq_420_{W}x{H}" + (f"_ri_{how}" if how else ""),
                    R.transcode(frame, planes, script, sequential=True, ri=_restarts(frame, script, how, True) if how else None), f))
    # quality-100 noise: every band of every block is busy
    for g, (sname, make) in enumerate(SCRIPTS):
        f, frame, planes = source("cmyk_q100", 33, 20, 40 + g)
        out.append((f"prog_cmyk_q100_{sname}", R.transcode(frame, planes, make(4)), f))
    f, frame, planes = source("cmyk_q100", 33, 20, 46)
    out.append(("seq_cmyk_q100_k_first", R.transcode(frame, planes, [[3], [0, 1], [2]], sequential=True), f))
    # RGB-coded by the component ids R, G, B alone: the same files stripped of their Adobe marker
    f, frame, planes = source("rgb_g2x1", 35, 21, 47)
    adobe = b"\xff\xee\x00\x0eAdobe\0\x64\0\0\0\0\0"
    bare = C.edit(f, lambda s: [(m, pl) for m, pl in s if m != 0xEE])
    for name, g in (("prog_rgb_by_ids", R.transcode(frame, planes, dc_subset(3))), ("seq_rgb_by_ids", R.transcode(frame, planes, [[2], [0, 1]], sequential=True))):
        assert g.count(adobe) == 1
        out.append((name, g.replace(adobe, b""), bare))
    return out


def scan_limit(extra=0):
    """A 4:4:0 file of 64 + extra scans: component 0's coefficients one band each."""
    f, frame, planes = source("440", 9, 17, 60)
    n = 61 + extra
    bands = [(k, k) for k in range(1, n)] + [(n, 63)]
    script = [([0, 1, 2], 0, 0, 0, 0), ([1], 1, 63, 0, 0), ([2], 1, 63, 0, 0)] + [([0], lo, hi, 0, 0) for lo, hi in bands]
    assert len(script) == 64 + extra
    return R.transcode(frame, planes, script), f


@functools.lru_cache(maxsize=None)
def limits():
    """(name, file, source): both kernel limits: ten blocks per MCU in a four-component frame, and 64 scans."""
    f, frame, planes = source("ycck_y2x2", 35, 37, 70)
    out = [("limit_ten_blocks_prog", R.transcode(frame, planes, approximation(4)), f),
           ("limit_ten_blocks_seq", R.transcode(frame, planes, [[3], [0, 1], [2]], sequential=True), f)]
    g, src = scan_limit()
    return out + [("limit_64_scans", g, src)]


@functools.lru_cache(maxsize=None)
def good():
    """(name, file): every file decodes with Pillow."""
    out = pillow() + [(n, f) for n, f, _ in transcoded()] + [(n, f) for n, f, _ in limits()]
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    return out


def good_file(name):
    return dict(good())[name]


def _rst_edit(f, scan, which, mode):
    """The which-th restart marker of scan `scan` dropped ("missing") or renumbered ("index")."""
    p = R.parse(f)
    at, b, seen = p["scans"][scan]["off"], bytearray(f), 0
    while True:
        if b[at] == 0xFF and 0xD0 <= b[at + 1] <= 0xD7:
            if seen == which:
                break
            seen += 1
            at += 2
        else:
            assert not (b[at] == 0xFF and b[at + 1] != 0), "the scan has too few restart markers"
            at += 2 if b[at] == 0xFF else 1
    if mode == "missing":
        del b[at:at + 2]
    else:
        b[at + 1] = 0xD0 + ((b[at + 1] + 3) & 7)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def malformed():
    """(name, file): broken files of both kinds; the status is the restatement's."""
    ones = [(0xFFFF, 16), (0xFFFF, 16)]                      # no code of the fixed tables is all ones
    acc = R.P._codes(R.P.AC_TABLE)
    f, frame, planes = source("cmyk_k2x2", 35, 21, 80)
    prog, seq = spectral(4), [[3], [0, 1], [2]]
    out = []
    for i, what in ((0, "dc"), (2, "ac")):
        out += [(f"prog_{what}_cut_{int(fr * 100)}", R.transcode(frame, planes, prog, cut=(i, fr))) for fr in (0.0, 0.5, 0.9)]
    out += [(f"seq_cut_{int(fr * 100)}", R.transcode(frame, planes, seq, sequential=True, cut=(0, fr))) for fr in (0.0, 0.5, 0.9)]
    out.append(("prog_bad_code_dc", R.transcode(frame, planes, prog, hack={(0, 5): ones})))
    out.append(("prog_bad_code_ac", R.transcode(frame, planes, prog, hack={(3, 2): ones})))
    out.append(("seq_bad_code", R.transcode(frame, planes, seq, sequential=True, hack={(1, 7): ones})))
    ri = _restarts(frame, prog, "mcu")
    with_ri = R.transcode(frame, planes, prog, ri=ri)
    out.append(("prog_rst_missing_in_scan_1", _rst_edit(with_ri, 1, 1, "missing")))
    out.append(("prog_rst_wrong_index_in_scan_1", _rst_edit(with_ri, 1, 0, "index")))
    seq_ri = R.transcode(frame, planes, seq, sequential=True, ri=_restarts(frame, seq, "mcu", True))
    out.append(("seq_rst_missing_in_scan_1", _rst_edit(seq_ri, 1, 2, "missing")))
    out.append(("seq_rst_wrong_index_in_scan_1", _rst_edit(seq_ri, 1, 1, "index")))
    l61, c61 = acc[0x61]
    out.append(("prog_run_past_se", R.transcode(frame, planes, prog, hack={(1, 0): [(c61, l61), (1, 1)]})))     # scan 1: band 1..5, a run of 6
    l02, c02 = acc[0x02]
    out.append(("prog_refinement_of_size_2", R.transcode(frame, planes, approximation(4), hack={(5, 1): [(c02, l02), (3, 2)]})))   # scan 5: Ah = 2
    out.append(("prog_no_eoi", R.transcode(frame, planes, prog, eoi=False)))
    out.append(("seq_no_eoi", R.transcode(frame, planes, seq, sequential=True, eoi=False)))
    out.append(("seq_ends_inside_scan_1_of_3", R.transcode(frame, planes, seq, sequential=True, cut=(1, 0.5))))
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def refused():
    """(name, file, a word of the ValueError's message): refused even with ``all_scans=True``."""
    f, frame, planes = source("440", 9, 17, 60)
    R4 = {n: g for n, g, _, _ in C.refused()}
    eleven = C.edit(C.write(C.noise(16, 16, 3, 20), quality=75, subsampling=0, progressive=True), _sof(lambda b: C._set(b, 7, 0x33)))
    lacks = bytearray(R.transcode(frame, planes, [[0], [1], [2]], sequential=True))
    at = lacks.index(b"\xff\xda")
    lacks[at + 5] = 0x7A
    return [
        ("eleven_blocks", eleven, "blocks per MCU"),
        ("sent_twice", R.transcode(frame, planes, [[0], [0], [1], [2]], sequential=True), "already sent"),
        ("never_sent", R.transcode(frame, planes, [[0], [1]], sequential=True), "incomplete"),
        ("65_scans", scan_limit(1)[0], "more than 64 scans"),
        ("ac_scan_of_two_components", R.transcode(frame, planes, [([0, 1, 2], 0, 0, 0, 0), ([0, 1], 1, 63, 0, 0), ([2], 1, 63, 0, 0)]), "bad progression"),
        ("component_the_frame_lacks", bytes(lacks), "component the frame does not have"),
        ("dqt_16_bit", R4["dqt_16_bit"], "16-bit"),
        ("precision_12", R4["precision_12"], "precision 12"),
        ("arithmetic", R4["arithmetic"], "arithmetic"),
        ("lossless", R4["lossless"], "lossless"),
        ("hierarchical", R4["hierarchical"], "hierarchical"),
    ]
