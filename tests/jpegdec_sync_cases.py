"""Marker-less files for the tests of the JPEG decoder's sub-streams (test_jpegdec_sync_ref_cpu.py,
test_jpegdec_sync_host_cpu.py, test_jpegdec_sync_gpu.py), made with Pillow through jpegdec_cases.write: files that fall in
step quickly and slowly, one with more 32-byte segments than a workgroup has lanes, one with FF 00 pairs across segment
boundaries, one shorter than two segments."""
from __future__ import annotations

import functools

import jpegdec_cases as C
import jpegdec_ref as D

SEGMENT_BYTES = (32, 64, 128, 256, 512)
MAX_ROUNDS = 256                                           # the slowest file here needs 233 rounds at 32 bytes
STRADDLE = "smooth_512x384_q90_s2"                          # FF | 00 across a boundary at 32, 64 and 128 bytes
LARGE = "smooth_400x300_q95_s0"                             # >= 33 KB, quick to synchronise: the stride loop at 32 bytes
SLOW = "noise_64x48_q100_s0"                                # needs 116 rounds at 32 bytes
SHORT = "grey_8x8_short"                                    # data shorter than two segments of any size


@functools.lru_cache(maxsize=None)
def good():
    out = [
        ("smooth_256x192_q75_s2", C.write(C.smooth_detail(256, 192), quality=75, subsampling=2)),
        (STRADDLE, C.write(C.smooth_detail(512, 384, 2), quality=90, subsampling=2)),
        (LARGE, C.write(C.smooth_detail(400, 300), quality=95, subsampling=0)),
        ("smooth_200x136_q90_s0", C.write(C.smooth_detail(200, 136), quality=90, subsampling=0)),
        ("noise_128x96_q50_s1", C.write(C.noise(128, 96), quality=50, subsampling=1)),
        ("blocky_128x128_q75_optimize", C.write(C.blocky(128, 128), quality=75, optimize=True)),
        ("grey_160x120_q75", C.write(C.noise(160, 120, 1), quality=75)),
        ("noise_96x96_q100_s0", C.write(C.noise(96, 96), quality=100, subsampling=0)),
        (SLOW, C.write(C.noise(64, 48), quality=100, subsampling=0)),
        (SHORT, C.write(C.smooth_detail(8, 8)[:, :, 0].copy(), quality=30)),
    ]
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    return out


def good_file(name):
    return dict(good())[name]


def one_unit(files):
    """The (name, file) pairs whose plan has exactly one unit."""
    return [(n, f) for n, f in files if D.geometry(D.parse(f))["nunits"] == 1]


@functools.lru_cache(maxsize=None)
def all_one_unit_good():
    return one_unit(list(C.good()) + list(good()))
