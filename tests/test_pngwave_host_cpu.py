"""The wave route's shared host / device core (attwarp_amd/csrc/pngdec_wave_blocks.hpp) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/pngwave_host_main.cpp -- the same text with a host loop in place of the wave -- is compiled
as a stand-alone program and run as a child process over both limit corpora, the new cases (tests/pngwave_cases.py) and
the malformed files, at 16 and at 128 bytes per segment.  It must end clean and print the restatement's answers
(tests/pngwave_ref.py): windows, rounds, accepted, resolution rounds and the Adler-32 of the bytes of an accepted file."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import pngdec_cases as C
import pngdec_limit_cases as L
import pngdec_ref as D
import pngwave_cases as WC
import pngwave_ref as W

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def corpus(files):
    out = [struct.pack("<I", len(files))]
    for f in files:
        p = D.parse(f)
        rb = 1 + p["W"] * D.CHANNELS[p["color_type"]]
        out.append(struct.pack("<III", p["H"] * rb, rb, len(p["chunks"])))
        out += [struct.pack("<II", len(c), crc) for c, crc in p["chunks"]]
        out.append(p["stream"])
    return b"".join(out)


def test_host_core_under_sanitizers_equals_the_restatement(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "pngwave_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "pngwave_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    files = ([(n, f) for n, f, _ in L.limit_good()] + list(C.good()) + WC.good() + [(n, f) for n, f, _ in L.limit_malformed()] +
             [(n, f) for n, f, _ in C.malformed()] + [(n, f) for n, f, _ in WC.malformed()])
    path = tmp_path / "corpus.bin"
    path.write_bytes(corpus([f for _, f in files]))
    for seg, mr in ((16, 64), (128, 64), (16, 63)):
        r = subprocess.run([str(exe), str(path), str(seg), str(mr)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(files)
        accepted = 0
        for (name, f), line in zip(files, lines):
            p = D.parse(f)
            out, info, res_rounds = W.decode_stream(p["stream"], p["H"] * (1 + p["W"] * D.CHANNELS[p["color_type"]]), seg, mr)
            want = info + (res_rounds, zlib.adler32(out) if out is not None else 0)
            assert tuple(int(x) for x in line.split()) == want, (name, seg, mr)
            accepted += info[2]
        assert accepted > 300
