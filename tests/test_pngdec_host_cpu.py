"""The PNG decoder's shared host / device core (attwarp_amd/csrc/pngdec_blocks.hpp) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/pngdec_host_main.cpp is compiled as a stand-alone program and run as a child process
over the whole corpus and over the limit files (tests/pngdec_limit_cases.py), the malformed files included.  It must end clean and print, per file, the restatement's status,
Adler-32 of the bytes produced, route and chain."""
import os
import shutil
import struct
import subprocess

import pytest

import zlib

import pngdec_cases as C
import pngdec_limit_cases as L
import pngdec_ref as D

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
    exe = tmp_path / "pngdec_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "pngdec_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    route_id = {"unit": 0, "serial": 1, None: 2}

    def expected(f):
        st, _, info = D.decode(f)
        return (st, info["adler"], route_id[info["route"]], info["chain"], info["nunits"])

    # the corpus of pngdec_cases, then the limit files (pngdec_limit_cases), good and malformed; of the two row-limit files
    # the builder states what the restatement would take minutes to find
    first = [(n, f, None) for n, f in C.good()] + [(n, f, None) for n, f, _ in C.malformed()]
    second = [(n, f, None) for n, f, _ in L.limit_good()] + [(n, f, None) for n, f, _ in L.limit_malformed()]
    second += [(k.name, k.file, (0, zlib.adler32(k.filtered), 0, k.expect["chain"], k.expect["nkept"])) for k in L.limit_rowmax()]
    for tag, files in (("corpus", first), ("limits", second)):
        path = tmp_path / f"{tag}.bin"
        path.write_bytes(corpus([f for _, f, _ in files]))
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(files)
        for (name, f, want), line in zip(files, lines):
            assert tuple(int(x) for x in line.split()) == (want or expected(f)), name
