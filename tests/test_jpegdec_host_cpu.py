"""The JPEG decoder's shared host / device core (attwarp_amd/csrc/jpegdec_blocks.hpp) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/jpegdec_host_main.cpp is compiled as a stand-alone program and run as a child process
over the whole corpus, the malformed files and the longest hand-written blocks (tests/jpegdec_limit_cases.py) included.  It must end clean and print, per file, the restatement's status,
the CRC-32 of the coefficients and the planned units."""
import os
import shutil
import struct
import subprocess

import pytest

import jpegdec_cases as C
import jpegdec_limit_cases as L
import jpegdec_ref as D

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def corpus(files):
    out = [struct.pack("<I", len(files))]
    for f in files:
        p = D.parse(f)
        out.append(struct.pack("<IIIIII", p["W"], p["H"], p["ncomp"], p["hs"], p["vs"], p["ri"]))
        for c in range(p["ncomp"]):
            for counts, syms in (p["dc"][c], p["ac"][c]):
                out.append(bytes(counts) + bytes(syms).ljust(256, b"\0"))
        out.append(struct.pack("<I", len(p["stream"])) + p["stream"])
    return b"".join(out)


def test_host_core_under_sanitizers_equals_the_restatement(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "jpegdec_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "jpegdec_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    limits = L.long_files() + L.long_cuts()                  # blocks as long as a block can be, whole and cut short
    names = [n for n, _ in C.good()] + [n for n, _, _ in C.malformed()] + [n for n, _ in limits]
    files = [f for _, f in C.good()] + [f for _, f, _ in C.malformed()] + [f for _, f in limits]
    (tmp_path / "corpus.bin").write_bytes(corpus(files))
    r = subprocess.run([str(exe), str(tmp_path / "corpus.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(files) + 1 and lines[-1].startswith("arith ")
    for name, f, line in zip(names, files, lines):
        st, _, info = D.decode(f)
        assert tuple(int(x) for x in line.split()) == (st, info["crc"], info["nunits"]), name
