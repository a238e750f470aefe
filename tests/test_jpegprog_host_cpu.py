"""The progressive JPEG decoder's shared host / device core (attwarp_amd/csrc/jpegprog_blocks.hpp) on the CPU under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/jpegprog_host_main.cpp is compiled as a stand-alone program and run
as a child process over the whole corpus, hostile and malformed files included.  It must end clean and print, per file,
the restatement's status, the CRC-32 of the coefficients and the planned units."""
import os
import shutil
import struct
import subprocess

import pytest

import jpegprog_cases as C
import jpegprog_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "attwarp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def corpus(files):
    out = [struct.pack("<I", len(files))]
    for f in files:
        p = R.parse(f)
        data = p["data"][p["first"]:]
        out.append(struct.pack("<IIIIIII", p["W"], p["H"], p["ncomp"], p["hs"], p["vs"], len(p["scans"]), len(data)) + data)
        for s in p["scans"]:
            comps = (s["comps"] + [0, 0])[:3]
            out.append(struct.pack("<11I", len(s["comps"]), *comps, s["ss"], s["se"], s["ah"], s["al"], s["ri"], s["off"] - p["first"],
                                   len(s["tables"])))
            for counts, syms in s["tables"]:
                out.append(bytes(counts) + bytes(syms).ljust(256, b"\0"))
    return b"".join(out)


def test_host_core_under_sanitizers_equals_the_restatement(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "jpegprog_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "jpegprog_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    named = C.good() + C.malformed() + [("eob_run", C.eob_run_case()[0])]
    (tmp_path / "corpus.bin").write_bytes(corpus([f for _, f in named]))
    r = subprocess.run([str(exe), str(tmp_path / "corpus.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(named)
    for (name, f), line in zip(named, lines):
        st, _, info = R.decode(f)
        assert tuple(int(x) for x in line.split()) == (st, info["crc"], info["units"]), name
