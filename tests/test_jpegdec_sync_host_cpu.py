"""The sub-stream core of the JPEG decoder (attwarp_amd/csrc/jpegdec_blocks.hpp) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/jpegdec_sync_host_main.cpp is compiled as a stand-alone program, with a host loop standing
in for the workgroup, and run as a child process over both corpora and the malformed files at two segment sizes.  It must
end clean and print, per file, the restatement's accepted flag, rounds and coefficient CRC."""
import os
import shutil
import subprocess

import pytest

import jpegdec_cases as C
import jpegdec_limit_cases as L
import jpegdec_ref as D
import jpegdec_sync_cases as SC
import jpegdec_sync_ref as R
from test_jpegdec_host_cpu import CSRC, HERE, HIPCC, corpus

MAX_ROUNDS = 256


def test_sub_stream_core_under_sanitizers_equals_the_restatement(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the host program cannot be compiled")
    exe = tmp_path / "jpegdec_sync_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(HERE, "jpegdec_sync_host_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=600)
    named = list(C.good()) + list(SC.good()) + [(n, f) for n, f, _ in C.malformed()]
    named += [(n, f) for n, f in L.long_files() + L.long_cuts() if D.parse(f)["ri"] == 0]      # many segments inside one block
    (tmp_path / "corpus.bin").write_bytes(corpus([f for _, f in named]))
    seen = set()
    for S in (32, 128):
        r = subprocess.run([str(exe), str(tmp_path / "corpus.bin"), str(S), str(MAX_ROUNDS)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(named)
        for (name, f), line in zip(named, lines):
            accepted, rounds, planes, _ = R.decode_file(f, S, MAX_ROUNDS)
            want = (accepted, rounds, D.coef_crc(planes) if accepted else 0)
            assert tuple(int(x) for x in line.split()) == want, (name, S)
            seen.add(accepted)
    assert seen == {0, 1}
