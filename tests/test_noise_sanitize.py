"""ASan + UBSan (with float-cast-overflow) run of pt_noise_host, next to the host ingest's
(tests/test_sanitize.py): tests/sanitize/noise_host_san.cpp is a stand-alone program linked
with csrc/pt_noise.cpp, so the per-pixel code the device kernels share (csrc/pt_noise.h) meets
moments of every bit pattern on the host.  Any sanitizer report aborts it.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(REPO, "tests", "sanitize", "noise_host_san.cpp"),
       os.path.join(REPO, "opengl-path-tracing_amd", "csrc", "pt_noise.cpp")]


def test_noise_host_under_asan_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "noise_host_san")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                        "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                        "-o", exe] + SRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "noise_host_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
