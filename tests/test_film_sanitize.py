"""ASan + UBSan (with float-cast-overflow) run of pt_film_expose_host, after the pattern of
tests/test_camera_sanitize.py: tests/sanitize/film_host_san.cpp is a stand-alone program with its own main, linked with
the host sources an exposure needs (csrc/pt_film.cpp, pt_query.cpp, the packer and what it calls), so the per-pixel
code the device kernel shares (csrc/pt_film.h on csrc/pt_camera.h) meets the fuzz scenes, the four models, cameras and
priors of arbitrary bit patterns, the sizes 1 x 1 and 1 x 65536 and guide_frames above and below the frame range on the
host.  Any sanitizer report aborts it.  No Python runs under a sanitizer.  No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import query_cases as QC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "opengl-path-tracing_amd", "csrc")
SRC = [os.path.join(REPO, "tests", "sanitize", "film_host_san.cpp")] + \
      [os.path.join(CSRC, f) for f in ("pt_film.cpp", "pt_query.cpp", "pt_scene_pack.cpp", "pt_wide.cpp", "pt_scene.cpp")]
SCENES = ["fuzz1", "fuzz2", "fuzz24", "fuzz300", "fuzz700", "tiny300", "spheres_only"]


def test_film_host_under_asan_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.fail("no host C++ compiler")
    files = []
    for name in SCENES:
        sc = QC.scene(name)
        parts = [np.ascontiguousarray(sc[k], np.float32).reshape(-1) for k in ("tris", "nodes", "mats", "spheres")]
        counts = np.array([len(sc["tris"]), len(sc["nodes"]), len(sc["mats"]), len(sc["spheres"]), 0], np.int32)
        path = str(tmp_path / (name + ".scene"))
        with open(path, "wb") as f:
            f.write(counts.tobytes())
            for p in parts:
                f.write(p.tobytes())
        files.append(path)
    exe = str(tmp_path / "film_host_san")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                        "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                        "-o", exe] + SRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "film_host_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
