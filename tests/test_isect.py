"""The per-ray arithmetic of the render kernels (csrc/pt_isect.h), run on the CPU.

tests/isect/isect_check.cpp calls the functions the kernels call -- slab_fast, slab_oct, tri_plane,
tri_mt, aces_px, accumulate -- on the host and compares bit patterns, with no tolerance:
the two Markstein slab tests with the IEEE division chain `slab` on triples built inside the
exact-reciprocal guard, the triangle tests and the tonemap with the oracle, the
running mean with its definition in correctly rounded binary32.  This layer sits between the
CPU-checked headers (pt_math.h, pt_cull.h, pt_wide.h) and the kernel; before, only a GPU run
executed it.
"""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("isect") / "isect_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-march=x86-64-v3", "-Wall", "-o", exe,
                           os.path.join(REPO, "tests", "isect", "isect_check.cpp"),
                           os.path.join(REPO, "oracle", "pt_oracle.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode in (0, 1), r.stderr[:2000]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    out["rc"], out["stderr"] = r.returncode, r.stderr[:2000]
    return out


def test_slab_fast_and_slab_oct_equal_the_ieee_chain(result):
    """2e6 (box, ray, t) triples inside the guard -- flat boxes, origins on a face and inside the
    box, t = +inf, t at the near quotient and one ulp either side, boxes at both guard edges: the
    verdicts of slab_fast and slab_oct (bounds near-first by the sign of d) equal slab's on every
    one.  The generator stays inside the guard by construction, so none is skipped."""
    assert result["slab_triples"] == 2000000 and result["slab_outside_guard"] == 0, result["stderr"]
    assert result["slab_fast_mismatches"] == 0 and result["slab_oct_mismatches"] == 0, result["stderr"]
    # the sample reaches both verdicts
    assert 1000 < result["slab_hits"] < result["slab_triples"] - 1000


def test_triangle_plane_and_edges_equal_the_oracle(result):
    """ptp::tri_plane + pti::tri_plane + the edge tests, composed as hit_triangle, against
    oracle_hit_triangle on 1e6 triangle / ray pairs: degenerate triangles, rays parallel to the
    plane (quotient +-inf or NaN), hit points on an edge or a vertex."""
    assert result["tri_pairs"] == 1000000 and result["tri_mismatches"] == 0, result["stderr"]
    assert 1000 < result["tri_hits"] < result["tri_pairs"] - 1000


def test_moller_trumbore_equals_the_oracle(result):
    assert result["mt_mismatches"] == 0, result["stderr"]
    assert result["mt_hits"] > 1000


def test_aces_equals_the_oracle(result):
    """1e6 RGBA values: 0, negatives, NaN, inf, random bit patterns, and 3 ulps either side of the
    least x that maps to each of the bytes 1..255."""
    assert result["aces_pixels"] == 1000000 and result["aces_boundaries"] == 255
    assert result["aces_mismatches"] == 0, result["stderr"]


def test_accumulate_equals_its_definition(result):
    """prev*w + rgb/ff, w = (ff-1)/ff, without contraction: frames 1, 2, 3, 2986 and 2^24+1, and
    accumulate off."""
    assert result["accum_cases"] == 200000 and result["accum_mismatches"] == 0, result["stderr"]
    assert result["rc"] == 0
