"""The cases of the device twin (tests/device/device_twin.hip), judged on the CPU alone.

The device twin runs the device compilation of the pinned headers (pt_math.h, pt_cull.h, pt_wide.h,
pt_isect.h, pt_noise.h) case by case and compares words (tests/test_gpu_device_twin.py).  That says
something only if the cases reach the hard inputs, so before anything is asserted about the device,
tests/device/twin_host.cpp -- plain C++ over the same generators and the same family definitions --
must show, with the host compilation alone:
  * every boolean family reaches both verdicts in at least 1% of its cases;
  * at least 1% of the wide_next steps flush, and at least 100 groups of 64 consecutive steps (what
    one wave takes) hold both a flushing and a non-flushing step: the lane mix `if (__any(flush))`
    exists for;
  * every sweep table yields the empty mask and a mask of several bits;
  * no generator left its stated domain (the count of dropped cases is 0);
  * the host compilation agrees with every independent reference on every case.
The generators draw once per statement, so g++ here and the HIP compiler's host pass there build the
same cases: EXPECTED below is what both tests see.
"""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "opengl-path-tracing_amd")
HIPCC = "/opt/rocm/bin/hipcc"

# family: (cases, positives, boolean, has an independent reference) -- the host reference's counts at the
# default case set.  positives: slab / slab_wild / cull accept, sweep mask not empty, tri hit_triangle hits, aces
# not black, accumulate on, quantise below the cap of 64, target q above target_q, retire true, fold S1 > 1,
# wide_hits any child pending, wide_next flushes, rng normal > 0, vec dot(a, a) inside the fast forms' guard,
# guard inside, sphere distance above 1e-4, leaf_choice takes a triangle, pinhole right of the centre column,
# sky_depth with the sky on, bounce ends the path.
EXPECTED = {
    "slab": (2000003, 736846, True, True),
    "slab_wild": (500009, 163818, True, False),
    "cull": (1000003, 458318, True, True),
    "sweep": (500015, 237872, True, True),
    "tri": (1000003, 355647, True, True),
    "aces": (1000003, 979322, False, True),
    "accumulate": (200030, 100015, False, True),
    "noise_quantise": (300007, 231108, True, True),
    "noise_target": (100003, 48669, True, False),
    "noise_retire": (100003, 66895, True, False),
    "noise_fold": (20011, 18088, False, True),
    "wide_hits": (500009, 146994, True, False),
    "wide_next": (1000003, 13170, False, False),
    "math_rng": (1048579, 523977, False, False),
    "math_vec": (500009, 283099, False, False),
    "guard": (100003, 43975, True, True),
    "sphere": (100003, 52813, True, True),
    "leaf_choice": (100003, 39281, True, True),
    "pinhole": (100003, 54958, False, True),
    "sky_depth": (100003, 87641, False, False),
    "bounce": (100003, 91441, False, False),
}


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("twin") / "twin_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-march=x86-64-v3", "-Wall", "-o", exe,
                           os.path.join(REPO, "tests", "device", "twin_host.cpp"),
                           os.path.join(REPO, "oracle", "pt_oracle.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)   # the whole default set: about 3 s
    assert r.returncode in (0, 1), r.stderr[:2000]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    fams = {l["family"]: l for l in lines if "family" in l}
    cov = [l for l in lines if l.get("coverage")]
    assert len(cov) == 1, r.stdout[-2000:]
    return {"families": fams, "coverage": cov[0], "rc": r.returncode, "stderr": r.stderr[:4000]}


def test_every_family_is_there_with_its_case_count(result):
    assert sorted(result["families"]) == sorted(EXPECTED)
    for name, (cases, positives, boolean, has_ref) in EXPECTED.items():
        f = result["families"][name]
        assert (f["cases"], f["positives"], f["boolean"], f["has_ref"]) == (cases, positives, boolean, has_ref), f
        assert cases % 64 != 0, name    # the last wave of its launch is partial


@pytest.mark.parametrize("name", [n for n, e in EXPECTED.items() if e[2]])
def test_boolean_families_reach_both_verdicts(result, name):
    f = result["families"][name]
    assert 0.01 * f["cases"] < f["positives"] < 0.99 * f["cases"], f


def test_wide_next_flushes_and_mixes_them_into_waves(result):
    """13170 of 1000003 steps push onto a full stack (1.3%), and 8905 of the 15625 groups of 64 consecutive cases
    hold both kinds of step: case i belongs to walk i % 4099, so a wave never holds one walk's steps alone."""
    cov, f = result["coverage"], result["families"]["wide_next"]
    assert cov["wide_next_flushes"] == f["positives"] == 13170
    assert cov["wide_next_flushes"] >= 0.01 * f["cases"]
    assert cov["wide_next_mixed_groups"] == 8905 and cov["wide_next_mixed_groups"] >= 100


def test_every_sweep_table_yields_the_empty_and_a_multi_bit_mask(result):
    """Tables of 1, 2, 17, 24 and 32 boxes, 100003 rays each.  A table of one box has no mask of several bits: there
    the two masks it has must both occur."""
    cov = result["coverage"]
    assert cov["sweep_n"] == [1, 2, 17, 24, 32]
    assert cov["sweep_zero"] == [59501, 54759, 50128, 47967, 49788]
    assert cov["sweep_multi"] == [0, 17975, 28257, 32197, 28457]
    for n, zero, multi in zip(cov["sweep_n"], cov["sweep_zero"], cov["sweep_multi"]):
        assert 0 < zero < 100003, n
        assert multi > 0 or n == 1, n


def test_no_case_is_dropped(result):
    """slab, cull, sweep and wide_hits cases are built inside the exact-reciprocal guard; one that is not would be
    counted here instead of being skipped."""
    assert result["coverage"]["dropped"] == 0
    assert result["coverage"]["aces_boundaries"] == 255


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_host_compilation_equals_the_reference(result, name):
    """slab_fast / slab_oct against the IEEE chain, slab_oct_cons against sweep_hit, sweep_mask against the mask of
    sweep_hit verdicts, the triangle tests and the tonemap against the oracle, the running mean, quantise and the
    moment fold against their double-rounded definitions, the guard and the leaf's choice against the float compares
    of tests/ref_walk.h, the sphere distance against the oracle's hit_sphere, the film coordinates against the
    reference's division.  (Families without a reference report 0 by construction.)"""
    assert result["families"][name]["host_vs_ref"] == 0, result["stderr"]
    assert result["rc"] == 0


def test_device_twin_cross_compiles():
    """The device program and its mutant build for gfx950 from the Makefile's own flags."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc at " + HIPCC + ": the device twin cannot be compiled here")
    subprocess.check_call(["make", "-s", "-j", "2", "-C", PKG, "build/device_twin", "build/device_twin_nodiv"])
    for exe in ("device_twin", "device_twin_nodiv"):
        assert os.path.getsize(os.path.join(PKG, "build", exe)) > 0
