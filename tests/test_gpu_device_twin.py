"""The device compilation of the pinned headers, case by case (tests/device/device_twin.hip).

The CPU suite runs the HOST compilation of pt_math.h, pt_cull.h, pt_wide.h, pt_isect.h and pt_noise.h on
millions of adversarial cases; the GPU suite compares whole renders.  A render reaches a t one ulp beside an
entry distance, a hit point on an edge, the least x of an ACES byte, frame 2^24 + 1 or a full wide stack in
some lanes of a wave by accident if at all -- and there the device runs other text than the host: v_med3 for
fminf, the ballot-fed v_addc_co of sweep_push, `if (__any(flush))`, v_ldexp, the compiler's division
expansion.  The device twin runs the cases of tests/test_device_twin_cases.py (whose coverage that test
asserts on the CPU) through one plain kernel per family and compares the result words with the host
compilation's and with the independent references, with no tolerance.

Two more runs show that the program can see an error at all: with --nudge the device's copy of every case has
one operand moved by its smallest step, and device_twin_nodiv is built without the correctly rounded divide.
"""
import json
import os
import subprocess

import pytest

from test_device_twin_cases import EXPECTED

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "opengl-path-tracing_amd")

# Measured on an MI355X node (profiles/device_twin.json): `make -j2` builds both programs from nothing in 3.5 s, and
# one run takes 2.0 s, of which the kernels are milliseconds: the rest generates the cases and evaluates them on the
# host.  The limits are ten times that or more.
BUILD_TIMEOUT = 60
RUN_TIMEOUT = 25


def _run(args):
    """One run of the program: its JSON lines by family.  A HIP error (exit 2), a signal or a timeout raises."""
    r = subprocess.run(args, capture_output=True, text=True, timeout=RUN_TIMEOUT, cwd=PKG)
    assert r.returncode in (0, 1), "%s ended with %d\n%s" % (args, r.returncode, r.stderr[-2000:])
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines and lines[-1].get("done"), r.stdout[-2000:]
    return {"families": {l["family"]: l for l in lines if "family" in l}, "rc": r.returncode, "stderr": r.stderr[:4000]}


@pytest.fixture(scope="module")
def twin():
    # The three runs come one after another, and the first that ends in a HIP error, a signal or a timeout fails
    # the fixture there: nothing more is started on the GPU.
    subprocess.run(["make", "-s", "-j", "2", "-C", PKG, "build/device_twin", "build/device_twin_nodiv"], check=True,
                   timeout=BUILD_TIMEOUT)
    out = {"pinned": _run(["build/device_twin"])}
    out["nudge"] = _run(["build/device_twin", "--nudge"])
    out["nodiv"] = _run(["build/device_twin_nodiv"])
    return out


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_device_equals_host_and_reference(twin, name):
    """Under the library's flags every family has no mismatch, device against the host compilation and device
    against the independent reference, on exactly the cases whose coverage the CPU test asserts."""
    run = twin["pinned"]
    assert sorted(run["families"]) == sorted(EXPECTED)
    cases, positives, boolean, _ = EXPECTED[name]
    f = run["families"][name]
    assert f["cases"] == cases and f["positives"] == positives, f
    assert f["dev_vs_host"] == 0 and f["dev_vs_ref"] == 0, run["stderr"]
    if boolean:
        assert 0.01 * cases < f["positives"] < 0.99 * cases, f
    assert run["rc"] == 0


def test_a_one_step_nudge_shows_in_every_family(twin):
    """t, a pixel component or a moment one ulp away, the verdict fed to sweep_push inverted, the lowest bit of
    pend flipped, on the device's side only: every family reports it."""
    run = twin["nudge"]
    assert sorted(run["families"]) == sorted(EXPECTED)
    for name, f in run["families"].items():
        assert f["nudge"] is True and f["dev_vs_host"] > 0, f
    assert run["rc"] == 1


def test_the_build_without_exact_division_is_caught(twin):
    """-fno-hip-fp32-correctly-rounded-divide-sqrt in place of the pinned flag: the running mean's divisions, and
    those of the IEEE slab chain or the tonemap, stop matching the host.  The families without a division or a
    square root of the compiler's stay equal, so the mismatches are the flag's and not the build's."""
    fam = twin["nodiv"]["families"]
    assert fam["accumulate"]["dev_vs_host"] > 0, fam["accumulate"]
    assert fam["slab"]["dev_vs_host"] > 0 or fam["aces"]["dev_vs_host"] > 0
    for name in ("cull", "sweep", "wide_hits", "wide_next", "math_rng", "noise_target", "noise_retire", "noise_fold"):
        assert fam[name]["dev_vs_host"] == 0, fam[name]
    assert twin["nodiv"]["rc"] == 1
