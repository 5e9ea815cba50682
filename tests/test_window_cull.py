"""CPU checks of the culling walk's window clause (pt_cull.h).

tests/cull/window_cull_sim.cpp runs the kernel's own node test, per-ray addends and the
uploader's window slack (ptc::cull_hit / cull_addends / window_slack, compiled for the host)
beside the reference's binary32 walk (calculateRayCollision, computeShader.c:367-432) on
diffuse paths and adversarial rays, and fails on
  (a) a segment whose final t (bitwise) or triangle differs from the reference's,
  (b) a leaf at which the reference accepts a triangle while the clause rejects that leaf or
      one of its ancestors,
  (c) a node the exact test accepts and the conservative test (without the clause) rejects.
The GPU parity tests (tests/test_gpu_window_cull.py) then compare the kernel with the oracle.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import fuzz_scenes
import pt_host as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cull", "window_cull_sim.cpp")
ADVERSARIAL = 100000      # rays per scene


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    d = tmp_path_factory.mktemp("cull")
    exe = str(d / "window_cull_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-march=x86-64-v3", "-o", exe, SRC])

    def run(sb, stride=32, bounces=8, adversarial=ADVERSARIAL):
        path = str(d / "scene.bin")
        with open(path, "wb") as f:
            np.array([len(sb["tris"]), len(sb["nodes"]), len(sb["spheres"])], np.int32).tofile(f)
            for k in ("tris", "nodes", "spheres", "cam"):
                np.ascontiguousarray(sb[k], np.float32).tofile(f)
        r = subprocess.run([exe, path, str(stride), str(bounces), str(adversarial)], capture_output=True, text=True)
        assert r.returncode in (0, 1, 3), r.stderr
        out = json.loads(r.stdout.strip().splitlines()[-1])
        out["rc"], out["stderr"] = r.returncode, r.stderr
        return out
    return run


def _ok(res):
    assert res["rc"] == 0, res["stderr"][:2000]
    assert res["mismatches"] == 0 and res["window_violations"] == 0 and res["cons_violations"] == 0, res["stderr"][:2000]
    assert res["adv_segments"] > 0.5 * ADVERSARIAL      # most adversarial rays are inside the guard


def moved(sb, offset=(0.0, 0.0, 0.0), scale=1.0):
    """The scene's triangles, spheres and camera scaled about the origin, then translated; the
    tree is rebuilt from the moved triangles."""
    off = np.asarray(offset, np.float32)
    tris = np.array(sb["tris"], np.float32).copy()
    for c in (0, 4, 8):
        tris[:, c:c + 3] = tris[:, c:c + 3] * np.float32(scale) + off
    cam = np.array(sb["cam"], np.float32).copy()
    cam[0:3] = cam[0:3] * np.float32(scale) + off
    out = H.scene_from_arrays(tris, sb["mats"], builtins=False, camera=cam)
    sph = np.array(sb["spheres"], np.float32).copy()
    if len(sph):
        sph[:, 0:3] = sph[:, 0:3] * np.float32(scale) + off
        sph[:, 3] *= np.float32(scale)
    out["spheres"] = sph
    return out


def thin_scene():
    """Parallel quads 1.2e-4 apart (and a slanted one through them) inside a 2e-3 cell: hits of
    rays between them fall around the acceptance threshold 1e-4."""
    tris = []
    s = 2e-3

    def quad(p00, p10, p11, p01):
        for a, b, c in ((p00, p10, p11), (p00, p11, p01)):
            t = np.zeros(16, np.float32)
            t[0:3], t[4:7], t[8:11] = a, b, c
            tris.append(t)
    for k in range(5):
        z = 1.2e-4 * k
        quad((0, 0, z), (s, 0, z), (s, s, z), (0, s, z))
    quad((0, 0, -1e-4), (s, 0, -1e-4), (s, s, 6e-4), (0, s, 6e-4))
    quad((0.25 * s, 0, -1e-4), (0.25 * s + 1.2e-4, 0, -1e-4), (0.25 * s + 1.2e-4, s, 6e-4), (0.25 * s, s, 6e-4))
    mats = np.zeros((1, 16), np.float32)
    mats[0, 0:3] = 0.7
    cam = np.array([0.5 * s, -3 * s, 3e-4, 0, 0, 1, 0.02, 0, 0, 0, 0, 0], np.float32)
    return H.scene_from_arrays(np.stack(tris), mats, builtins=False, camera=cam)


def test_cornell_paths_and_adversarial(sim, cornell_scene):
    """Cornell's diffuse paths: the reference's results on every segment, and the clause alone
    removes at least a quarter of the reference's leaf visits (a float64 model of the walk with
    a bare `far >= 0.5e-4` clause removes 48%; the kernel's clause carries the lemma's slack)."""
    res = sim(cornell_scene, stride=8)
    print({k: v for k, v in res.items() if k != "stderr"})
    _ok(res)
    assert res["path_segments"] > 100000
    assert res["window_on"] and res["window_slack"] < 5e-5
    assert res["path_removed_frac"] >= 0.25, res
    assert res["path_on_leaves"] < 0.75 * res["path_off_leaves"] and res["path_on_nodes"] <= res["path_off_nodes"]


def test_ship(sim, ship_scene):
    res = sim(ship_scene, stride=24)
    print({k: v for k, v in res.items() if k != "stderr"})
    _ok(res)


@pytest.mark.parametrize("seed", [3, 4, 5, 13, 22, 31])
def test_fuzz_scenes(sim, seed):
    """Triangle soups with flat quads, degenerate and duplicate triangles, floors (tests/fuzz_scenes.py)."""
    sc, _ = fuzz_scenes.random_case(seed)
    res = sim(sc, stride=96)
    print({k: v for k, v in res.items() if k != "stderr"})
    _ok(res)


def test_hits_around_the_threshold(sim):
    """True hits between 0.5e-4 and 4e-4: the clause must keep every leaf whose triangle is
    accepted just above 1e-4, and does cull leaves that end just below it."""
    res = sim(thin_scene(), stride=16)
    print({k: v for k, v in res.items() if k != "stderr"})
    _ok(res)
    assert res["window_on"] and res["window_slack"] < 1e-6
    assert res["near_hits"] > 2000 and res["adv_removed"] + res["path_removed"] > 2000, res


def test_cornell_scaled_to_the_threshold(sim, cornell_scene):
    """Cornell shrunk so that its whole box is a few acceptance thresholds wide."""
    res = sim(moved(cornell_scene, scale=1e-4), stride=24)
    print({k: v for k, v in res.items() if k != "stderr"})
    _ok(res)
    assert res["near_hits"] > 2000, res


def test_translated_scene(sim, cornell_scene):
    """Scene and camera moved by (1000, -3000, 500): the slack grows with the coordinates (the
    hit point itself is only known to a few ulps of 3000), so the clause culls little there --
    and never a leaf the reference accepts."""
    res = sim(moved(cornell_scene, offset=(1000.0, -3000.0, 500.0)), stride=16)
    print({k: v for k, v in res.items() if k != "stderr"})
    _ok(res)
    assert res["window_on"]
