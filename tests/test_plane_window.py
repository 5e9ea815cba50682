"""CPU checks of the path pool's plane-window filter (pti::pair_in_window, csrc/pt_isect.h; DESIGN.md §5.12,
"Round 20"): the set-up pass of k_render_pool clears the candidate bit of the pair a bounce ray leaves when both of
the pair's plane distances are outside their hit windows at the segment's initial t0.

tests/pool/plane_window_sim.cpp runs the kernel's own candidate test, the packer's table and triangle quads and the
shared filter function (compiled for the host) beside the reference's binary32 walk (tests/ref_walk.h) and fails on a
segment whose final (t bitwise, triangle) through the filtered mask differs from the reference's.  Its `--cases` mode
runs the function on hand-made cases.  tests/pool/pool_hist_sim.cpp is tests/pool/pool_sim.cpp's cost model with the
histogram as an argument.  The GPU side is tests/test_gpu_plane_filter.py.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import fuzz_scenes
from test_leaf_sweep import CXX, SWEEP_MAX_LEAVES, quad_rows, scene_with_leaves, write_scene_bin

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "opengl-path-tracing_amd", "csrc")
ADVERSARIAL = 100000
SIM_SOURCES = [os.path.join(REPO, "tests", "pool", "plane_window_sim.cpp"), os.path.join(CSRC, "pt_scene_pack.cpp"),
               os.path.join(CSRC, "pt_wide.cpp"), os.path.join(CSRC, "pt_scene.cpp")]
# a soup of 24 leaves, the mask's cap, with non-coplanar pairs (tests/test_gpu_path_pool.py pools it)
SOUP = dict(seed=4, n_tris=40)


def soup():
    return fuzz_scenes.random_case(SOUP["seed"], n_tris=SOUP["n_tris"])[0]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("plane_window") / "plane_window_sim")
    subprocess.check_call(CXX + ["-o", path] + SIM_SOURCES)
    return path


@pytest.fixture(scope="module")
def sim(exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("plane_window_scenes")

    def run(sb, stride=32, bounces=8, adversarial=ADVERSARIAL):
        path = str(d / "scene.bin")
        write_scene_bin(sb, path)
        r = subprocess.run([exe, path, str(stride), str(bounces), str(adversarial)], capture_output=True, text=True)
        assert r.returncode in (0, 1), r.stderr
        out = json.loads(r.stdout.strip().splitlines()[-1])
        out["rc"], out["stderr"] = r.returncode, r.stderr
        return out
    return run


def _ok(res, adversarial=ADVERSARIAL):
    print({k: v for k, v in res.items() if k != "stderr"})
    assert res["rc"] == 0 and res["sweep_ok"], res["stderr"][:2000]
    assert res["mismatches"] == 0 and res["verdict_errors"] == 0, res["stderr"][:2000]
    assert res["adv_segments"] > 0.5 * adversarial      # most adversarial rays are inside the guard


@pytest.fixture(scope="module")
def cornell(sim, cornell_scene):
    """Cornell's diffuse 1080p paths at every 8th pixel, 8 bounces, and the adversarial rays: run once."""
    return sim(cornell_scene, stride=8)


def test_cornell_paths_and_adversarial(cornell):
    """The reference's (t, triangle) on every segment.  The figures of DESIGN.md §5.12, "Round 20", per segment: 1.43
    candidate visits, 0.30 of them the own pair outside its windows at t0 (20.9% of the visits); a filter over every
    bit would remove 0.31, and 0.48 are outside at the t current at the visit."""
    _ok(cornell)
    assert cornell["n_leaves"] == 18 and cornell["path_segments"] > 100000
    # the filter removes own-pair visits only, and every own-pair visit that is outside its windows at t0
    assert cornell["path_removed"] == cornell["path_outside_t0_own"] <= cornell["path_outside_t0"] <= cornell["path_outside_current"]
    assert abs(cornell["path_left"] - (cornell["path_candidates"] - cornell["path_removed"])) < 2e-4
    assert abs(sum(cornell["path_hist"]) - 1.0) < 1e-3
    # the issue's CPU measurement (140,421 segments): 1.4315 visits, 0.2991 removed, 0.3098 / 0.4773 outside
    assert abs(cornell["path_candidates"] - 1.4315) < 0.002 and abs(cornell["path_removed"] - 0.2991) < 0.002
    assert abs(cornell["path_outside_t0"] - 0.3098) < 0.002 and abs(cornell["path_outside_current"] - 0.4773) < 0.002


def test_sweep_cap_single_leaf_and_soup(sim):
    """The scene at the mask's cap (every bit in use), a single-triangle leaf (its pair is the triangle twice, flagged
    coplanar) and a soup at the cap with non-coplanar pairs, whose own-pair bit may have to stay."""
    res = sim(scene_with_leaves(SWEEP_MAX_LEAVES), stride=64, adversarial=20000)
    _ok(res, 20000)
    assert res["n_leaves"] == SWEEP_MAX_LEAVES
    _ok(sim(quad_rows(5, drop_last=True), stride=64, adversarial=20000), 20000)
    res = sim(soup(), stride=48, adversarial=50000)
    _ok(res, 50000)
    assert res["n_leaves"] == SWEEP_MAX_LEAVES and res["non_coplanar_pairs"] >= 4, res
    assert res["adv_removed"] > 0.01 and res["adv_outside_t0"] > res["adv_removed"], res


def test_hand_made_cases(exe):
    """1e-4 exactly for the first triangle (open) and the second (closed), a distance equal to t0, t0 = +inf, a zero
    denominator (+-inf) and NaN, a non-coplanar pair with only its second triangle in window, and a ray that starts on
    the pair's own plane with its origin moved 0..4 ulps either way."""
    r = subprocess.run([exe, "--cases"], capture_output=True, text=True)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and out["failed"] == 0 and out["cases"] >= 35, (out, r.stderr)


def test_model_under_sanitizers(tmp_path, cornell_scene):
    """The model is a plain program over the packer path and the shared function: built with ASan and UBSan it runs
    the hand-made cases, Cornell, the scene at the cap, the single-triangle leaf and the soup clean."""
    san = str(tmp_path / "plane_window_sim_san")
    subprocess.check_call(CXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san] + SIM_SOURCES)
    runs = [[san, "--cases"]]
    for i, sc in enumerate((cornell_scene, scene_with_leaves(SWEEP_MAX_LEAVES), quad_rows(5, drop_last=True), soup())):
        path = str(tmp_path / ("scene%d.bin" % i))
        write_scene_bin(sc, path)
        runs.append([san, path, "64", "8", "5000"])
    for cmd in runs:
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, (cmd, r.returncode, r.stderr[-2000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]


# ------------------------------------------------------------------ the pool's cost model on the filtered histogram
POOL_SIM_HIST = (0.137, 0.487, 0.246, 0.082, 0.048)    # tests/pool/pool_sim.cpp's own


@pytest.fixture(scope="module")
def cost(tmp_path_factory):
    d = tmp_path_factory.mktemp("pool_hist")
    exes = {}
    for name in ("pool_sim", "pool_hist_sim"):
        exes[name] = str(d / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exes[name],
                               os.path.join(REPO, "tests", "pool", name + ".cpp")])

    def run(name, *args):
        r = subprocess.run([exes[name]] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout.strip().splitlines()[-1])
    return run


def test_driver_is_pool_sims_model(cost):
    """With pool_sim's histogram the driver draws the same paths and prints pool_sim's figures."""
    for P in (96, 128):
        a, b = cost("pool_sim", P, 5000), cost("pool_hist_sim", P, 5000, *POOL_SIM_HIST)
        for k in ("segments", "shade_passes", "leaf_passes", "wave_valu_per_segment", "leaf_lane_use"):
            assert a[k] == b[k], (P, k, a, b)


def test_filtered_histogram_costs_fewer_leaf_passes(cost, cornell):
    """The model's figure beside the measured one: fewer path visits are fewer LEAF passes at the
    same lanes per pass.  The set-up pass pays 36 VALU for the filter on Cornell, whose pairs are all coplanar (one
    IEEE division; the compiled block)."""
    hist = cornell["path_hist"]
    base = cost("pool_hist_sim", 128, 20000, *POOL_SIM_HIST)
    head = cost("pool_hist_sim", 128, 20000, *hist, 756, 450, 30)
    print(base, head)
    assert head["leaf_passes"] < 0.85 * base["leaf_passes"] and head["leaf_lane_use"] > 0.9
    assert head["wave_valu_per_segment"] < base["wave_valu_per_segment"]
