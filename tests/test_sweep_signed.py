"""CPU checks of the signed leaf sweep of k_render_pool ("Round 17"): ptc::sweep_mask_signed_piped on
the signed table (pt_cull.h) against ptc::sweep_mask on the {lo, hi} table -- random rays and tables at every n in
1..32, the sweep model's Cornell rays, and adversarial families (tests/cull/sweep_signed_check.cpp, which compiles the
kernel's own header for the host) -- and the planner's LDS account of the second table.  tests/test_gpu_sweep_signed.py
holds the device side.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import fuzz_scenes
import pt_host as H
import test_gpu_path_pool
from test_launch_plan import LDS_CU, scene
from test_leaf_sweep import CSRC, CXX, REPO, SWEEP_MAX_LEAVES, n_leaves, quad_rows, scene_with_leaves, write_scene_bin
from test_pool_plan import POOLED, dump, pool_case  # noqa: F401  (dump: the planner on the host, a fixture)

TESTED_DEPTHS = (1, 2, 3, 4)        # one_depth<D> in sweep_signed_check.cpp
FAMILIES = ("d_edge", "zero_bound", "zero_addend", "flat", "t0_inf", "t0_low")


@pytest.fixture(scope="module")
def signed_check(tmp_path_factory, cornell_scene):
    d = tmp_path_factory.mktemp("sweep_signed")
    exe, path = str(d / "sweep_signed_check"), str(d / "scene.bin")
    subprocess.check_call(CXX + ["-o", exe, os.path.join(REPO, "tests", "cull", "sweep_signed_check.cpp"),
                                 os.path.join(CSRC, "pt_scene_pack.cpp"), os.path.join(CSRC, "pt_wide.cpp"),
                                 os.path.join(CSRC, "pt_scene.cpp")])
    write_scene_bin(cornell_scene, path)
    r = subprocess.run([exe, path, "24"], capture_output=True, text=True)
    assert r.returncode in (0, 1), (r.stdout, r.stderr[-2000:])
    words = r.stdout.strip().splitlines()[-1].split()
    got = {k: int(v) for k, v in zip(words[::2], words[1::2])}
    got["stderr"] = r.stderr[-2000:]
    print(got)
    return got


def test_signed_sweep_equals_the_plain_loop(signed_check):
    got = signed_check
    assert got["mismatches"] == 0, got
    assert got["octants"] == 0xff and got["infinite"] > 0, got
    assert got["random"] == 40 * 24 * 32 and got["cornell"] > 10000 and got["leaves"] == 18, got


def test_builder_matches_the_sweep_records(signed_check):
    assert signed_check["builder_bad"] == 0, signed_check


@pytest.mark.parametrize("family", FAMILIES)
def test_adversarial_families_reach_both_verdicts(signed_check, family):
    """Every family runs, and in each some case reaches a box that passes and some case one that fails: the equal masks
    are not equal because they are all empty or all full."""
    got = signed_check
    assert got[family] >= 12 * 16 * 32, got
    assert got[family + "_true"] > 0 and got[family + "_false"] > 0, got


def test_the_kernel_depth_is_a_tested_one():
    text = open(os.path.join(CSRC, "pt_render_pool.h")).read()
    m = re.search(r"#ifndef PT_POOL_SWEEP_DEPTH\s*\n#define PT_POOL_SWEEP_DEPTH (\d+)", text)
    assert m, "PT_POOL_SWEEP_DEPTH has no default"
    assert int(m.group(1)) in TESTED_DEPTHS
    m = re.search(r"#ifndef PT_POOL_SWEEP_SIGNED\s*\n#define PT_POOL_SWEEP_SIGNED (\d+)", text)
    assert m and int(m.group(1)) == 1, "the signed sweep is not the default"


def facts_of(sc):
    """The planner's scene facts of an uploaded scene, as far as the pool's LDS account reads them."""
    size = lambda k, floats: np.asarray(sc[k], np.float32).size // floats      # noqa: E731
    return scene(size("nodes", 12), n_leaves(sc), n_mats=size("mats", 16), n_spheres=size("spheres", 8))


def test_every_pinned_pooled_scene_still_pools(dump):
    """With the signed table in the place of the {lo, hi} copy (3 quads per leaf instead of 2) every scene an existing
    test pins as pooled keeps two workgroups per CU, 16 waves: test_pool_plan.py's POOLED, test_gpu_path_pool.py's
    FUZZ_POOLED (one of them 24 leaves with 13 materials: both tables side by side, 5 quads per leaf, would cost it a
    workgroup per CU), scene_with_leaves(n) up to the mask's cap, quad_rows(11)."""
    cases = list(POOLED)
    for seed, n_tris, cut in test_gpu_path_pool.FUZZ_POOLED:
        sc, _ = fuzz_scenes.random_case(seed, n_tris=n_tris)
        if cut:
            sc = H.SceneBuffers(sc)
            sc["spheres"] = np.array(sc["spheres"][:1], np.float32)
        cases.append(pool_case(facts=facts_of(sc)))
    for n in range(2, SWEEP_MAX_LEAVES + 1):
        cases.append(pool_case(facts=facts_of(scene_with_leaves(n))))
    cases.append(pool_case(facts=facts_of(quad_rows(11))))
    cases.append(pool_case(facts=scene(47, 24, n_mats=13)))
    assert max(c["n_leaves"] for c in cases) == SWEEP_MAX_LEAVES and max(c["n_mats"] for c in cases[:-1]) >= 13
    for c, r in zip(cases, dump(cases)):
        assert r["pool"] == 1, (c, r)
        signed = (4 * c["n_slots"] + 3 * c["n_mats"] + 2 * c["n_spheres"] + 3 * c["n_leaves"]) * 16
        assert r["pool_lds_bytes"] >= signed + (r["pool_nt"] // 64) * (r["pool_paths"] * 80 + (r["pool_paths"] + 15) // 16 * 16), (c, r)
        if c["width"] == 1920 and c["rows_local"] == 1080:
            assert r["per_cu"] * (r["pool_nt"] // 64) == 16 and r["per_cu"] * r["pool_lds_bytes"] <= LDS_CU, (c, r)
    (cornell,), (full,) = dump([pool_case()]), dump([pool_case(facts=scene(47, 24))])
    assert cornell["pool_lds_bytes"] - 8 * 9408 == 3728 and full["pool_lds_bytes"] - 8 * 9408 == 4784
