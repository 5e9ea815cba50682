"""The leaf sweep (pt_cull.h sweep_mask, tuning key 23, DESIGN.md §5.6, "The leaf sweep") on the GPU: every case renders the
oracle's words with the sweep on and with it off (the culling walk), and pt_debug_sweep reports the sweep where it
is expected.  tests/test_leaf_sweep.py holds the CPU model and the scenes shared with it.
"""
import numpy as np
import pytest

import fuzz_scenes
import oracle_lib as O
import pt_host as H
from test_gpu_parity import assert_bitwise
from test_leaf_sweep import SWEEP_MAX_LEAVES, n_leaves, quad_rows, scene_with_leaves
from test_window_cull import moved, thin_scene

pytestmark = pytest.mark.gpu

BOUNCES = 8


def both(sc, label, W, Hh, n_frames=4, frame_first=1, max_bounce=BOUNCES, mode=1, flags=0, rpp=1, expect_swept=True,
         warm=False):
    """Oracle parity with the sweep on and off; -> (generic, specialised) launches of the two renders."""
    want = O.render(sc, W, Hh, max_bounce=max_bounce, mode=mode, frame_first=frame_first, n_frames=n_frames, flags=flags,
                    rpp=rpp)
    pt = H.PathTracer(W, Hh, max_bounce=max_bounce, display_mode=mode, flags=flags, rays_per_pixel=rpp)
    pt.upload(sc)
    if warm:        # a learned tile order: the default configuration then runs the specialised line
        pt.render(1, 1, 0)
        pt.render(1, 64, 0)
    assert (pt.leaf_sweep()["qualifies"] or not expect_swept) and pt.leaf_sweep()["n_leaves"] == n_leaves(sc), label
    ran = {}
    for on in (True, False):
        pt.set_sweep(on)
        before = pt.launches()
        pt.render(frame_first, n_frames, 0)
        after = pt.launches()
        ran[on] = (after[0] - before[0], after[1] - before[1])
        assert pt.leaf_sweep()["swept"] == (on and expect_swept) == pt.diag()["swept"], (label, on)
        assert_bitwise(pt.read_rgba32f(), want, "%s, sweep %s" % (label, "on" if on else "off"))
    pt.close()
    return ran


def test_cornell_specialised_line(cornell_scene):
    """Frames 1..4 at 64x48: the sweep is a constant of the specialised kernel, which has a build with it and one
    without."""
    ran = both(cornell_scene, "cornell, specialised line", 64, 48, warm=True)
    assert ran[True] == (0, 1) and ran[False] == (0, 1), ran


def test_cornell_generic_line(cornell_scene):
    ran = both(cornell_scene, "cornell, generic line (no sky)", 64, 48, warm=True, flags=H.PT_FLAG_NO_SKY)
    assert ran[True][1] == 0 and ran[False][1] == 0, ran


def test_grazing_origins(cornell_scene):
    """The camera on the floor plane looking along it: origins with a zero coordinate on a box face."""
    sc = H.SceneBuffers(cornell_scene)
    sc["cam"] = np.array([0.3, 0.2, 0.0, 0, 0.1, 1.0, 0.0, 0, 0, 0, 0, 0], np.float32)
    both(sc, "camera on the floor plane", 32, 24)


def test_rays_outside_the_guard_walk_beside_swept_ones(cornell_scene):
    """Without jitter and looking straight along +y, the middle column's camera rays have d.x = 0: they are outside
    the exact-reciprocal guard and walk the tree, in waves whose other rays sweep."""
    sc = H.SceneBuffers(cornell_scene)
    cam = np.array(cornell_scene["cam"], np.float32).copy()
    cam[4:7] = [0.0, 1.0, 0.0]
    sc["cam"] = cam
    both(sc, "axis-parallel camera rays", 32, 24, flags=H.PT_FLAG_NO_AA)


def test_hits_around_the_threshold(cornell_scene):
    both(thin_scene(), "parallel quads 1.2e-4 apart", 32, 24)
    both(moved(cornell_scene, scale=1e-4), "cornell scaled by 1e-4", 32, 24)


def test_translated_scene(cornell_scene):
    both(moved(cornell_scene, offset=(1000.0, -3000.0, 500.0)), "cornell moved by (1000, -3000, 500)", 32, 24)


def test_scene_below_the_guard_walks(cornell_scene):
    """Cornell scaled by 2^-100 lies outside the scene half of the guard: no table, every ray walks."""
    both(moved(cornell_scene, scale=2.0 ** -100), "cornell scaled by 2^-100", 32, 24, expect_swept=False)


def test_leaf_count_cap():
    """A scene of exactly kSweepMaxLeaves leaves sweeps (every bit of the mask in use), one more leaf walks."""
    both(scene_with_leaves(SWEEP_MAX_LEAVES), "%d leaves" % SWEEP_MAX_LEAVES, 32, 24)
    both(scene_with_leaves(SWEEP_MAX_LEAVES + 1), "%d leaves" % (SWEEP_MAX_LEAVES + 1), 32, 24, expect_swept=False)


def test_single_triangle_leaf():
    sc = quad_rows(5, drop_last=True)
    nodes = np.array(sc["nodes"], np.float32).reshape(-1, 12)
    assert ((nodes[:, 8] > -1.0) & (nodes[:, 8] == nodes[:, 9])).any()
    both(sc, "a single-triangle leaf", 32, 24)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 10, 12])
def test_fuzz_seeds(seed):
    """Soups of 1 to 24 triangles with whatever camera, flags, mode and frames the seed draws."""
    sc, kw = fuzz_scenes.random_case(seed)
    pt = H.PathTracer(8, 8)
    pt.upload(sc)
    q = pt.leaf_sweep()["qualifies"] and pt.diag()["culling_walk"]
    pt.close()
    both(sc, "fuzz seed %d" % seed, 32, 24, frame_first=kw["frame_first"], max_bounce=kw["max_bounce"], mode=kw["mode"],
         flags=kw["flags"], expect_swept=q)


def test_some_fuzz_seed_sweeps():
    n = 0
    for seed in (0, 1, 2, 3, 10, 12):
        pt = H.PathTracer(8, 8)
        pt.upload(fuzz_scenes.random_case(seed)[0])
        n += pt.leaf_sweep()["qualifies"]
        pt.close()
    assert n >= 3


def test_moller_trumbore(cornell_scene):
    both(cornell_scene, "Moller-Trumbore", 64, 48, flags=H.PT_FLAG_MOLLER_TRUMBORE, warm=True)


def test_two_rays_per_pixel(cornell_scene):
    both(cornell_scene, "raysPerPixel 2", 16, 16, rpp=2)


def test_key_validation(cornell_scene):
    pt = H.PathTracer(16, 16)
    pt.upload(cornell_scene)
    with pytest.raises(H.PTError):
        pt.set_key(23, 2)
    with pytest.raises(H.PTError):
        pt.set_key(23, -1)
    pt.set_key(23, 1)
    pt.render(1, 1, 0)
    assert pt.leaf_sweep() == dict(swept=False, qualifies=True, n_leaves=18)
    pt.set_key(23, 0)
    pt.render(1, 1, 0)
    assert pt.leaf_sweep()["swept"] is True
    pt.set_culling(False)           # no culling walk, no sweep
    pt.render(1, 1, 0)
    assert pt.leaf_sweep()["swept"] is False and pt.diag()["culling_walk"] is False
    pt.close()
