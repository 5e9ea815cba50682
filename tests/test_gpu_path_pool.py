"""The path pool (k_render_pool, pt_pool.h, tuning key 24) on the GPU: every case renders the oracle's
words with the pool on and with it off (k_render_sm's swept line), and pt_debug_pool reports the pool where it is
expected.  The pool needs the specialised swept line (a learned tile order) and a launch without an overlap slot, so
the cases warm their context and render short launches on one stream (tuning key 9 = 1).  The shapes are the smallest
at which a pool can go wrong; tests/test_path_pool.py holds the CPU model of the lists.
"""
import numpy as np
import pytest

import fuzz_scenes
import oracle_lib as O
import pt_host as H
from test_gpu_parity import assert_bitwise
from test_leaf_sweep import SWEEP_MAX_LEAVES, quad_rows, scene_with_leaves
from test_window_cull import moved, thin_scene

pytestmark = pytest.mark.gpu

BOUNCES = 8


def context(sc, W, Hh, max_bounce=BOUNCES, **kw):
    """A context with a learned tile order and no overlap slots: its default-configuration launches may pool."""
    pt = H.PathTracer(W, Hh, max_bounce=max_bounce, **kw)
    pt.upload(sc)
    pt.set_key(9, 1)
    pt.render(1, 1, 0)
    pt.render(1, 64, 0)
    return pt


def both(sc, label, W, Hh, n_frames=4, frame_first=1, max_bounce=BOUNCES, mode=1, flags=0, rpp=1, expect_pool=True,
         keys=(), want=None, rows=slice(None), **kw):
    """Oracle parity with key 24 = 0 and = 1; the pool runs exactly where the case says."""
    if want is None:
        want = O.render(sc, W, Hh, max_bounce=max_bounce, mode=mode, frame_first=frame_first, n_frames=n_frames,
                        flags=flags, rpp=rpp)
    pt = context(sc, W, Hh, max_bounce=max_bounce, display_mode=mode, flags=flags, rays_per_pixel=rpp, **kw)
    for k, v in keys:
        pt.set_key(k, v)
    for on in (False, True):
        pt.set_pool(on)
        pt.render(frame_first, n_frames, 0)
        assert pt.pooled() == (on and expect_pool), (label, on)
        assert_bitwise(pt.read_rgba32f(), want[rows], "%s, pool %s" % (label, "on" if on else "off"))
    pt.close()


def test_fewer_ids_than_one_pool(cornell_scene):
    """8x8 is one tile: no tile order to learn, so the generic line (and no pool) renders it.  9x2 is two tiles with 18
    pixels inside: the specialised line, and fewer paths than one wave's pool ever fills."""
    both(cornell_scene, "8x8, 1 frame", 8, 8, n_frames=1, expect_pool=False)
    both(cornell_scene, "9x2, 1 frame", 9, 2, n_frames=1)


def test_one_pixel_more_than_a_pool(cornell_scene):
    """117 pixels in 15 tiles of which every one is partial: one path more than a 116-path pool, and one more than a
    pass of 64."""
    both(cornell_scene, "117x1, 2 frames", 117, 1, n_frames=2)
    both(cornell_scene, "65x1, 1 frame", 65, 1, n_frames=1)


def test_partial_tiles(cornell_scene):
    both(cornell_scene, "20x12", 20, 12, n_frames=3)


@pytest.mark.parametrize("group", [0, 4])
def test_launch_drains_mid_item(cornell_scene, group):
    """70 frames are no multiple of the frames per item, forced (key 5 = 4) or automatic."""
    both(cornell_scene, "16x16, 70 frames, key 5 = %d" % group, 16, 16, n_frames=70, keys=((5, group),))


def test_continuation(cornell_scene):
    """Frames 1..8, then 9..20 accumulated onto them: one render of 1..20."""
    want = O.render(cornell_scene, 16, 16, max_bounce=BOUNCES, n_frames=20)
    pt = context(cornell_scene, 16, 16)
    for on in (True, False):
        pt.set_pool(on)
        pt.render(1, 8, 0)
        assert pt.pooled() == on
        pt.render(9, 12, 1)
        assert pt.pooled() == on
        assert_bitwise(pt.read_rgba32f(), want, "1..8 then 9..20, pool %s" % ("on" if on else "off"))
    pt.close()


def test_row_share(cornell_scene):
    want = O.render(cornell_scene, 24, 18, max_bounce=BOUNCES, n_frames=5)
    both(cornell_scene, "rank 1 of 3, 24x18", 24, 18, n_frames=5, want=want, rows=slice(1, None, 3), rank=1, world=3)


def test_grazing_origins(cornell_scene):
    sc = H.SceneBuffers(cornell_scene)
    sc["cam"] = np.array([0.3, 0.2, 0.0, 0, 0.1, 1.0, 0.0, 0, 0, 0, 0, 0], np.float32)
    both(sc, "camera on the floor plane", 32, 24)


def test_rays_outside_the_guard_beside_swept_ones(cornell_scene):
    """A camera at x = 1e-13, below the guard's 2^-40: every camera ray is outside the guard and takes the pool
    kernel's cold walk, in passes whose other paths (bounce rays, from hit points) sweep.  The leaf-sweep suite's
    axis-parallel camera rays need the no-jitter flag, which is the generic line: that case must fall back."""
    sc = H.SceneBuffers(cornell_scene)
    cam = np.array(cornell_scene["cam"], np.float32).copy()
    cam[0] = 1e-13
    sc["cam"] = cam
    both(sc, "camera origin below the guard", 32, 24)
    cam[0] = cornell_scene["cam"][0]
    cam[4:7] = [0.0, 1.0, 0.0]
    sc["cam"] = cam
    both(sc, "axis-parallel camera rays", 32, 24, flags=H.PT_FLAG_NO_AA, expect_pool=False)


def test_hits_around_the_threshold(cornell_scene):
    # (thin_scene is built without the built-in sphere, and the specialised line holds one sphere as a constant: it
    # runs the generic line, so the pool must stay off and the image match; the scaled Cornell box is the pooled case)
    both(thin_scene(), "parallel quads 1.2e-4 apart", 32, 24, expect_pool=False)
    both(moved(cornell_scene, scale=1e-4), "cornell scaled by 1e-4", 32, 24)


def test_translated_scene(cornell_scene):
    both(moved(cornell_scene, offset=(1000.0, -3000.0, 500.0)), "cornell moved by (1000, -3000, 500)", 32, 24)


def test_camera_outside_the_root_box():
    both(quad_rows(11), "11 quads seen from outside their box", 32, 24)


def test_single_triangle_leaf():
    both(quad_rows(5, drop_last=True), "a single-triangle leaf", 32, 24)


# Seeded soups (tests/fuzz_scenes.py) that run the pool kernel, established once by rendering seeds 0..119 at their
# own size and at 12 and 40 triangles: a soup pools exactly when it has a sweep table (2 to 24 leaves), its root is no
# leaf and the built-in sphere is its only one -- about a quarter of the seeds draw no extra sphere; with the extra
# spheres cut to the built-in one every sweeping soup pooled.  (seed, n_tris or None = the seed's own, cut spheres):
# 7 to 40 triangles, 4 to 24 leaves (the mask's cap), 0 to 8 bounces, two scenes moved far from the origin; the soups
# mix degenerate and duplicate triangles, flat quads and large floor triangles in random order.
FUZZ_POOLED = [(29, None, False), (30, None, False), (74, None, False), (34, 12, False), (4, 40, False),
               (58, 40, False), (3, None, True), (2, None, True), (12, None, True)]
# ... and soups that must fall back and still match: a single triangle (the root is a leaf), extra spheres
FUZZ_FALLBACK = [(0, None, False), (2, None, False), (8, 40, False)]


def fuzz_case(seed, n_tris, cut):
    sc, kw = fuzz_scenes.random_case(seed, n_tris=n_tris)
    if cut:
        sc = H.SceneBuffers(sc)
        sc["spheres"] = np.array(sc["spheres"][:1], np.float32)
    return sc, kw


@pytest.mark.parametrize("seed,n_tris,cut", FUZZ_POOLED)
def test_fuzz_soups_pool(seed, n_tris, cut):
    """With the default mode and flags (the specialised line's), at the seed's frame number and bounce count."""
    sc, kw = fuzz_case(seed, n_tris, cut)
    both(sc, "fuzz seed %d (%s triangles%s)" % (seed, n_tris or "own", ", one sphere" if cut else ""), 32, 24,
         frame_first=kw["frame_first"], max_bounce=kw["max_bounce"], expect_pool=True)


@pytest.mark.parametrize("seed,n_tris,cut", FUZZ_FALLBACK)
def test_fuzz_soups_fall_back(seed, n_tris, cut):
    sc, kw = fuzz_case(seed, n_tris, cut)
    both(sc, "fuzz seed %d (%s triangles)" % (seed, n_tris or "own"), 32, 24, frame_first=kw["frame_first"],
         max_bounce=kw["max_bounce"], expect_pool=False)


def test_fallbacks(cornell_scene):
    both(cornell_scene, "raysPerPixel 2", 16, 16, rpp=2, expect_pool=False)
    both(cornell_scene, "Moller-Trumbore", 32, 24, flags=H.PT_FLAG_MOLLER_TRUMBORE, expect_pool=False)
    both(scene_with_leaves(SWEEP_MAX_LEAVES + 1), "%d leaves" % (SWEEP_MAX_LEAVES + 1), 32, 24, expect_pool=False)


def test_overlapped_short_launch_does_not_pool(cornell_scene):
    pt = H.PathTracer(32, 24, max_bounce=BOUNCES)
    pt.upload(cornell_scene)
    pt.render(1, 1, 0)
    pt.render(1, 64, 0)
    assert pt.pooled()
    pt.render(1, 4, 0)
    assert not pt.pooled()
    assert_bitwise(pt.read_rgba32f(), O.render(cornell_scene, 32, 24, max_bounce=BOUNCES, n_frames=4), "overlap slot")
    pt.close()


def test_cornell_sorted_order(cornell_scene):
    """64x32 for 80 frames: the tile order is learned and the sorted permutation runs with the pool."""
    both(cornell_scene, "cornell 64x32, 80 frames", 64, 32, n_frames=80)


def test_key_validation(cornell_scene):
    pt = H.PathTracer(16, 16)
    pt.upload(cornell_scene)
    for bad in (2, -1):
        with pytest.raises(H.PTError):
            pt.set_key(24, bad)
    pt.close()
