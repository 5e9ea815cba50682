"""The window clause of the LDS culling walk (pt_cull.h, tuning key 22) on the
GPU: every case renders the oracle's words with the clause on and with it off, on the specialised
line and on a generic culling line, and pt_debug_window_cull reports the clause where it is
expected.  tests/test_window_cull.py holds the CPU model and the scenes shared with it.
"""
import numpy as np
import pytest

import fuzz_scenes
import oracle_lib as O
import pt_host as H
from test_gpu_parity import assert_bitwise
from test_window_cull import moved, thin_scene

pytestmark = pytest.mark.gpu

BOUNCES = 8


def both(sc, label, W, Hh, n_frames, frame_first=1, max_bounce=BOUNCES, mode=1, flags=0, expect_active=True,
         expect_walk=True, warm=False):
    """Oracle parity with the clause on and off; -> (generic, specialised) launches of the two renders."""
    want = O.render(sc, W, Hh, max_bounce=max_bounce, mode=mode, frame_first=frame_first, n_frames=n_frames, flags=flags)
    pt = H.PathTracer(W, Hh, max_bounce=max_bounce, display_mode=mode, flags=flags)
    pt.upload(sc)
    if warm:        # a learned tile order: the default configuration then runs the specialised line
        pt.render(1, 1, 0)
        pt.render(1, 64, 0)
    assert pt.diag()["culling_walk"] == expect_walk, label
    ran = {}
    for on in (True, False):
        pt.set_window_cull(on)
        active, slack = pt.window_cull()
        assert active == (on and expect_active), (label, on, active, slack)
        assert np.isfinite(slack) and (slack > 0 or not expect_active), (label, slack)
        before = pt.launches()
        pt.render(frame_first, n_frames, 0)
        after = pt.launches()
        ran[on] = (after[0] - before[0], after[1] - before[1])
        assert_bitwise(pt.read_rgba32f(), want, "%s, clause %s" % (label, "on" if on else "off"))
    pt.close()
    return ran


def test_cornell_specialised_line(cornell_scene):
    """Frames 1..4 at 64x48: the clause's c_lo is a constant of the specialised kernel; key 22 = 1
    sends the launch to the generic line."""
    ran = both(cornell_scene, "cornell, specialised line", 64, 48, 4, warm=True)
    assert ran[True] == (0, 1) and ran[False] == (1, 0), ran


@pytest.mark.parametrize("name,kw", [("no_sky", dict(flags=H.PT_FLAG_NO_SKY)), ("normals", dict(mode=2))])
def test_cornell_generic_culling_line(cornell_scene, name, kw):
    ran = both(cornell_scene, "cornell, generic line (%s)" % name, 64, 48, 4, warm=True, **kw)
    assert ran[True][1] == 0 and ran[False][1] == 0, ran


def test_mid_size_lds_scene_and_ship(tmp_path, ship_scene):
    import pt_scenes
    sc = H.setupBuffers(*pt_scenes.write_scene("bunny", str(tmp_path), target_tris=80))
    pt = H.PathTracer(8, 8)
    pt.upload(sc)
    active = pt.window_cull()[0]        # whatever the uploader decided for this mesh, parity holds
    pt.close()
    both(sc, "80-triangle LDS scene", 48, 32, 4, expect_active=active)
    # ship walks global memory (no LDS culling walk): the clause is not in its kernels
    pt = H.PathTracer(8, 8)
    pt.upload(ship_scene)
    d, active = pt.diag(), pt.window_cull()[0]
    pt.close()
    both(ship_scene, "ship", 48, 32, 2, expect_active=active, expect_walk=d["culling_walk"])


def test_grazing_origins(cornell_scene):
    """The camera on the floor plane looking along it: origins with a zero coordinate on a box face."""
    sc = H.SceneBuffers(cornell_scene)
    sc["cam"] = np.array([0.3, 0.2, 0.0, 0, 0.1, 1.0, 0.0, 0, 0, 0, 0, 0], np.float32)
    both(sc, "camera on the floor plane", 32, 24, 4)


def test_hits_around_the_threshold(cornell_scene):
    both(thin_scene(), "parallel quads 1.2e-4 apart", 32, 24, 4)
    both(moved(cornell_scene, scale=1e-4), "cornell scaled by 1e-4", 32, 24, 4)


def test_translated_scene(cornell_scene):
    both(moved(cornell_scene, offset=(1000.0, -3000.0, 500.0)), "cornell moved by (1000, -3000, 500)", 32, 24, 4)


@pytest.mark.parametrize("seed", [3, 4, 5, 13, 22, 31])
def test_fuzz_seeds(seed):
    sc, kw = fuzz_scenes.random_case(seed)
    pt = H.PathTracer(8, 8)
    pt.upload(sc)
    d, active = pt.diag(), pt.window_cull()[0]
    pt.close()
    both(sc, "fuzz seed %d" % seed, 32, 24, 4, frame_first=kw["frame_first"], max_bounce=kw["max_bounce"],
         mode=kw["mode"], flags=kw["flags"], expect_active=active, expect_walk=d["culling_walk"])


def test_some_fuzz_scene_and_every_cornell_runs_the_clause(cornell_scene):
    """The uploader's conditions (pt_cull.h) admit Cornell, its scaled and moved copies and the thin
    scene, and reject a soup with a degenerate triangle."""
    def active(sc):
        pt = H.PathTracer(8, 8)
        pt.upload(sc)
        a = pt.window_cull()
        pt.close()
        return a
    for sc in (cornell_scene, moved(cornell_scene, scale=1e-4), moved(cornell_scene, offset=(1000.0, -3000.0, 500.0)),
               thin_scene()):
        a, slack = active(sc)
        assert a and 0 < slack < 1e-2
    assert active(cornell_scene)[1] < 5e-5
    assert active(fuzz_scenes.random_case(3)[0])[1] > 0
    assert active(fuzz_scenes.random_case(4)[0]) == (False, 0.0)


def test_moller_trumbore_runs_without_the_clause(cornell_scene):
    """PT_FLAG_MOLLER_TRUMBORE accepts through another test and window (t > 1e-7): c_lo = -inf."""
    both(cornell_scene, "Moller-Trumbore", 64, 48, 4, flags=H.PT_FLAG_MOLLER_TRUMBORE, expect_active=False, warm=True)


def test_key_validation(cornell_scene):
    pt = H.PathTracer(16, 16)
    pt.upload(cornell_scene)
    with pytest.raises(H.PTError):
        pt.set_key(22, 2)
    pt.set_key(22, 1)
    assert pt.window_cull()[0] is False
    pt.set_key(22, 0)
    assert pt.window_cull()[0] is True
    pt.set_culling(False)           # no culling walk, no clause
    assert pt.window_cull()[0] is False
    pt.close()
