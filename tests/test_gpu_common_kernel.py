"""The specialised default-path kernel (k_render_sm<..., COMMON>, tuning key 21) on
the GPU: it renders the same words as the generic kernel and as the oracle, it is the line that
runs once a context has a learned tile order, and every launch outside its facts falls back to the
generic line.  64x48 is whole tiles; 72x40 has a partial tile column and a partial tile row.
"""
import numpy as np
import pytest

import oracle_lib as O
import pt_host as H
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (72, 40)]
LAUNCHES = (1, 5, 24)       # frames 1..n in one launch each
BOUNCES = 8


@pytest.fixture(scope="module")
def want(cornell_scene):
    """Oracle images of frames 1..n for each size, rendered once."""
    return {(W, Hh, n): O.render(cornell_scene, W, Hh, max_bounce=BOUNCES, n_frames=n)
            for W, Hh in SIZES for n in LAUNCHES + (8,)}


def warmed(cornell_scene, W, Hh, **kw):
    """A context whose tile order has been learned: its first launch (no order yet) ran the generic
    line, and a 64-frame render -- probe launch, sort, the rest -- leaves a sorted order."""
    pt = H.PathTracer(W, Hh, max_bounce=BOUNCES, **kw)
    pt.upload(cornell_scene)
    pt.render(1, 1, 0)
    assert pt.launches() == (1, 0), "a context's first launch has no learned tile order"
    pt.render(1, 64, 0)
    return pt


def render_counted(pt, n):
    before = pt.launches()
    pt.render(1, n, 0)
    after = pt.launches()
    return pt.read_rgba32f(), (after[0] - before[0], after[1] - before[1])


@pytest.mark.parametrize("W,Hh", SIZES)
def test_common_line_runs_and_matches(cornell_scene, want, W, Hh):
    pt = warmed(cornell_scene, W, Hh)
    assert pt.launches()[1] >= 1, "the 64-frame render's launch after the sort is on the specialised line"
    for n in LAUNCHES:
        pt.set_common(False)
        off, ran_off = render_counted(pt, n)
        pt.set_common(True)
        on, ran_on = render_counted(pt, n)
        assert ran_off == (1, 0) and ran_on == (0, 1), (n, ran_off, ran_on)
        assert_bitwise(on, off, "key 21 on vs off, %d frames" % n)
        assert_bitwise(on, want[W, Hh, n], "specialised line vs oracle, %d frames" % n)
    pt.close()


@pytest.mark.parametrize("W,Hh", SIZES)
@pytest.mark.parametrize("name,kw,okw", [("no_sky", dict(flags=2), dict(flags=2)),
                                         ("normals", dict(display_mode=2), dict(mode=2)),
                                         ("no_spheres", dict(flags=4), dict(flags=4))])
def test_fallback_to_the_generic_line(cornell_scene, W, Hh, name, kw, okw):
    pt = H.PathTracer(W, Hh, max_bounce=BOUNCES, **kw)
    pt.upload(cornell_scene)
    pt.render(1, 64, 0)
    got, ran = render_counted(pt, 5)
    total = pt.launches()
    pt.close()
    assert ran == (1, 0) and total[1] == 0, (name, ran, total)
    assert_bitwise(got, O.render(cornell_scene, W, Hh, max_bounce=BOUNCES, n_frames=5, **okw), name)


@pytest.mark.parametrize("W,Hh", SIZES)
def test_mode_set_after_create_falls_back(cornell_scene, want, W, Hh):
    """pt_set_display_mode is seen by the launch, not the planner: albedo falls back, shaded returns."""
    pt = warmed(cornell_scene, W, Hh)
    pt.set_display_mode(3)
    got, ran = render_counted(pt, 5)
    assert ran == (1, 0)
    assert_bitwise(got, O.render(cornell_scene, W, Hh, max_bounce=BOUNCES, n_frames=5, mode=3), "albedo")
    pt.set_display_mode(1)
    got, ran = render_counted(pt, 5)
    pt.close()
    assert ran == (0, 1)
    assert_bitwise(got, want[W, Hh, 5], "shaded again")


@pytest.mark.parametrize("W,Hh", SIZES)
def test_row_split_share(cornell_scene, want, W, Hh):
    """Rank 1 of 3: without PT_FLAG_REF_DISPATCH the footprint is the image, so the share's limits
    do not clip and it runs the specialised line."""
    pt = warmed(cornell_scene, W, Hh, rank=1, world=3)
    got, ran = render_counted(pt, 24)
    pt.close()
    assert ran == (0, 1)
    assert_bitwise(got, want[W, Hh, 24][1::3], "rank 1 of 3")


@pytest.mark.parametrize("W,Hh", SIZES)
def test_captured_graph(cornell_scene, want, W, Hh):
    """A progressive graph of 2 x 4 frames is captured with the line the planner says -- the
    specialised one with a learned order, the generic one with key 21 off -- and replays bit-exactly."""
    pt = warmed(cornell_scene, W, Hh)
    for on in (True, False):
        pt.set_common(on)
        before = pt.launches()
        pt.progressive_setup(frames_per_launch=4, launches_per_replay=2)
        after = pt.launches()
        assert (after[0] - before[0], after[1] - before[1]) == ((0, 2) if on else (2, 0))
        pt.progressive_reset(1)
        pt.progressive_run(replays=1)
        assert_bitwise(pt.read_rgba32f(), want[W, Hh, 8], "graph, key 21 %s" % ("on" if on else "off"))
        pt.progressive_reset(1)
        pt.progressive_run(replays=1)
        assert_bitwise(pt.read_rgba32f(), want[W, Hh, 8], "graph replayed again, key 21 %s" % ("on" if on else "off"))
    pt.close()
