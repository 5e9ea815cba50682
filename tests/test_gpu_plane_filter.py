"""The path pool's plane-window filter (PT_POOL_PLANE_FILTER, csrc/pt_render_pool.h; DESIGN.md §5.12, "Round 20") on
the GPU: k_render_pool clears the candidate bit of the pair a bounce ray leaves where the pair's plane distances are
outside their windows; k_render_sm visits every candidate.  Every case renders with the pool (tuning key 24 = 1) and
with k_render_sm's swept line (key 24 = 0) and compares the two images word for word.  The shapes are the smallest at
which the filter can go wrong; tests/test_plane_window.py holds its CPU model.
"""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import assert_bitwise
from test_gpu_path_pool import BOUNCES, context
from test_leaf_sweep import quad_rows
from test_plane_window import soup

pytestmark = pytest.mark.gpu


def pool_against_sm(sc, label, W, Hh, n_frames, keys=(), want=None, max_bounce=BOUNCES, frame_first=1):
    """The pooled image against k_render_sm's, and both against `want` (the oracle's) where given."""
    pt = context(sc, W, Hh, max_bounce=max_bounce)
    for k, v in keys:
        pt.set_key(k, v)
    img = {}
    for on in (False, True):
        pt.set_pool(on)
        pt.render(frame_first, n_frames, 0)
        assert pt.pooled() == on, (label, on)
        img[on] = pt.read_rgba32f().copy()
    pt.close()
    assert_bitwise(img[True], img[False], "%s: the pool against k_render_sm" % label)
    assert np.isfinite(img[True][..., :3]).all() and float(img[True][..., :3].max()) > 0.0, label
    if want is not None:
        assert_bitwise(img[True], want, "%s: the pool against the oracle" % label)


def test_cornell_against_sm_and_oracle(cornell_scene):
    want = O.render(cornell_scene, 64, 48, max_bounce=BOUNCES, n_frames=4)
    pool_against_sm(cornell_scene, "cornell 64x48, 4 frames", 64, 48, 4, want=want)


def test_soup_with_non_coplanar_pairs():
    """24 leaves, ten of them non-coplanar pairs: the own pair's second triangle may be in window, and its bit stays."""
    pool_against_sm(soup(), "24-leaf soup", 32, 24, 4)


def test_single_triangle_leaf():
    pool_against_sm(quad_rows(5, drop_last=True), "a single-triangle leaf", 32, 24, 4)


def test_one_frame_launch(cornell_scene):
    pool_against_sm(cornell_scene, "cornell 32x24, 1 frame", 32, 24, 1)


def test_frames_in_more_than_one_group(cornell_scene):
    """10 frames at 4 per work item (key 5): three groups, the last one short."""
    pool_against_sm(cornell_scene, "cornell 16x16, 10 frames in groups of 4", 16, 16, 10, keys=((5, 4),))
