"""The signed leaf sweep of k_render_pool (ptc::sweep_mask_signed_piped on the workgroup's signed table, which also
serves the exact leaf re-test; DESIGN.md §5.12, "Round 17") on the GPU.  Every case renders the oracle's words with the
pool on and with it off (k_render_sm's swept line on the scalar table), as tests/test_gpu_path_pool.py does, at 32x24
for 4 frames; tests/test_sweep_signed.py holds the CPU side.
"""
import pytest

from test_gpu_path_pool import FUZZ_POOLED, both, fuzz_case
from test_leaf_sweep import quad_rows, scene_with_leaves
from test_window_cull import moved

pytestmark = pytest.mark.gpu

FAR_SOUP = (34, 12, False)      # (seed, triangles, cut spheres) of FUZZ_POOLED


@pytest.mark.parametrize("leaves", [2, 3, 4, 5, 24])
def test_signed_table_sizes(leaves):
    """At two boxes per chunk: one chunk, the remainder and one chunk, two chunks, the remainder and two chunks, and the
    full mask (trips of the unrolled loop; 3 and 5 leave a remainder)."""
    both(scene_with_leaves(leaves), "%d leaves" % leaves, 32, 24)


def test_cornell_eight_bounces(cornell_scene):
    both(cornell_scene, "cornell, 8 bounces", 32, 24, max_bounce=8)


def test_small_and_large_addends(cornell_scene):
    """Bounds and addends four orders below and three above Cornell's: the box scaled by 1e-4, and the soup of
    test_gpu_path_pool.py's pooled ones that its seed moves farthest from the origin (coordinates up to 2235)."""
    both(moved(cornell_scene, scale=1e-4), "cornell scaled by 1e-4", 32, 24)
    seed, n_tris, cut = FAR_SOUP
    assert FAR_SOUP in FUZZ_POOLED
    sc, kw = fuzz_case(seed, n_tris, cut)
    both(sc, "fuzz seed %d (%d triangles), far from the origin" % (seed, n_tris), 32, 24, frame_first=kw["frame_first"],
         max_bounce=kw["max_bounce"])


def test_waves_that_skip_the_sweep():
    """The camera stands outside the root box: whole waves skip the sweep on the root's own test, which keeps the
    split reciprocal."""
    both(quad_rows(11), "11 quads seen from outside their box", 32, 24)
