"""The adaptive tile order (k_tile_order) on the GPU.  The sort writes the
permutation every later launch reads its tiles from: a dropped or repeated tile is a wrong image.
pt_debug_tile_order (PathTracer.tile_order) shows whether a sort ran and what it wrote; each test
checks that the permutation holds every tile of the grid exactly once -- the grid worked out here
from the image width, the rank's local rows and the tile shape -- and that launches reading the
learned order still give the oracle's image, bit for bit."""
import numpy as np
import pytest

import oracle_lib as O
import pt_host as H
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu

W, HH, BOUNCES = 100, 44, 6           # partial tiles on both edges for every tile shape


@pytest.fixture(scope="module")
def want(cornell_scene):
    """The oracle's accumulated image after n frames, computed once per n."""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = O.render(cornell_scene, W, HH, max_bounce=BOUNCES, n_frames=n)
            cache[n].setflags(write=False)
        return cache[n]
    return get


def grid(width, rows_local, key20):
    """The (ty, tx) of every tile: 64 pixels as (8 << s) columns x (8 >> s) local rows."""
    s = key20 - 1 if key20 else 0
    tw, th = 8 << s, 8 >> s
    tiles_x, tiles_y = -(-width // tw), -(-rows_local // th)
    return tiles_x, [(ty, tx) for ty in range(tiles_y) for tx in range(tiles_x)]


def check_order(pt, key20, sorts=None):
    to = pt.tile_order()
    tiles_x, tiles = grid(pt.width, pt.rows_local, key20)
    assert (to["tiles_x"], to["n_tiles"], len(to["perm"])) == (tiles_x, len(tiles), len(tiles))
    got = sorted(map(tuple, to["perm"].tolist()))
    assert got == tiles, "the order is not a permutation of the grid: %d distinct of %d" % (len(set(got)), len(tiles))
    if sorts is not None:
        assert to["sorts"] == sorts
    return to


def one_frame_launches(pt, first, count):
    for f in range(first, first + count):
        pt.render_async(f, 1, 0 if f == 1 else 1)


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("key20", [0, 1, 2, 3, 4])
def test_learned_order_every_shape_and_rank(cornell_scene, want, key20, world):
    """Eight one-frame launches after an upload learn an order (one sort); the next three read it."""
    for rank in range(world):
        pt = H.PathTracer(W, HH, max_bounce=BOUNCES, rank=rank, world=world)
        pt.set_key(20, key20)
        pt.upload(cornell_scene)
        check_order(pt, key20, sorts=0)
        one_frame_launches(pt, 1, 7)
        check_order(pt, key20, sorts=0)
        one_frame_launches(pt, 8, 1)
        to = check_order(pt, key20, sorts=1)
        # the box's tiles cost several segments a pixel, the sky's one: a sort by cost cannot
        # leave the raster order in place
        assert to["perm"].tolist() != [list(t) for t in grid(W, pt.rows_local, key20)[1]]
        one_frame_launches(pt, 9, 3)
        got = pt.read_rgba32f()
        check_order(pt, key20, sorts=1)
        pt.close()
        assert_bitwise(got, want(11)[rank::world], "key 20 = %d, world %d rank %d" % (key20, world, rank))


@pytest.mark.parametrize("key20", [0, 1, 2, 3, 4])
def test_cold_probe(cornell_scene, want, key20):
    """A long first render sorts after its two probe frames, so the rest reads a learned order."""
    pt = H.PathTracer(W, HH, max_bounce=BOUNCES)
    pt.upload(cornell_scene)
    pt.set_key(20, key20)
    pt.render(1, 66, 0)
    to = check_order(pt, key20)
    got = pt.read_rgba32f()
    pt.close()
    assert to["sorts"] >= 1
    assert_bitwise(got, want(66), "cold probe, key 20 = %d" % key20)


def test_more_tiles_than_sort_threads(cornell_scene):
    """264 x 264 is 1,089 8x8 tiles: the sort's 1,024 threads take their strided second turn."""
    n = 264
    ref = O.render(cornell_scene, n, n, max_bounce=1, n_frames=9)
    pt = H.PathTracer(n, n, max_bounce=1)
    pt.upload(cornell_scene)
    one_frame_launches(pt, 1, 8)
    to = check_order(pt, 0, sorts=1)
    assert to["n_tiles"] == 1089
    one_frame_launches(pt, 9, 1)
    got = pt.read_rgba32f()
    pt.close()
    assert_bitwise(got, ref, "1,089 tiles")


def test_edges(cornell_scene):
    """One tile, or the adaptive order switched off: no sort ever runs and the order stays the
    raster order.  Exactly two tiles: the sort runs."""
    for width, adaptive, sorts in ((8, 1, 0), (16, 0, 0), (16, 1, 1)):
        ref = O.render(cornell_scene, width, 8, max_bounce=BOUNCES, n_frames=10)
        pt = H.PathTracer(width, 8, max_bounce=BOUNCES)
        pt.set_tuning(adaptive=adaptive)
        pt.upload(cornell_scene)
        one_frame_launches(pt, 1, 9)
        to = check_order(pt, 0, sorts=sorts)
        assert to["n_tiles"] == width // 8
        if not sorts:
            assert to["perm"].tolist() == [[0, tx] for tx in range(width // 8)]
        one_frame_launches(pt, 10, 1)
        got = pt.read_rgba32f()
        pt.close()
        assert_bitwise(got, ref, "width %d adaptive %d" % (width, adaptive))


def test_graph_sorts_once_per_replay(cornell_scene, want):
    pt = H.PathTracer(W, HH, max_bounce=BOUNCES)
    pt.upload(cornell_scene)
    pt.progressive_setup(frames_per_launch=2, launches_per_replay=1)
    check_order(pt, 0, sorts=0)                   # the capture itself runs nothing
    pt.progressive_run(replays=1)
    check_order(pt, 0, sorts=1)
    pt.progressive_run(replays=2)
    check_order(pt, 0, sorts=3)
    got = pt.read_rgba32f()
    pt.upload(cornell_scene)                      # the count restarts with the scene
    check_order(pt, 0, sorts=0)
    pt.close()
    assert_bitwise(got, want(6), "three replays of two frames")
