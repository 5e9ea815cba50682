"""The BVH edge cases of tests/bvh_cases.py against the host builder: every case's stated
preconditions (what makes it reach the path it is named for), and the argument errors of
pt_bvh_build_gpu that return before any device call.  No GPU; the GPU builder runs the same
cases in tests/test_gpu_bvh.py."""
import ctypes as C

import numpy as np
import pytest

import bvh_cases as B
import fuzz_scenes as F
import pt_host as H

F32_MIN_NORMAL = np.float32(1.1754944e-38)
COORDS = [0, 1, 2, 4, 5, 6, 8, 9, 10]
MAX_DEPTH = 3000            # one GPU builder level (and one host sync) per tree level


@pytest.fixture(scope="module")
def host_trees():
    return {name: H.buildSAHTree(B.get(name)) for name in B.CASES}


@pytest.mark.parametrize("name", list(B.CASES))
def test_case_preconditions(name, host_trees):
    tris, nodes = B.get(name), host_trees[name]
    n = len(tris)
    assert tris.shape == (n, 16) and tris.dtype == np.float32
    assert np.isfinite(tris).all()
    assert np.isfinite(nodes[:, [0, 1, 2, 4, 5, 6]]).all(), "node boxes must stay finite"
    assert len(nodes) <= 2 * n - 1
    depth, leaves = B.tree_depth(nodes)
    assert 2 * leaves - 1 == len(nodes)
    assert depth <= MAX_DEPTH
    assert np.array_equal(B.CASES[name](), tris), "the case is deterministic"


@pytest.mark.parametrize("name", B.MULTI_TILE)
def test_multi_tile_cases_span_four_tiles(name):
    assert len(B.get(name)) >= 4 * B.SCAN_TILE


def test_flat_ints_is_deep(host_trees):
    """Triangles that share a box peel off one at a time: thousands of levels, most of them with
    one active node, and a window that shrinks."""
    depth, _ = B.tree_depth(host_trees["flat_ints"])
    assert depth >= 1000
    assert np.any(np.signbit(B.get("flat_ints")[:, 2])) and not np.all(np.signbit(B.get("flat_ints")[:, 2]))


@pytest.mark.parametrize("name", list(B.CHAINS))
def test_chains_are_unbalanced(name, host_trees):
    n = B.CHAINS[name][0]
    depth, _ = B.tree_depth(host_trees[name])
    assert depth >= n / 8, depth


def test_magnitude_cases(host_trees):
    c = B.get("subnormal_1e-41")[:, COORDS]
    assert np.mean((np.abs(c) < F32_MIN_NORMAL) & (c != 0)) >= 0.99
    c = B.get("overflow_3.3e38")[:, COORDS]
    with np.errstate(over="ignore"):
        assert np.isinf(c.max(0) - c.min(0)).all(), "the root's extents overflow"
    # no finite cost anywhere: the median fallback halves every node
    assert B.tree_depth(host_trees["overflow_3.3e38"])[0] == 8
    assert np.abs(B.get("large_1e37")[:, COORDS]).max() > 9e36


def test_fuzz_seeds_leave_no_scene_empty():
    """tests/test_gpu_bvh.py builds the fuzz scenes of seeds 0-39: all nine sizes, none empty."""
    sizes = set()
    for seed in range(40):
        sc, _ = F.random_case(seed)
        assert len(sc["tris"]) > 0 and len(sc["nodes"]) > 0
        sizes.add(len(sc["tris"]))
    assert sizes == set(F.SIZES)


# ------------------------------------------------------------------ argument errors, no device call
def raw_build_gpu():
    """pt_bvh_build_gpu with plain pointer arguments (pt_host's binding refuses None)."""
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int)
    return C.cast(H.lib().pt_bvh_build_gpu, proto)


def last_error():
    return H.lib().pt_bvh_last_error().decode()


def test_gpu_builder_argument_errors():
    build = raw_build_gpu()
    tris = np.zeros((2, 16), np.float32)
    nodes = np.zeros((3, 12), np.float32)
    nn = C.c_int(-7)
    tp, np_, cp = tris.ctypes.data, nodes.ctypes.data, C.addressof(nn)
    for args in ((tp, 0, np_, 3, cp, 0), (None, 2, np_, 3, cp, 0), (tp, 2, np_, 3, None, 0)):
        # the count is checked before the data is read: a small buffer is enough
        assert build(tp, (1 << 23) + 1, np_, 3, cp, 0) == -4         # PT_E_SCENE
        assert last_error() == "more than 2^23 triangles (float index limit)"
        assert build(*args) == -1                                    # PT_E_ARG
        assert last_error() == "empty triangle list"
    assert nn.value == -7, "a refused call writes no count"
    # the host builder documents the same codes and messages
    assert H.lib().pt_bvh_build(tris.reshape(-1), 0, nodes.reshape(-1), 3, C.byref(nn)) == -1
    assert last_error() == "empty triangle list"
