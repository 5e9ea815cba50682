"""The GPU BVH builder (pt_bvh_build_gpu) against the host builder, whose
node arrays are themselves pinned to the oracle's literal restatement of buildSAHTree
(tests/test_scene.py): the same node numbering, bounds, leaf indices and links, word for
word, on the reference's shipped scenes, the benchmark stand-ins and edge cases.

The edge cases are those of tests/bvh_cases.py (its docstring has which of the builder's four
order-sensitive rules each one notices, and the hipcub tile sizes they were sized against: 1,024
items per scan-by-key tile and per block sort, so the multi-tile cases span 6 to 21 tiles), the
suite's fuzz scenes, the reference's scenes through the scene handle, the error paths and two
host threads building at once."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

import bvh_cases as B
import fuzz_scenes as F
import pt_host as H
import pt_scenes
from test_bvh_cases import last_error, raw_build_gpu

pytestmark = pytest.mark.gpu


def same(tris, want=None):
    if want is None:
        want = H.buildSAHTree(tris)
    got = H.buildSAHTree(tris, device=0)
    assert got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%d words differ, first at node %s" % (len(bad), bad[:3].tolist())
    return got


@pytest.mark.parametrize("name", ["cornell", "bunny", "sponza"])
def test_benchmark_scenes(name, tmp_path):
    sb = H.setupBuffers(*pt_scenes.write_scene(name, str(tmp_path)))
    got = same(sb["tris"])
    assert np.array_equal(got.view(np.uint32), np.asarray(sb["nodes"], np.float32).view(np.uint32))


def test_shipped_ship_scene(ship_scene):
    same(ship_scene["tris"])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 61, 62, 121, 1000])
def test_sizes_and_duplicates(n):
    rng = np.random.default_rng(n)
    t = np.zeros((n, 16), np.float32)
    t[:, :12] = rng.normal(size=(n, 12)).astype(np.float32)
    t[:, [3, 7, 11]] = 0
    t[:, 12] = rng.integers(0, 4, n)
    if n >= 4:
        t[n // 2] = t[0]                      # duplicate triangle: leaf index = first occurrence
        t[1, :12] = np.round(t[1, :12])       # integer coordinates: centroid ties
        t[2, :12] = np.round(t[2, :12])
    same(t)


def test_ties_signed_zeros_and_degenerate_boxes():
    """Equal centroids everywhere (stable order decides), -0 coordinates, zero-area boxes
    (no finite split cost: the median fallback)."""
    n = 40
    t = np.zeros((n, 16), np.float32)
    t[:, 0:3] = [0.0, 1.0, 2.0]
    t[:, 4:7] = [0.0, 1.0, 2.0]
    t[:, 8:11] = [0.0, 1.0, 2.0]
    t[::3, 0] = -0.0
    t[:, 12] = np.arange(n)
    same(t)
    q = np.zeros((n, 16), np.float32)           # flat quads in z = 0 with -0 / +0 mixed
    rng = np.random.default_rng(5)
    q[:, [0, 1, 4, 5, 8, 9]] = rng.integers(-3, 4, (n, 6)).astype(np.float32)
    q[::2, [2, 6, 10]] = -0.0
    same(q)


@pytest.mark.parametrize("name", list(B.CASES))
def test_edge_cases(name):
    """tests/bvh_cases.py: ties over many scan tiles and sort blocks, unbalanced trees (a window
    that shrinks, one that starts past position 0, levels of one active node), subnormal and
    near-overflow coordinates, sizes around the candidate stride."""
    same(B.get(name))


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_scenes(seed):
    """The suite's fuzz generator (flat quads, duplicates, degenerates, floors, far offsets, four
    decades of size), against the nodes its host build made."""
    sc, _ = F.random_case(seed)
    same(sc["tris"], np.ascontiguousarray(sc["nodes"], np.float32))


@pytest.mark.parametrize("name,robust", [("drift", False), ("p", False), ("p2", False), ("ship", False),
                                         ("ship", True)])
def test_reference_scenes_through_the_scene_handle(name, robust, ref_scenes):
    """OBJ, built-ins, then pt_scene_build_bvh_gpu: the five buffers of the host's setupBuffers."""
    obj, mtl = os.path.join(ref_scenes, name + "obj.txt"), os.path.join(ref_scenes, name + "mtl.txt")
    want = H.setupBuffers(obj, mtl, robust=robust)
    got = H.setupBuffers(obj, mtl, robust=robust, device=0)
    for key in ("tris", "nodes", "mats", "spheres", "cam"):
        a, b = np.asarray(got[key], np.float32), np.asarray(want[key], np.float32)
        assert a.shape == b.shape and a.size > 0, key
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), key
    assert got["n_loaded_mats"] == want["n_loaded_mats"]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_data_is_refused_like_the_host(bad):
    t = B.get("soup120").copy()
    t[77, 5] = bad
    errs = []
    for device in (None, 0):
        with pytest.raises(H.PTError) as e:
            H.buildSAHTree(t, device=device)
        errs.append((e.value.code, str(e.value)))
    assert errs[0] == errs[1] and errs[0][0] == -4 and "non-finite triangle data" in errs[0][1]
    same(B.get("soup120"))                       # the next good build on this thread


def test_node_buffer_errors_and_count_only():
    build = raw_build_gpu()
    tris = B.get("soup59")
    want = H.buildSAHTree(tris)
    nn = C.c_int(0)
    small = np.zeros((len(want) - 1, 12), np.float32)
    assert build(tris.ctypes.data, len(tris), small.ctypes.data, len(small), C.addressof(nn), 0) == -1   # PT_E_ARG
    assert last_error() == "node buffer too small" and nn.value == len(want)
    assert not small.any(), "a too-small buffer is left alone"
    nn = C.c_int(0)
    assert build(tris.ctypes.data, len(tris), None, 0, C.addressof(nn), 0) == 0      # the count only
    assert nn.value == len(want)
    exact = np.zeros((len(want), 12), np.float32)
    assert build(tris.ctypes.data, len(tris), exact.ctypes.data, len(exact), C.addressof(nn), 0) == 0
    assert np.array_equal(exact.view(np.uint32), want.view(np.uint32))
    assert build(tris.ctypes.data, len(tris), exact.ctypes.data, len(exact), C.addressof(nn), 1 << 20) == -5  # PT_E_HIP
    assert "hipSetDevice" in last_error()
    same(tris)


def test_two_host_threads():
    """Two threads build different cases at once, three times each (ctypes releases the GIL; every
    build has its own stream and buffers): the host's nodes every time.  Then a build that fails
    on one thread leaves the other thread's pt_bvh_last_error alone."""
    names = ["plane", "lattice"]
    want = {n: H.buildSAHTree(B.get(n)) for n in names}
    H.buildSAHTree(B.get("soup59"), device=0)               # module load before the threads start
    got, errors = {n: [] for n in names}, []
    start = threading.Barrier(2)

    def work(name):
        try:
            start.wait()
            for _ in range(3):
                got[name].append(H.buildSAHTree(B.get(name), device=0))
        except BaseException as e:      # noqa: BLE001 (reported below, on the main thread)
            errors.append((name, e))

    threads = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for n in names:
        assert len(got[n]) == 3
        for g in got[n]:
            assert g.shape == want[n].shape and np.array_equal(g.view(np.uint32), want[n].view(np.uint32)), n

    build = raw_build_gpu()
    seen, step = {}, [threading.Event(), threading.Event()]
    tris = B.get("soup60")
    nodes = np.zeros((2 * len(tris), 12), np.float32)

    def first():
        nn = C.c_int()
        seen["a_rc"] = build(tris.ctypes.data, (1 << 23) + 1, nodes.ctypes.data, len(nodes), C.addressof(nn), 0)
        step[0].set()
        step[1].wait(60)
        seen["a_msg"] = last_error()

    def second():
        step[0].wait(60)
        bad = tris.copy()
        bad[3, 0] = np.nan
        nn = C.c_int()
        seen["b_rc"] = build(bad.ctypes.data, len(bad), nodes.ctypes.data, len(nodes), C.addressof(nn), 0)
        seen["b_msg"] = last_error()
        step[1].set()

    threads = [threading.Thread(target=first), threading.Thread(target=second)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert seen == dict(a_rc=-4, a_msg="more than 2^23 triangles (float index limit)", b_rc=-4,
                        b_msg="non-finite triangle data")


def test_gpu_builder_is_faster_on_sponza(tmp_path):
    tris, _ = H.load_vertex_data(*pt_scenes.write_scene("sponza", str(tmp_path)))
    H.buildSAHTree(tris[:1000], device=0)                    # warm-up (module load)
    t0 = time.perf_counter()
    H.buildSAHTree(tris)
    cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    H.buildSAHTree(tris, device=0)
    gpu = time.perf_counter() - t0
    print("sponza stand-in (%d tris): host %.3f s, GPU %.3f s" % (len(tris), cpu, gpu))
    assert gpu < cpu


def test_cli_gpu_bvh_same_image(tmp_path):
    """ptrace --gpu-bvh renders the same image as the host-built tree."""
    import subprocess
    from test_gpu_cli import EXE, read_pfm
    obj, mtl = pt_scenes.write_scene("cornell", str(tmp_path))
    outs = []
    for extra in ([], ["--gpu-bvh"]):
        pfm = str(tmp_path / ("x%d.pfm" % len(outs)))
        r = subprocess.run([EXE, obj, mtl, "--width", "48", "--height", "32", "--spp", "3", "--bounces", "8",
                            "--pfm", pfm, "--ppm", str(tmp_path / "x.ppm")] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append(read_pfm(pfm))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
