"""The ray query on the GPU (pt_api.h: pt_intersect, pt_intersect_device, pt_pick; ptrace --pick, --rays / --hits;
DESIGN.md §12) against the host twin (pt_intersect_host, itself checked against the numpy model of the reference in
tests/test_query_host.py), word for word: every comparison is of uint32 words, with no tolerance.  The scenes and ray
families are tests/query_cases.py's; they cover the three storage classes of the walk -- the whole tree in the staged
top (Cornell, 35 nodes), trees straddling the 768 staged records (767 / 769 nodes) and a tree mostly in global memory
(2,500 triangles)."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import pt_host as H
import pt_scenes
import query_cases as QC
from test_gpu_cli import EXE

pytestmark = pytest.mark.gpu

f32 = np.float32
W, HH = 64, 48


def words(h):
    return H.hits_words(h)


def same(got, want, what):
    bad = np.nonzero(np.any(words(got) != words(want), axis=1))[0]
    assert bad.size == 0, "%s: %d of %d hit records differ, first at ray %d: got %s, want %s" % (
        what, bad.size, len(want), bad[0], got[bad[0]], want[bad[0]])


def tracer(sc, **kw):
    pt = H.PathTracer(W, HH, max_bounce=8, **kw)
    pt.upload(sc)
    return pt


def batch(sc, scale=1.0):
    return QC.ray_batch(sc, 7, lambda r: H.intersect_host(sc, r), scale)[0]


def device_cast(pt, rays, any_hit=False, wait=True):
    """pt_intersect_device on device arrays of the HIP runtime the library links (its symbols resolve through the
    library's handle): the blocking copies order themselves, the query is enqueued on the context's stream and the
    context is synchronised before the read.  wait=False: returns a function that reads the hits, to call after
    the caller's own pt.sync()."""
    L = H.lib()
    for fn, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipFree", [C.c_void_p]),
                     ("hipMemcpy", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int])):
        getattr(L, fn).restype, getattr(L, fn).argtypes = C.c_int, args
    rays = np.ascontiguousarray(rays)
    hits = np.zeros(len(rays), H.HIT_DTYPE)
    d_rays, d_hits = C.c_void_p(), C.c_void_p()
    assert L.hipMalloc(C.byref(d_rays), max(rays.nbytes, 16)) == 0 and L.hipMalloc(C.byref(d_hits), max(hits.nbytes, 16)) == 0
    assert L.hipMemcpy(d_rays, rays.ctypes.data, rays.nbytes, 1) == 0              # hipMemcpyHostToDevice
    pt.intersect_device(d_rays.value, len(rays), d_hits.value, any_hit)

    def read():
        rc = L.hipMemcpy(hits.ctypes.data, d_hits, hits.nbytes, 2)                 # hipMemcpyDeviceToHost
        L.hipFree(d_rays)
        L.hipFree(d_hits)
        assert rc == 0
        return hits
    if not wait:
        return read
    pt.sync()
    return read()


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", QC.NAMES)
def test_parity(name, cornell_scene, ship_scene):
    sc = QC.scene(name, cornell_scene, ship_scene)
    rays = batch(sc)
    pt = tracer(sc)
    for any_hit in (False, True):
        want = H.intersect_host(sc, rays, any_hit)
        same(pt.intersect(rays, any_hit), want, "%s pt_intersect any %d" % (name, any_hit))
        same(device_cast(pt, rays, any_hit), want, "%s pt_intersect_device any %d" % (name, any_hit))
    pt.close()


@pytest.mark.parametrize("flags", [H.PT_FLAG_NO_SPHERES, H.PT_FLAG_NO_TRIANGLES, H.PT_FLAG_MOLLER_TRUMBORE])
@pytest.mark.parametrize("name", ["cornell", "top769"])
def test_context_flags(name, flags, cornell_scene, ship_scene):
    sc = QC.scene(name, cornell_scene, ship_scene)
    rays = batch(sc)
    pt = tracer(sc, flags=flags)
    for any_hit in (False, True):
        same(pt.intersect(rays, any_hit), H.intersect_host(sc, rays, any_hit, flags), "%s flags %d" % (name, flags))
    pt.close()


# 256 threads x the 2,048-workgroup cap = 524,288: the last count runs the stride loop with a ragged tail
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1 << 16, 256 * 2048 + 77])
def test_ray_counts(n, cornell_scene):
    rays = np.resize(batch(cornell_scene), n)
    pt = tracer(cornell_scene)
    got = pt.intersect(rays)
    assert len(got) == n
    same(got, H.intersect_host(cornell_scene, rays), "%d rays" % n)
    if n in (65, 1 << 16):
        same(device_cast(pt, rays, True), H.intersect_host(cornell_scene, rays, True), "%d rays, device, any-hit" % n)
    pt.close()


@pytest.mark.parametrize("name", ["cornell", "top767", "top769", "fuzz2500"])
def test_kernel_variants_agree(name, cornell_scene, ship_scene):
    """Variant 3 keeps the scene in global memory: the unstaged walk."""
    sc = QC.scene(name, cornell_scene, ship_scene)
    rays = batch(sc, 0.5)
    pt = tracer(sc)
    want = H.intersect_host(sc, rays)
    for variant in (0, 3, 0):
        pt.set_kernel(variant)
        same(pt.intersect(rays), want, "%s variant %d" % (name, variant))
    pt.close()


def test_pick(cornell_scene):
    pt = tracer(cornell_scene)
    ys, xs = np.meshgrid(np.arange(HH), np.arange(W), indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], 1)[::7]
    rays = H.pixel_rays(W, HH, cornell_scene["cam"], xy)
    got = pt.pick(xy)
    same(got, pt.intersect(rays), "pt_pick")
    same(got, H.intersect_host(cornell_scene, rays), "pt_pick against the host")
    assert len(set(got["kind"])) == 3
    cam = np.array(cornell_scene["cam"], f32)
    cam[0:3], cam[4:7] = [0.5, -5, 1.5], [0.1, 1, -0.1]
    pt.set_camera(cam)                                   # the context's camera, not the scene's
    same(pt.pick(xy), H.intersect_host(cornell_scene, H.pixel_rays(W, HH, cam, xy)), "pt_pick after pt_set_camera")
    pt.close()


def test_row_split(cornell_scene):
    rays = batch(cornell_scene, 0.5)
    want = H.intersect_host(cornell_scene, rays)
    xy = np.array([[3, 5], [32, 24], [60, 40], [10, 47]], np.int32)
    picks = H.intersect_host(cornell_scene, H.pixel_rays(W, HH, cornell_scene["cam"], xy))
    for rank in range(3):
        pt = tracer(cornell_scene, rank=rank, world=3)
        same(pt.intersect(rays), want, "rank %d of 3" % rank)
        same(pt.pick(xy), picks, "pick on rank %d of 3" % rank)     # image rows, whoever renders them
        pt.close()


# ---------------------------------------------------------------- errors
def test_errors(cornell_scene):
    pt = H.PathTracer(W, HH)
    rays = H.make_rays([[0, -6, 1]], [[0, 1, 0]])
    hits = np.zeros(1, H.HIT_DTYPE)
    xy = np.zeros((1, 2), np.int32)
    L = H.lib()
    with pytest.raises(H.PTError) as e:
        pt.intersect(rays)
    assert e.value.code == -6                                              # PT_E_STATE: before an upload
    assert L.pt_intersect_device(pt.h, None, 0, None, 0) == -6
    assert L.pt_pick(pt.h, xy.ctypes.data, 1, hits.ctypes.data) == -6
    pt.upload(cornell_scene)
    assert L.pt_pick(pt.h, xy.ctypes.data, 1, hits.ctypes.data) == 0
    assert L.pt_intersect(None, rays.ctypes.data, 1, hits.ctypes.data, 0) == -1
    assert L.pt_intersect(pt.h, None, 1, hits.ctypes.data, 0) == -1        # PT_E_ARG: null with n > 0
    assert L.pt_intersect(pt.h, rays.ctypes.data, 1, None, 0) == -1
    assert L.pt_intersect(pt.h, rays.ctypes.data, 1, hits.ctypes.data, 2) == -1    # unknown query flag
    assert L.pt_intersect(pt.h, rays.ctypes.data, -1, hits.ctypes.data, 0) == -1
    assert L.pt_intersect_device(pt.h, None, 1, None, 0) == -1
    assert L.pt_intersect_device(pt.h, 8, 1, 16, 0) == -1                   # misaligned device arrays, before any launch
    assert L.pt_pick(pt.h, None, 1, hits.ctypes.data) == -1
    assert L.pt_intersect(pt.h, None, 0, None, 0) == 0                     # n = 0: PT_OK without a launch
    assert L.pt_intersect_device(pt.h, None, 0, None, PT_ANY) == 0
    assert L.pt_pick(pt.h, None, 0, None) == 0
    pt.close()


PT_ANY = H.PT_QUERY_ANY_HIT


# ---------------------------------------------------------------- invisibility
def test_query_is_invisible(cornell_scene):
    """Two tracers, one render sequence -- a long launch, short overlapped launches, a progressive replay -- and one
    of them queries between the steps (tests/test_gpu_denoise.py's pattern).  64 x 48: one wave of the tile sort."""
    plain, qry = tracer(cornell_scene), tracer(cornell_scene)
    for pt in (plain, qry):
        pt.set_moments(True)
    rays = batch(cornell_scene, 0.3)
    want = H.intersect_host(cornell_scene, rays)

    def state(pt):
        mom, n = pt.read_moments()
        to = pt.tile_order()
        return dict(image=pt.read_rgba32f(), moments=mom, frames=n, sorts=to["sorts"], perm=to["perm"],
                    grid=(to["n_tiles"], to["tiles_x"]), launches=pt.launches(), sweep=pt.leaf_sweep(),
                    pooled=pt.pooled(), n_timed=pt.timing()[1], rgba8=pt.read_rgba8())

    def check(step):
        a, b = state(plain), state(qry)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (step, k)
            else:
                assert a[k] == b[k], (step, k, a[k], b[k])

    def query():
        same(qry.intersect(rays), want, "a query between renders")
        qry.pick(np.array([[5, 5], [40, 30]], np.int32))

    for pt in (plain, qry):
        pt.render(1, 40, 0)
    query()
    check("a long launch")
    for pt in (plain, qry):
        for f in range(41, 49):
            pt.render_async(f, 1, 1)
            if pt is qry and f == 44:
                read = device_cast(pt, rays, True, wait=False)  # between launches in flight
        pt.sync()
    same(read(), H.intersect_host(cornell_scene, rays, True), "a device query between launches in flight")
    query()
    check("short overlapped launches")
    for pt in (plain, qry):
        pt.progressive_setup(2, 2)
    query()                                                    # the captured graph stays
    for pt in (plain, qry):
        pt.progressive_run(1)
    query()
    for pt in (plain, qry):
        pt.progressive_run(1)
    check("a progressive replay")
    for pt in (plain, qry):
        pt.render(9, 20, 1)
    query()
    check("a later render")
    plain.close()
    qry.close()


# ---------------------------------------------------------------- the command line
def test_cli_pick_and_rays(tmp_path):
    obj, mtl = pt_scenes.write_scene("cornell", str(tmp_path))
    sc = H.setupBuffers(obj, mtl)
    picks = [(5, 5), (32, 24), (40, 30), (63, 47), (20, 10)]
    rays = batch(sc, 0.3)
    rpath, hpath = str(tmp_path / "rays.bin"), str(tmp_path / "hits.bin")
    rays.tofile(rpath)
    args = [EXE, obj, mtl, "--width", str(W), "--height", str(HH)]
    for x, y in picks:
        args += ["--pick", "%d,%d" % (x, y)]
    pt = tracer(sc)
    want = pt.pick(np.array(picks, np.int32))
    want_any = pt.intersect(rays, True)
    pt.close()
    for extra in ([], ["--spp", "2", "--bounces", "3", "--pfm", str(tmp_path / "o.pfm"), "--ppm", str(tmp_path / "o.ppm")]):
        out = subprocess.run(args + ["--rays", rpath, "--hits", hpath, "--any-hit"] + extra, capture_output=True,
                             text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith('{"pick"')]
        assert len(lines) == len(picks)
        for ln, (x, y), h in zip(lines, picks, want):
            assert ln["pick"] == [x, y] and (ln["kind"], ln["prim"], ln["mat"]) == (h["kind"], h["prim"], h["mat"])
            if h["kind"] == 0:
                assert ln["t"] is None and ln["albedo"] is None
            else:
                assert f32(ln["t"]) == h["t"]            # %.9g round-trips a binary32
                assert np.array_equal(np.array(ln["albedo"], f32), np.asarray(sc["mats"], f32).reshape(-1, 16)[h["mat"], 0:3])
            assert np.array_equal(np.array(ln["n"], f32), h["n"][0:3]) and np.array_equal(np.array(ln["p"], f32), h["p"][0:3])
        same(np.fromfile(hpath, H.HIT_DTYPE), want_any, "--rays / --hits --any-hit")
        assert (tmp_path / "o.pfm").exists() == bool(extra)      # alone: nothing rendered, no image written
