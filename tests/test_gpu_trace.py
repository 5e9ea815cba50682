"""Traced rays on the GPU (pt_api.h: pt_trace, pt_trace_device; ptrace --radiance, --pick with --spp)
against the host twin (pt_trace_host, itself checked against the oracle's renders in tests/test_trace_host.py), and
directly against the oracle and the context's own render, word for word: every comparison is of uint32 words, with no
tolerance (between device and host a NaN must meet a NaN, but not the same one: trace_cases.same_device).  The scenes
are tests/query_cases.py's three storage classes of the walk (the whole tree in the staged top, trees straddling the
768 staged records, a tree mostly in global memory) and a scene without nodes; the ray families are
tests/trace_cases.py's.  The kernel's refill paths are reached with a thousand rays by capping its grid through
pt__trace_debug."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import oracle_lib
import pt_host as H
import pt_scenes
import query_cases as QC
import trace_cases as TC
from test_gpu_cli import EXE

pytestmark = pytest.mark.gpu

f32 = np.float32
W, HH = 64, 48
STAGING, REFILL, GRID_CAP = 0, 1, 2            # ptt::Debug (csrc/pt_trace_launch.h)
_host = {}


def tracer(sc, max_bounce=8, **kw):
    pt = H.PathTracer(W, HH, max_bounce=max_bounce, **kw)
    pt.upload(sc)
    return pt


def host(name, sc, rays, seeds, **kw):
    """pt_trace_host, computed once per (scene, settings) and shared among the tests."""
    key = (name, len(rays), tuple(sorted((k, v if np.isscalar(v) else id(v)) for k, v in kw.items())))
    if key not in _host:
        kw.setdefault("max_bounce", 8)
        _host[key] = H.trace_host(sc, rays, seeds, **kw)
        _host[key].setflags(write=False)
    return _host[key]


def debug(what, value):
    assert H.lib().pt__trace_debug(what, value) == 0


@pytest.fixture(autouse=True)
def default_debug_settings():
    yield
    for what in (STAGING, REFILL, GRID_CAP):
        debug(what, 0)


def device_trace(pt, rays, seeds, frame_first=1, n_frames=1, prior=None, wait=True):
    """pt_trace_device on device arrays of the HIP runtime the library links: the blocking copies order themselves, the
    trace is enqueued on the context's stream and the context is synchronised before the read.  wait=False: returns
    a function that reads the result, to call after the caller's own pt.sync()."""
    L = H.lib()
    for fn, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipFree", [C.c_void_p]),
                     ("hipMemcpy", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int])):
        getattr(L, fn).restype, getattr(L, fn).argtypes = C.c_int, args
    rays = np.ascontiguousarray(rays)
    out = np.full((len(rays), 4), np.nan, f32) if prior is None else np.array(prior, f32)
    d_rays, d_seeds, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.hipMalloc(C.byref(d_rays), max(rays.nbytes, 16)) == 0 and L.hipMalloc(C.byref(d_out), max(out.nbytes, 16)) == 0
    assert L.hipMemcpy(d_rays, rays.ctypes.data, rays.nbytes, 1) == 0              # hipMemcpyHostToDevice
    assert L.hipMemcpy(d_out, out.ctypes.data, out.nbytes, 1) == 0                 # the prior, or NaNs never read
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, np.uint32)
        assert L.hipMalloc(C.byref(d_seeds), max(seeds.nbytes, 16)) == 0
        assert L.hipMemcpy(d_seeds, seeds.ctypes.data, seeds.nbytes, 1) == 0
    pt.trace_device(d_rays.value, d_seeds.value, len(rays), d_out.value, frame_first, n_frames, int(prior is not None))

    def read():
        rc = L.hipMemcpy(out.ctypes.data, d_out, out.nbytes, 2)                    # hipMemcpyDeviceToHost
        for p in (d_rays, d_seeds, d_out):
            if p.value:
                L.hipFree(p)
        assert rc == 0
        return out
    if not wait:
        return read
    pt.sync()
    return read()


# ---------------------------------------------------------------- parity with the host twin
@pytest.mark.parametrize("name", ["cornell", "top767", "top769", "fuzz24", "fuzz2500", "spheres_only"])
def test_parity(name, cornell_scene, ship_scene):
    sc = QC.scene(name, cornell_scene, ship_scene)
    rays, seeds = TC.ray_batch(sc, 17)
    assert 1500 < len(rays) < 3000
    prior = np.random.default_rng(3).random((len(rays), 4)).astype(f32)
    pt = tracer(sc)
    for first, n, pr in ((1, 1, None), (1, 3, None), (5, 2, prior)):
        want = host(name, sc, rays, seeds, frame_first=first, n_frames=n, prior=pr)
        what = "%s frames %d..%d" % (name, first, first + n - 1)
        TC.same_device(pt.trace(rays, seeds, first, n, pr), want, what + " pt_trace")
        TC.same_device(device_trace(pt, rays, seeds, first, n, pr), want, what + " pt_trace_device")
    # the batch is not vacuous: hits and misses, paths of several segments (frames differ), NaN rays
    h = H.intersect_host(sc, rays)
    assert 0.2 < np.mean(h["kind"] > 0) < 0.98
    one, three = host(name, sc, rays, seeds, frame_first=1, n_frames=1, prior=None), host(
        name, sc, rays, seeds, frame_first=1, n_frames=3, prior=None)
    assert np.mean(np.any(TC.words(one) != TC.words(three), axis=1)) > 0.1
    assert 0 < np.mean(np.isnan(three).any(axis=1)) < 0.02      # TC.same_device compares no more than these loosely
    pt.close()


def test_default_seeds(cornell_scene):
    rays, _ = TC.ray_batch(cornell_scene, 17, 0.2)
    pt = tracer(cornell_scene)
    want = H.trace_host(cornell_scene, rays, None, n_frames=2, max_bounce=8)
    TC.same_device(pt.trace(rays, None, 1, 2), want, "seeds = NULL, pt_trace")
    TC.same_device(device_trace(pt, rays, None, 1, 2), want, "seeds = NULL, pt_trace_device")
    pt.close()


# ---------------------------------------------------------------- against the oracle and the render
def test_equals_oracle_and_render(cornell_scene):
    w, h = 16, 12
    pt = H.PathTracer(w, h, max_bounce=8, flags=H.PT_FLAG_NO_AA)
    pt.upload(cornell_scene)
    xy = TC.image_xy(w, h)
    got = pt.trace(H.pixel_rays(w, h, cornell_scene["cam"], xy), H.pixel_seeds(xy), 1, 3)
    TC.same(got, oracle_lib.render(cornell_scene, w, h, max_bounce=8, n_frames=3, flags=H.PT_FLAG_NO_AA), "the oracle")
    pt.render(1, 3, 0)
    TC.same(got, pt.read_rgba32f(), "the same context's render")
    pt.close()


# ---------------------------------------------------------------- refill
@pytest.mark.parametrize("name", ["cornell", "top769"])
def test_refill(name, cornell_scene):
    """n = 1000 rays in 1 and in 3 workgroups: every wave refills across several 64-ray blocks (16 blocks over 4 or
    12 waves), the last block is the ragged tail (1000 = 15 * 64 + 40), and with 12 waves some own one block and some
    two."""
    sc = QC.scene(name, cornell_scene)
    rays, seeds = TC.ray_batch(sc, 19)
    rays, seeds = rays[:1000], seeds[:1000]
    assert len(rays) == 1000
    want = host(name + "/refill", sc, rays, seeds, n_frames=3)
    pt = tracer(sc)
    for cap in (1, 3):
        debug(GRID_CAP, cap)
        for variant in (0, 3, 0):                       # the render's kernel variants: a trace answers alike under each
            pt.set_kernel(variant)
            for refill in (1, 2):
                debug(REFILL, refill)
                TC.same_device(pt.trace(rays, seeds, 1, 3), want, "%s cap %d variant %d refill %d" % (name, cap, variant, refill))
        debug(REFILL, 1)
        for staging in (1, 2):
            debug(STAGING, staging)
            TC.same_device(pt.trace(rays, seeds, 1, 3), want, "%s cap %d staging %d" % (name, cap, staging))
        debug(STAGING, 0)
        debug(REFILL, 0)
    pt.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_ray_counts(n, cornell_scene):
    rays, seeds = TC.ray_batch(cornell_scene, 17, 0.2)
    rays, seeds = np.resize(rays, n), np.resize(seeds, n)
    pt = tracer(cornell_scene)
    want = H.trace_host(cornell_scene, rays, seeds, n_frames=2, max_bounce=8)
    for refill in (1, 2):
        debug(REFILL, refill)
        got = pt.trace(rays, seeds, 1, 2)
        assert got.shape == (n, 4)
        TC.same_device(got, want, "%d rays, refill %d" % (n, refill))
    pt.close()


# ---------------------------------------------------------------- settings
@pytest.mark.parametrize("max_bounce", [0, 1, 8])
def test_max_bounce(max_bounce, cornell_scene):
    rays, seeds = TC.ray_batch(cornell_scene, 17, 0.3)
    pt = tracer(cornell_scene, max_bounce=max_bounce)
    TC.same_device(pt.trace(rays, seeds, 1, 2), H.trace_host(cornell_scene, rays, seeds, n_frames=2, max_bounce=max_bounce),
            "max_bounce %d" % max_bounce)
    pt.close()


def test_display_modes(cornell_scene):
    rays, seeds = TC.ray_batch(cornell_scene, 17, 0.3)
    pt = tracer(cornell_scene)
    seen = []
    for mode in (2, 3, 4, 1):
        pt.set_display_mode(mode)
        got = pt.trace(rays, seeds, 1, 2)
        TC.same_device(got, H.trace_host(cornell_scene, rays, seeds, n_frames=2, max_bounce=8, mode=mode), "mode %d" % mode)
        seen.append(TC.words(got).tobytes())
    assert len(set(seen)) == 4
    pt.close()


@pytest.mark.parametrize("flags", [H.PT_FLAG_NO_AA, H.PT_FLAG_NO_SKY, H.PT_FLAG_NO_SPHERES, H.PT_FLAG_NO_TRIANGLES,
                                   H.PT_FLAG_REF_DISPATCH, H.PT_FLAG_MOLLER_TRUMBORE])
def test_context_flags(flags, cornell_scene):
    rays, seeds = TC.ray_batch(cornell_scene, 17, 0.3)
    pt = tracer(cornell_scene, flags=flags)
    got = pt.trace(rays, seeds, 1, 2)
    TC.same_device(got, H.trace_host(cornell_scene, rays, seeds, n_frames=2, max_bounce=8, flags=flags), "flags %d" % flags)
    if flags in (H.PT_FLAG_NO_AA, H.PT_FLAG_REF_DISPATCH):       # they mean nothing to a trace
        TC.same_device(got, H.trace_host(cornell_scene, rays, seeds, n_frames=2, max_bounce=8), "flags %d ignored" % flags)
    pt.close()


def test_row_split(cornell_scene):
    rays, seeds = TC.ray_batch(cornell_scene, 17, 0.3)
    want = H.trace_host(cornell_scene, rays, seeds, n_frames=2, max_bounce=8)
    for rank in range(3):
        pt = tracer(cornell_scene, rank=rank, world=3)
        TC.same_device(pt.trace(rays, seeds, 1, 2), want, "rank %d of 3" % rank)
        pt.close()


# ---------------------------------------------------------------- errors and ordering
def test_errors(cornell_scene):
    pt = H.PathTracer(W, HH)
    rays = H.make_rays([[0, -6, 1]], [[0, 1, 0]])
    out = np.zeros((1, 4), f32)
    L = H.lib()
    r, o = rays.ctypes.data, out.ctypes.data
    with pytest.raises(H.PTError) as e:
        pt.trace(rays)
    assert e.value.code == -6                                              # PT_E_STATE: before an upload
    assert L.pt_trace_device(pt.h, None, None, 0, 1, 1, 0, None) == -6
    pt.upload(cornell_scene)
    assert L.pt_trace(None, r, None, 1, 1, 1, 0, o) == -1
    assert L.pt_trace(pt.h, None, None, 1, 1, 1, 0, o) == -1               # PT_E_ARG: null with n > 0
    assert L.pt_trace(pt.h, r, None, 1, 1, 1, 0, None) == -1
    assert L.pt_trace(pt.h, r, None, -1, 1, 1, 0, o) == -1
    assert L.pt_trace(pt.h, r, None, 1, 0, 1, 0, o) == -1                  # frame_first < 1
    assert L.pt_trace(pt.h, r, None, 1, 1, 0, 0, o) == -1                  # n_frames < 1
    assert L.pt_trace(pt.h, r, None, 1, 2 ** 31 - 1, 1, 0, o) == -1        # frame_first + n_frames overflows int
    assert L.pt_trace(pt.h, r, None, 1, 1, 1, 2, o) == -1                  # accumulate_first not 0 or 1
    assert L.pt_trace_device(pt.h, None, None, 1, 1, 1, 0, None) == -1
    assert L.pt_trace_device(pt.h, 8, None, 1, 1, 1, 0, 16) == -1          # misaligned device arrays, before any launch
    assert L.pt_trace_device(pt.h, 16, None, 1, 1, 1, 0, 24) == -1
    assert L.pt_trace_device(pt.h, 16, 2, 1, 1, 1, 0, 32) == -1            # seeds not 4-byte aligned
    assert L.pt_trace_device(pt.h, 16, None, 1, 0, 1, 0, 32) == -1
    assert L.pt_trace(pt.h, None, None, 0, 1, 1, 0, None) == 0             # n = 0: PT_OK without a launch
    assert L.pt_trace_device(pt.h, None, None, 0, 1, 1, 1, None) == 0
    assert L.pt__trace_debug(3, 0) == -1 and L.pt__trace_debug(REFILL, 3) == -1 and L.pt__trace_debug(GRID_CAP, -1) == -1
    assert L.pt_trace(pt.h, r, None, 1, 1, 1, 0, o) == 0 and out[0, 3] == 1.0
    pt.close()


def test_stream_order(cornell_scene):
    """A device trace enqueued behind an unsynchronised render sees that render's scene, and an upload after it waits
    for it: the trace's result is the first scene's."""
    other = QC.scene("fuzz24")
    rays, seeds = TC.ray_batch(cornell_scene, 17, 0.5)
    pt = tracer(cornell_scene)
    pt.render_async(1, 8, 0)
    read = device_trace(pt, rays, seeds, 1, 3, wait=False)
    pt.upload(other)                                     # waits for the stream: the trace has read the old buffers
    TC.same_device(read(), H.trace_host(cornell_scene, rays, seeds, n_frames=3, max_bounce=8), "a trace behind a render")
    TC.same_device(pt.trace(rays, seeds, 1, 3), H.trace_host(other, rays, seeds, n_frames=3, max_bounce=8), "after the upload")
    pt.close()


# ---------------------------------------------------------------- invisibility
def test_trace_is_invisible(cornell_scene):
    """Two tracers, one render sequence -- a long launch, short overlapped launches, a progressive replay -- and one
    of them traces between the steps (tests/test_gpu_query.py's pattern).  64 x 48: one wave of the tile sort."""
    plain, trc = tracer(cornell_scene), tracer(cornell_scene)
    for pt in (plain, trc):
        pt.set_moments(True)
    rays, seeds = TC.ray_batch(cornell_scene, 17, 0.3)
    want = H.trace_host(cornell_scene, rays, seeds, n_frames=2, max_bounce=8)

    def state(pt):
        mom, n = pt.read_moments()
        to = pt.tile_order()
        return dict(image=pt.read_rgba32f(), moments=mom, frames=n, sorts=to["sorts"], perm=to["perm"],
                    grid=(to["n_tiles"], to["tiles_x"]), launches=pt.launches(), sweep=pt.leaf_sweep(),
                    pooled=pt.pooled(), n_timed=pt.timing()[1], rgba8=pt.read_rgba8())

    def check(step):
        a, b = state(plain), state(trc)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (step, k)
            else:
                assert a[k] == b[k], (step, k, a[k], b[k])

    def trace():
        TC.same_device(trc.trace(rays, seeds, 1, 2), want, "a trace between renders")

    for pt in (plain, trc):
        pt.render(1, 40, 0)
    trace()
    check("a long launch")
    for pt in (plain, trc):
        for f in range(41, 49):
            pt.render_async(f, 1, 1)
            if pt is trc and f == 44:
                read = device_trace(pt, rays, seeds, 1, 2, wait=False)   # between launches in flight
        pt.sync()
    TC.same_device(read(), want, "a device trace between launches in flight")
    trace()
    check("short overlapped launches")
    for pt in (plain, trc):
        pt.progressive_setup(2, 2)
    trace()                                                    # the captured graph stays
    for pt in (plain, trc):
        pt.progressive_run(1)
    trace()
    for pt in (plain, trc):
        pt.progressive_run(1)
    check("a progressive replay")
    for pt in (plain, trc):
        pt.render(9, 20, 1)
    trace()
    check("a later render")
    plain.close()
    trc.close()


# ---------------------------------------------------------------- the command line
def test_cli_radiance_and_pick(tmp_path):
    obj, mtl = pt_scenes.write_scene("cornell", str(tmp_path))
    sc = H.setupBuffers(obj, mtl)
    rays, seeds = TC.ray_batch(sc, 17, 0.3)
    rpath, spath, gpath = str(tmp_path / "rays.bin"), str(tmp_path / "seeds.bin"), str(tmp_path / "radiance.bin")
    rays.tofile(rpath)
    seeds.tofile(spath)
    picks = [(5, 5), (32, 24), (40, 30), (63, 47)]
    args = [EXE, obj, mtl, "--width", str(W), "--height", str(HH), "--bounces", "3", "--rays", rpath, "--radiance", gpath]
    # without --spp: frame 1, nothing rendered, default seeds
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    TC.same_device(np.fromfile(gpath, f32), H.trace_host(sc, rays, None, n_frames=1, max_bounce=3), "--rays / --radiance")
    # with --seeds, --spp and --pick: frames 1..2, and the pick lines gain the traced colour
    for x, y in picks:
        args += ["--pick", "%d,%d" % (x, y)]
    out = subprocess.run(args + ["--seeds", spath, "--spp", "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    TC.same_device(np.fromfile(gpath, f32), H.trace_host(sc, rays, seeds, n_frames=2, max_bounce=3), "--seeds --spp 2")
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith('{"pick"')]
    assert len(lines) == len(picks)
    xy = np.array(picks, np.int32)
    want = H.trace_host(sc, H.pixel_rays(W, HH, sc["cam"], xy), H.pixel_seeds(xy), n_frames=2, max_bounce=3)
    for ln, (x, y), rgba in zip(lines, picks, want):
        assert ln["pick"] == [x, y]
        assert np.array_equal(np.array(ln["radiance"], f32).view(np.uint32), rgba[0:3].view(np.uint32))   # %.9g round-trips
    # --pick alone keeps today's line
    out = subprocess.run(args[:7] + ["--pick", "5,5"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "radiance" not in out.stdout
    bad = subprocess.run(args[:7] + ["--rays", rpath, "--seeds", spath, "--hits", gpath], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2
