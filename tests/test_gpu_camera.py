"""Camera models on the GPU (pt_api.h: pt_trace_camera, pt_trace_camera_device, pt_camera_rays_device; ptrace
--camera-model) against the host twin (pt_trace_camera_host and pt_camera_rays_host, themselves checked
against the oracle's default renders and a float64 model in tests/test_camera_host.py), and directly against the
context's own render, word for word: every comparison is of uint32 words, with no tolerance (in the one test with a
degenerate camera a NaN must meet a NaN, but not the same one: trace_cases.same_device).

The image is 40 x 26 = 1,040 pixels: 16 blocks of 64 and a ragged 16.  Every test runs with the kernel's grid capped at
1 and at 3 workgroups through pt__camera_debug, and uncapped: the three refill regimes tests/test_gpu_trace.py names
(every wave refills across several blocks; some waves own one block and some two; one block per wave or none).
Bounces are 8."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import camera_cases as CC
import pt_host as H
import pt_scenes
import query_cases as QC
import trace_cases as TC
from test_gpu_cli import EXE, read_pfm

pytestmark = pytest.mark.gpu

f32 = np.float32
W, HH = 40, 26
N = W * HH
GRID_CAP = 0                                   # ptcam::Debug (csrc/pt_camera_launch.h)
CAPS = [1, 3, 0]
FRAME_SETS = [(1, 1, False), (1, 3, False), (5, 2, True)]
_host = {}


def tracer(sc, flags=0, w=W, h=HH):
    pt = H.PathTracer(w, h, max_bounce=8, flags=flags)
    pt.upload(sc)
    return pt


def cap_grid(value):
    assert H.lib().pt__camera_debug(GRID_CAP, value) == 0


@pytest.fixture(autouse=True)
def default_debug_settings():
    yield
    cap_grid(0)


def prior_image():
    return np.random.default_rng(3).random((N, 4)).astype(f32)


def host(name, sc, c, model, aa, first, n, with_prior):
    """pt_trace_camera_host, computed once per case and shared among the tests."""
    key = (name, model, aa, first, n, with_prior)
    if key not in _host:
        _host[key] = H.trace_camera_host(sc, c, first, n, prior=prior_image() if with_prior else None, max_bounce=8)
        _host[key].setflags(write=False)
    return _host[key]


def _hip():
    L = H.lib()
    for fn, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipFree", [C.c_void_p]),
                     ("hipMemcpy", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int])):
        getattr(L, fn).restype, getattr(L, fn).argtypes = C.c_int, args
    return L


class DeviceArray:
    """A device allocation of the HIP runtime the library links, filled from a numpy array (blocking copies)."""

    def __init__(self, host_array):
        self.host = np.ascontiguousarray(host_array)
        self.p = C.c_void_p()
        assert _hip().hipMalloc(C.byref(self.p), max(self.host.nbytes, 16)) == 0
        assert _hip().hipMemcpy(self.p, self.host.ctypes.data, self.host.nbytes, 1) == 0     # hipMemcpyHostToDevice

    @property
    def ptr(self):
        return self.p.value

    def read(self):
        out = np.empty_like(self.host)
        assert _hip().hipMemcpy(out.ctypes.data, self.p, out.nbytes, 2) == 0                # hipMemcpyDeviceToHost
        return out

    def free(self):
        if self.p.value:
            _hip().hipFree(self.p)
            self.p = C.c_void_p()


def device_trace(pt, c, first, n, prior=None):
    """pt_trace_camera_device on a device image holding the prior, or NaNs an overwriting call never reads."""
    buf = DeviceArray(np.full((c.pixels, 4), np.nan, f32) if prior is None else prior)
    pt.trace_camera_device(c, buf.ptr, first, n, int(prior is not None))
    pt.sync()
    out = buf.read()
    buf.free()
    return out


def device_rays(pt, c, frame):
    rays, states = DeviceArray(np.zeros(c.pixels, H.RAY_DTYPE)), DeviceArray(np.zeros(c.pixels, np.uint32))
    pt.camera_rays_device(c, frame, rays.ptr, states.ptr)
    pt.sync()
    out = rays.read(), states.read()
    rays.free()
    states.free()
    return out


def scene_camera(sc, model, aa, w=W, h=HH):
    return CC.camera(model, w, h, sc["cam"], aa=aa, aperture=0.1, focus=5.0, ortho_width=6.0)


# ---------------------------------------------------------------- 1. device against host
@pytest.mark.parametrize("model", CC.MODELS)
@pytest.mark.parametrize("name", ["cornell", "top769", "fuzz2500", "spheres_only"])
def test_parity(name, model, cornell_scene):
    sc = QC.scene(name, cornell_scene)
    pt = tracer(sc)
    images = []
    for aa in (True, False):
        c = scene_camera(sc, model, aa)
        for first, n, with_prior in FRAME_SETS:
            want = host(name, sc, c, model, aa, first, n, with_prior)
            images.append(want)
            prior = prior_image() if with_prior else None
            for cap in CAPS:
                cap_grid(cap)
                what = "%s %s aa=%d frames %d..%d cap %d" % (name, model, aa, first, first + n - 1, cap)
                TC.same(pt.trace_camera(c, first, n, prior), want, what + " pt_trace_camera")
                TC.same(device_trace(pt, c, first, n, prior), want, what + " pt_trace_camera_device")
    # not vacuous: no NaN, images of more than one colour, and the jitter and further frames move them
    assert not any(np.isnan(im).any() for im in images)
    assert all(len(np.unique(TC.words(im), axis=0)) > 1 for im in images)
    assert np.any(TC.words(images[0]) != TC.words(images[1])) and np.any(TC.words(images[0]) != TC.words(images[3]))
    pt.close()


# ---------------------------------------------------------------- 2. device against the render
@pytest.mark.parametrize("aa", [True, False])
def test_pinhole_is_the_render(aa, cornell_scene):
    """pt_trace_camera(pinhole) writes the pixels of pt_render on a context of the same size and camera: with
    anti-aliasing the default (flags 0) render, the image the NO_AA-only traced rays of §13 cannot reach."""
    pt = tracer(cornell_scene, flags=0 if aa else H.PT_FLAG_NO_AA)
    c = CC.camera("pinhole", W, HH, cornell_scene["cam"], aa=aa)
    pt.render(1, 4, 0)
    fresh = pt.read_rgba32f()
    prior = prior_image().reshape(HH, W, 4)
    pt.write_rgba32f(prior)
    pt.render(2985, 4, 1)
    late = pt.read_rgba32f()
    for cap in CAPS:
        cap_grid(cap)
        TC.same(pt.trace_camera(c, 1, 4), fresh, "aa=%d frames 1..4 cap %d" % (aa, cap))
        TC.same(pt.trace_camera(c, 2985, 4, prior), late, "aa=%d frames 2985..2988 over a prior, cap %d" % (aa, cap))
        TC.same(device_trace(pt, c, 2985, 4, prior.reshape(-1, 4)), late, "aa=%d the same, pt_trace_camera_device" % aa)
    assert len(np.unique(TC.words(fresh), axis=0)) > 1 and np.any(TC.words(fresh) != TC.words(late))
    pt.close()


# ---------------------------------------------------------------- 3. rays on the device
@pytest.mark.parametrize("size", [(W, HH), (1, 1), (65536, 1)])
def test_rays(size, cornell_scene):
    w, h = size
    pt = tracer(cornell_scene)
    xy = TC.image_xy(w, h)
    seen = {}
    for model in CC.MODELS:
        for aa in (True, False):
            c = scene_camera(cornell_scene, model, aa, w, h)
            for frame in (1, 2986):
                want_rays, want_states = H.camera_rays_host(c, xy, frame)
                rays, states = device_rays(pt, c, frame)
                what = "%s aa=%d frame %d %dx%d" % (model, aa, frame, w, h)
                assert np.array_equal(CC.ray_words(rays), CC.ray_words(want_rays)), what
                assert np.array_equal(states, want_states), what
                assert not np.isnan(rays["d"]).any()
                seen[(model, aa, frame)] = CC.ray_words(rays).tobytes()
    jittered = [v for (model, aa, frame), v in seen.items() if aa]
    assert len(set(jittered)) == len(jittered)              # with the jitter every model and frame makes other rays ...
    rays = DeviceArray(np.zeros(w * h, H.RAY_DTYPE))        # ... and the states may be left out
    pt.camera_rays_device(scene_camera(cornell_scene, "thinlens", True, w, h), 2986, rays.ptr, None)
    pt.sync()
    assert CC.ray_words(rays.read()).tobytes() == seen[("thinlens", True, 2986)]
    rays.free()
    pt.close()


# ---------------------------------------------------------------- 4. composition on the device
@pytest.mark.parametrize("model", CC.MODELS)
def test_composition_through_pt_trace_device(model, cornell_scene):
    """pt_camera_rays_device -> pt_trace_device, one frame per call, chained through one device image, is
    pt_trace_camera_device over the same prior."""
    sc = cornell_scene
    pt = tracer(sc)
    c = scene_camera(sc, model, True)
    prior = prior_image()
    for cap in CAPS:
        cap_grid(cap)
        want = device_trace(pt, c, 5, 3, prior)
        img = DeviceArray(prior)
        rays, states = DeviceArray(np.zeros(N, H.RAY_DTYPE)), DeviceArray(np.zeros(N, np.uint32))
        for f in (5, 6, 7):
            pt.camera_rays_device(c, f, rays.ptr, states.ptr)
            pt.sync()
            seeds = DeviceArray(states.read() - np.uint32((f * 719393) & CC.M32))          # uint32 arithmetic wraps
            pt.trace_device(rays.ptr, seeds.ptr, N, img.ptr, f, 1, 1)
            pt.sync()
            seeds.free()
        TC.same(img.read(), want, "%s cap %d" % (model, cap))
        for b in (img, rays, states):
            b.free()
    TC.same(want, host("cornell", sc, c, model, True, 5, 3, True), model + " against the host")
    pt.close()


# ---------------------------------------------------------------- 5. a degenerate camera
def test_fwd_along_z_completes(cornell_scene):
    """fwd = (0, 0, 1): `right` is 0/0, as in the reference.  The input is legal; the rays are NaN and fall out of the
    arithmetic."""
    cam = np.array(cornell_scene["cam"], f32)
    cam[4:7] = [0, 0, 1]
    pt = tracer(cornell_scene)
    for model in CC.MODELS:
        c = CC.camera(model, W, HH, cam, aperture=0.1, focus=5.0, ortho_width=6.0)
        want = H.trace_camera_host(cornell_scene, c, 1, 2, max_bounce=8)
        for cap in CAPS:
            cap_grid(cap)
            TC.same_device(pt.trace_camera(c, 1, 2), want, "%s fwd = z, cap %d" % (model, cap))
    pt.close()


# ---------------------------------------------------------------- errors
def test_errors(cornell_scene):
    pt = H.PathTracer(W, HH)
    L = H.lib()
    c = CC.camera("thinlens", 4, 3, cornell_scene["cam"])
    g = C.byref(c)
    out = np.zeros((12, 4), f32)
    o = out.ctypes.data
    with pytest.raises(H.PTError) as e:
        pt.trace_camera(c)
    assert e.value.code == -6                                                  # PT_E_STATE: before an upload
    assert L.pt_trace_camera_device(pt.h, g, 1, 1, 0, C.c_void_p(16)) == -6
    pt.upload(cornell_scene)
    assert L.pt_trace_camera(None, g, 1, 1, 0, o) == -1
    assert L.pt_trace_camera(pt.h, None, 1, 1, 0, o) == -1                     # PT_E_ARG: null camera
    assert L.pt_trace_camera(pt.h, g, 1, 1, 0, None) == -1                     # null rgba
    assert L.pt_trace_camera(pt.h, g, 0, 1, 0, o) == -1                        # frame_first < 1
    assert L.pt_trace_camera(pt.h, g, 1, 0, 0, o) == -1                        # n_frames < 1
    assert L.pt_trace_camera(pt.h, g, 2 ** 31 - 1, 1, 0, o) == -1              # frame_first + n_frames overflows int
    assert L.pt_trace_camera(pt.h, g, 1, 1, 2, o) == -1                        # accumulate_first not 0 or 1
    assert L.pt_trace_camera_device(pt.h, g, 1, 1, 0, None) == -1
    assert L.pt_trace_camera_device(pt.h, g, 1, 1, 0, C.c_void_p(24)) == -1    # misaligned, before any launch
    assert L.pt_trace_camera_device(pt.h, g, 1, 0, 0, C.c_void_p(32)) == -1
    assert L.pt_camera_rays_device(pt.h, None, 1, C.c_void_p(32), None) == -1
    assert L.pt_camera_rays_device(pt.h, g, 0, C.c_void_p(32), None) == -1     # frame < 1
    assert L.pt_camera_rays_device(pt.h, g, 1, None, None) == -1
    assert L.pt_camera_rays_device(pt.h, g, 1, C.c_void_p(8), None) == -1      # misaligned rays
    assert L.pt_camera_rays_device(pt.h, g, 1, C.c_void_p(32), C.c_void_p(2)) == -1
    from test_camera_host import bad_cameras
    for what, bad in bad_cameras(cornell_scene["cam"]):
        assert L.pt_trace_camera(pt.h, C.byref(bad), 1, 1, 0, o) == -1, what
        assert L.pt_trace_camera_device(pt.h, C.byref(bad), 1, 1, 0, C.c_void_p(32)) == -1, what
        assert L.pt_camera_rays_device(pt.h, C.byref(bad), 1, C.c_void_p(32), None) == -1, what
    assert L.pt__camera_debug(2, 0) == -1 and L.pt__camera_debug(GRID_CAP, -1) == -1 and L.pt__camera_debug(1, 2) == -1
    assert L.pt_trace_camera(pt.h, g, 1, 1, 0, o) == 0 and np.all(out[:, 3] == 1.0)
    pt.close()


# ---------------------------------------------------------------- 6. invisibility
def test_camera_calls_are_invisible(cornell_scene):
    """Two tracers, one render sequence -- a long launch, short overlapped launches, a progressive replay -- and one
    of them traces cameras and makes camera rays between the steps (tests/test_gpu_trace.py's pattern)."""
    plain, trc = tracer(cornell_scene), tracer(cornell_scene)
    for pt in (plain, trc):
        pt.set_moments(True)
    cams = [scene_camera(cornell_scene, m, True) for m in CC.MODELS]
    wants = [host("cornell", cornell_scene, c, m, True, 1, 3, False) for c, m in zip(cams, CC.MODELS)]
    xy = TC.image_xy(W, HH)

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

    turn = [0]

    def camera_calls():
        k = turn[0] % 4
        turn[0] += 1
        cap_grid(CAPS[k % 3])
        TC.same(trc.trace_camera(cams[k], 1, 3), wants[k], "a camera trace between renders")
        rays, states = device_rays(trc, cams[k], 2)
        want_rays, want_states = H.camera_rays_host(cams[k], xy, 2)
        assert np.array_equal(CC.ray_words(rays), CC.ray_words(want_rays)) and np.array_equal(states, want_states)

    for pt in (plain, trc):
        pt.render(1, 40, 0)
    camera_calls()
    check("a long launch")
    for pt in (plain, trc):
        buf = None
        for f in range(41, 49):
            pt.render_async(f, 1, 1)
            if pt is trc and f == 44:                    # between launches in flight
                buf = DeviceArray(np.full((N, 4), np.nan, f32))
                pt.trace_camera_device(cams[1], buf.ptr, 1, 3, 0)
        pt.sync()
        if buf is not None:
            TC.same(buf.read(), wants[1], "a device camera trace between launches in flight")
            buf.free()
    camera_calls()
    check("short overlapped launches")
    for pt in (plain, trc):
        pt.progressive_setup(2, 2)
    camera_calls()                                       # the captured graph stays
    for pt in (plain, trc):
        pt.progressive_run(1)
    camera_calls()
    for pt in (plain, trc):
        pt.progressive_run(1)
    check("a progressive replay")
    for pt in (plain, trc):
        pt.render(9, 20, 1)
    camera_calls()
    check("a later render")
    plain.close()
    trc.close()


# ---------------------------------------------------------------- 7. the command line
def test_cli_thin_lens_and_a_refusal(tmp_path):
    obj, mtl = pt_scenes.write_scene("cornell", str(tmp_path))
    sc = H.setupBuffers(obj, mtl)
    x, y = 20, 9
    pfm = str(tmp_path / "lens.pfm")
    args = [EXE, obj, mtl, "--width", str(W), "--height", str(HH), "--bounces", "8", "--ppm", str(tmp_path / "lens.ppm")]
    out = subprocess.run(args + ["--camera-model", "thinlens", "--aperture", "0.05", "--focus-at", "%d,%d" % (x, y),
                                 "--spp", "4", "--chunk", "3", "--pfm", pfm], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    pt = tracer(sc)
    hit = pt.pick(np.array([[x, y]], np.int32))[0]
    assert hit["kind"] != H.PT_HIT_NONE
    cam = np.asarray(sc["cam"], f32)
    fwd, rel = CC.normalize32(cam[4:7]), (hit["p"][0:3] - cam[0:3]).astype(f32)
    focus = f32(f32(f32(rel[0] * fwd[0]) + f32(rel[1] * fwd[1])) + f32(rel[2] * fwd[2]))       # dot(p - pos, fwd), binary32
    assert 1.0 < focus < 20.0
    c = CC.camera("thinlens", W, HH, cam, aperture=0.05, focus=float(focus))
    want = pt.trace_camera(c, 1, 4)
    got = read_pfm(pfm)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want[..., :3]).view(np.uint32))
    # the lens is on: another focus distance is another image
    assert np.any(TC.words(want) != TC.words(pt.trace_camera(CC.camera("thinlens", W, HH, cam, aperture=0.05, focus=1.0), 1, 4)))
    pt.close()
    bad = subprocess.run(args + ["--camera-model", "ortho", "--noise-target", "0.1"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--camera-model excludes --noise-target" in bad.stderr
    sky = subprocess.run(args + ["--camera-model", "thinlens", "--focus-at", "20,2", "--spp", "1"], capture_output=True,
                         text=True, timeout=120)
    assert sky.returncode != 0 and "nothing under that pixel" in sky.stderr
