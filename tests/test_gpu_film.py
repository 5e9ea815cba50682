"""The film on the GPU (pt_api.h: pt_film_*; ptrace --film), word for word against code that was there
before it: the image against pt_trace_camera_device, the moments against numpy binary32 folds of one-frame
pt_trace_camera calls, the guides against pt_trace_camera on contexts of display modes 2, 3 and 4, the noise summary
against pt_noise_host, the filter against pt_denoise_host, and the four planes of a pinhole film against a context's
own render, moments, guides and denoise.  Every comparison is of uint32 words (or bytes), with no tolerance.

The image is 40 x 26 = 1,040 pixels, tests/test_gpu_camera.py's: 16 blocks of 64 and a ragged 16.  The kernel's grid is
capped at 1 and at 3 workgroups through pt__film_debug, and uncapped: the three refill regimes.  Bounces are 8, and
the films keep guides of G = 3 frames."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import camera_cases as CC
import denoise_model as M
import film_cases as FC
import pt_host as H
import pt_scenes
import query_cases as QC
from test_gpu_camera import DeviceArray, device_trace
from test_gpu_cli import EXE, read_pfm

pytestmark = pytest.mark.gpu

f32 = np.float32
W, HH, B, G = 40, 26, 8, 3
GRID_CAP = 0                                   # ptfilm::Debug (csrc/pt_film_launch.h)
CAPS = [1, 3, 0]
FRAME_SETS = [(1, 1, 0), (1, 3, 0), (5, 2, 1)]
SCENES = ["fuzz24", "fuzz300", "cornell"]
PLANES = ("image", "moments", "guides")


def tracer(sc, flags=0, mode=1):
    pt = H.PathTracer(W, HH, max_bounce=B, display_mode=mode, flags=flags)
    pt.upload(sc)
    return pt


def cap_grid(value):
    assert H.lib().pt__film_debug(GRID_CAP, value) == 0


@pytest.fixture(autouse=True)
def default_debug_settings():
    yield
    cap_grid(0)


def scene_camera(sc, model, aa=True):
    return CC.camera(model, W, HH, sc["cam"], aa=aa, aperture=0.1, focus=5.0, ortho_width=6.0)


def planes(film):
    return {k: film.read(k) for k in PLANES}


def same_planes(got, want, what):
    for k in PLANES:
        FC.same(got[k], want[k], "%s: %s" % (what, k))


# ---------------------------------------------------------------- 1. the image, and every plane against the host twin
@pytest.mark.parametrize("model", CC.MODELS)
@pytest.mark.parametrize("name", SCENES)
def test_image_and_host_twin(name, model, cornell_scene):
    sc = QC.scene(name, cornell_scene)
    c = scene_camera(sc, model)
    host, state = [], None
    for first, n, acc in FRAME_SETS:                     # the host twin's chain, once for the three caps
        state = H.film_expose_host(sc, c, G, first, n, acc, state=state, max_bounce=B)
        host.append(state)
    pt = tracer(sc)
    for cap in CAPS:
        cap_grid(cap)
        film = H.Film(pt, c, G)
        for (first, n, acc), want in zip(FRAME_SETS, host):
            what = "%s %s frames %d..%d acc %d cap %d" % (name, model, first, first + n - 1, acc, cap)
            prior = film.read("image").reshape(-1, 4) if acc else None
            film.expose(first, n, acc)
            got = planes(film)
            FC.same(got["image"].reshape(-1, 4), device_trace(pt, c, first, n, prior), what + ": pt_trace_camera_device")
            same_planes(got, want, what + ": film_expose_host")
            assert film.info() == (want["frames"], want["guides_held"]), what
        film.close()
    assert not np.isnan(host[-1]["image"]).any() and len(np.unique(FC.words(host[-1]["image"]))) > 8
    pt.close()


# ---------------------------------------------------------------- 2. the moments
@pytest.mark.parametrize("name", SCENES)
def test_moments(name, cornell_scene):
    sc = QC.scene(name, cornell_scene)
    c = scene_camera(sc, "thinlens")
    pt = tracer(sc)
    colours = {f: pt.trace_camera(c, f, 1) for f in range(1, 9)}      # independent of the new kernel
    for cap in CAPS:
        cap_grid(cap)
        film = H.Film(pt, c, G)
        film.expose(1, 8, 0)
        FC.same(film.read("moments"), FC.fold_moments([colours[f] for f in range(1, 9)]), "frames 1..8, cap %d" % cap)
        assert film.info()[0] == 8
        film.expose(3, 2, 0)                                          # a restart: from (0, 0), n = 2
        restarted = FC.fold_moments([colours[3], colours[4]])
        FC.same(film.read("moments"), restarted, "a restart, cap %d" % cap)
        assert film.info()[0] == 2
        film.expose(7, 2, 1)                                          # ... continued: n = 4
        FC.same(film.read("moments"), FC.fold_moments([colours[7], colours[8]], restarted), "continued, cap %d" % cap)
        assert film.info()[0] == 4
        film.close()
    m = FC.fold_moments([colours[f] for f in range(1, 9)])
    assert (m[..., 0] > 0).any() and len(np.unique(m)) > 8
    pt.close()


# ---------------------------------------------------------------- 3. the guides
@pytest.mark.parametrize("flags", [0, H.PT_FLAG_NO_SKY])
@pytest.mark.parametrize("name,model", [("cornell", "thinlens"), ("fuzz24", "equirect"), ("fuzz300", "thinlens"),
                                        ("fuzz24", "ortho")])
def test_guides(name, model, flags, cornell_scene):
    """Existing code only on the right: pt_trace_camera(cam, 1, 3, 0) on contexts of display modes 2, 3 and 4.  The
    panorama of the fuzz scene sees the sky."""
    sc = QC.scene(name, cornell_scene)
    c = scene_camera(sc, model)
    modes = {m: tracer(sc, flags, m) for m in (2, 3, 4)}
    want = FC.guides_of(lambda cam, first, n, mode: modes[mode].trace_camera(cam, first, n), c, G)
    for pt in modes.values():
        pt.close()
    if model == "equirect":
        rays = H.camera_rays_host(scene_camera(sc, model, aa=False), np.stack(np.meshgrid(np.arange(W), np.arange(HH)), -1)
                                  .reshape(-1, 2).astype(np.int32), 1)[0]
        kinds = H.intersect_host(sc, rays, flags=flags)["kind"]
        assert (kinds == H.PT_HIT_NONE).any() and (kinds != H.PT_HIT_NONE).any()
    for own_mode in (1, 3):                              # the context's display mode governs the radiance only
        pt = tracer(sc, flags, own_mode)
        for cap in CAPS:
            cap_grid(cap)
            film = H.Film(pt, c, G)
            film.expose(1, 8, 0)
            what = "%s %s flags %d mode %d cap %d" % (name, model, flags, own_mode, cap)
            FC.same(film.read("guides"), want, what + ": guides")
            FC.same(film.read("image"), pt.trace_camera(c, 1, 8), what + ": image")
            assert film.info() == (8, G)
            film.close()
        pt.close()
    assert len(np.unique(FC.words(want[..., :7]))) > 4 and not want[..., 7].any()


# ---------------------------------------------------------------- 4. chunks across G
@pytest.mark.parametrize("name", SCENES)
def test_chunk_invariance_and_completion(name, cornell_scene):
    sc = QC.scene(name, cornell_scene)
    c = scene_camera(sc, "thinlens")
    pt = tracer(sc)
    for cap in CAPS:
        cap_grid(cap)
        whole, parts = H.Film(pt, c, G), H.Film(pt, c, G)
        whole.expose(1, 8, 0)
        parts.expose(1, 2, 0)
        assert parts.info() == (2, 2)
        parts.expose(3, 6, 1)
        assert parts.info() == (8, 3)
        same_planes(planes(parts), planes(whole), "%s cap %d: 1..2 then 3..8" % (name, cap))
        # frames 5..6 on a new film hold no guide frame; the denoise gathers frames 1..3 alone
        late, early = H.Film(pt, c, G), H.Film(pt, c, G)
        late.expose(5, 2, 0)
        assert late.info() == (2, 0) and not late.read("guides").any()
        early.expose(1, 3, 0)
        early.expose(5, 2, 0)
        assert early.info() == (2, 3)
        before = planes(late)
        info = late.denoise(guide_frames=G)
        assert info["guides_rendered"] and info["guided"] and late.info() == (2, 3)
        assert not early.denoise(guide_frames=G)["guides_rendered"]
        after = planes(late)
        FC.same(after["image"], before["image"], "a guides-only launch leaves the image")
        FC.same(after["moments"], before["moments"], "a guides-only launch leaves the moments")
        same_planes(after, planes(early), "%s cap %d: completed guides" % (name, cap))
        FC.same(late.read("denoised"), early.read("denoised"), "%s cap %d: denoised" % (name, cap))
        FC.same(after["guides"], whole.read("guides"), "%s cap %d: the guides of frames 1..3" % (name, cap))
        # another guide_frames re-gathers
        assert late.denoise(guide_frames=2)["guides_rendered"] and late.info() == (2, 2)
        two = H.Film(pt, c, 2)
        two.expose(1, 2, 0)
        FC.same(late.read("guides"), two.read("guides"), "guide_frames 2")
        for f in (whole, parts, late, early, two):
            f.close()
    pt.close()


# ---------------------------------------------------------------- 5. noise and the stop rule
def test_noise_and_stop_rule(cornell_scene):
    sc = cornell_scene
    c = scene_camera(sc, "thinlens")
    batch, max_frames = 2, 12
    # the host twin's own sequence of summaries, batch by batch: the target is the mean q of a batch strictly inside
    seq, state = [], None
    for k in range(max_frames // batch):
        state = H.film_expose_host(sc, c, G, 1 + k * batch, batch, int(k > 0), state=state, max_bounce=B)
        seq.append(H.noise_host(state["moments"], state["frames"], 0.0))
    px = W * HH
    stop = next(k for k in range(1, len(seq) - 1) if seq[k]["sum_q"] // px + 1 < min(s["sum_q"] // px for s in seq[:k]))
    target = (seq[stop]["sum_q"] // px + 1) / 65536.0                  # a multiple of 2^-16 below 64: exact in binary32
    tq = int(f32(target) * f32(65536.0))
    assert all(s["sum_q"] > tq * px for s in seq[:stop]) and seq[stop]["sum_q"] <= tq * px
    pt = tracer(sc)
    for cap in CAPS:
        cap_grid(cap)
        film = H.Film(pt, c, G)
        film.expose(1, 8, 0)
        mom = film.read("moments")
        for t in (0.0, 0.05, target):
            assert film.noise(t) == H.noise_host(mom, 8, t), "pt_film_noise, target %g cap %d" % (t, cap)
        done, last = film.expose_until(target, batch=batch, max_frames=max_frames)
        # the Python loop over pt_noise_host on the film's own moments
        loop, frames = H.Film(pt, c, G), 0
        while frames < max_frames:
            loop.expose(1 + frames, batch, int(frames > 0))
            frames += batch
            s = H.noise_host(loop.read("moments"), frames, target)
            if s["sum_q"] <= tq * s["pixels"]:
                break
        assert done == frames == (stop + 1) * batch and batch < done < max_frames
        assert last == s and last["frames"] == done and film.info() == (done, G)
        once = H.Film(pt, c, G)
        once.expose(1, done, 0)
        same_planes(planes(film), planes(once), "expose_until against expose(1, %d, 0), cap %d" % (done, cap))
        # a target never met runs to max_frames with a shorter last batch
        done, last = film.expose_until(1e-6, batch=5, max_frames=7)
        assert done == 7 and film.info()[0] == 7
        once.expose(1, 7, 0)
        same_planes(planes(film), planes(once), "a shorter last batch, cap %d" % cap)
        for f in (film, loop, once):
            f.close()
    pt.close()


def test_errors(cornell_scene):
    L = H.lib()
    pt = H.PathTracer(W, HH, max_bounce=B)
    c = scene_camera(cornell_scene, "thinlens")
    film = H.Film(pt, c, G)                              # a film needs no scene ...
    assert L.pt_film_expose(film.h, 1, 1, 0) == -6       # ... an exposure does: PT_E_STATE
    done, stats, info = C.c_int(), H.NoiseStats(), H.DenoiseInfo()
    assert L.pt_film_expose_until(film.h, 1, 0, 2, 4, 0.1, C.byref(done), C.byref(stats)) == -6
    assert L.pt_film_denoise(film.h, None, C.byref(info)) == -6
    pt.upload(cornell_scene)
    assert L.pt_film_noise(film.h, 0.1, C.byref(stats)) == -6                      # n < 2
    film.expose(1, 1, 0)
    assert L.pt_film_noise(film.h, 0.1, C.byref(stats)) == -6
    for args in ((0, 1, 0), (1, 0, 0), (2 ** 31 - 1, 1, 0), (1, 1, 2)):
        assert L.pt_film_expose(film.h, *args) == -1, args
    assert L.pt_film_expose(None, 1, 1, 0) == -1
    for batch, max_frames, target in ((1, 4, 0.1), (4, 3, 0.1), (2, 4, 0.0), (2, 4, float("nan"))):
        assert L.pt_film_expose_until(film.h, 1, 0, batch, max_frames, target, C.byref(done), None) == -1
    assert L.pt_film_expose_until(film.h, 1, 0, 2, 4, 0.1, None, None) == -1
    assert L.pt_film_noise(film.h, 0.1, None) == -1
    out = np.zeros((HH, W, 4), f32)
    assert L.pt_film_read(film.h, H.PT_FILM_DENOISED, out.ctypes.data, out.nbytes) == -6      # before a denoise
    assert L.pt_film_read(film.h, H.PT_FILM_DENOISED_ACES8, out.ctypes.data, W * HH * 4) == -6
    assert L.pt_film_read(film.h, H.PT_FILM_IMAGE, out.ctypes.data, out.nbytes - 4) == -1     # a wrong size
    assert L.pt_film_read(film.h, H.PT_FILM_IMAGE, out.ctypes.data, out.nbytes + 4) == -1
    assert L.pt_film_read(film.h, H.PT_FILM_MOMENTS, out.ctypes.data, out.nbytes) == -1
    assert L.pt_film_read(film.h, 6, out.ctypes.data, out.nbytes) == -1
    assert L.pt_film_read(film.h, H.PT_FILM_IMAGE, None, out.nbytes) == -1
    bad = H.denoise_params(iterations=9)
    assert L.pt_film_denoise(film.h, C.byref(bad), None) == -1
    bad = H.denoise_params(guide_frames=0)
    assert L.pt_film_denoise(film.h, C.byref(bad), None) == -1
    other = C.c_void_p()
    assert L.pt_film_create(pt.h, C.byref(c), 0, C.byref(other)) == -1
    assert L.pt_film_create(pt.h, None, G, C.byref(other)) == -1
    assert L.pt_film_create(pt.h, C.byref(H.Camera("thinlens", W, HH, aperture=-1.0)), G, C.byref(other)) == -1
    assert L.pt_film_set_camera(film.h, C.byref(CC.camera("thinlens", W + 1, HH, cornell_scene["cam"]))) == -1
    assert L.pt_film_set_camera(film.h, None) == -1
    assert L.pt__film_debug(2, 0) == -1 and L.pt__film_debug(GRID_CAP, -1) == -1 and L.pt__film_debug(1, 3) == -1
    p, n = film.device("image")
    assert p and n == out.nbytes and film.device("guides")[1] == 2 * out.nbytes
    with pytest.raises(H.PTError):
        film.device("denoised")
    film.expose(1, 2, 0)
    assert film.noise(0.1)["pixels"] == W * HH
    film.close()
    pt.close()


# ---------------------------------------------------------------- 6. the filter
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("n", [8, 1])
def test_denoise(n, iterations, cornell_scene):
    sc = cornell_scene
    c = scene_camera(sc, "thinlens")
    pt = tracer(sc)
    film = H.Film(pt, c, G)
    film.expose(1, n, 0)
    info = film.denoise(iterations=iterations)
    assert info == dict(guided=n >= 2, guides_rendered=n < G, iterations=iterations, frames=n)
    p = planes(film)
    var = M.variance_of(p["moments"], n) if n >= 2 else None
    want = H.denoise_host(p["image"], var, p["guides"], iterations=iterations, guide_frames=G)
    got = film.read("denoised")
    FC.same(got, want, "n %d iterations %d: pt_denoise_host" % (n, iterations))
    assert np.any(FC.words(got[..., :3]) != FC.words(p["image"][..., :3]))
    FC.same(got[..., 3], p["image"][..., 3], "alpha is the image's")
    FC.same(film.read("denoised_aces8"), H.aces_rgba8_host(got), "the denoised ACES view")
    FC.same(film.read("image_aces8"), H.aces_rgba8_host(p["image"]), "the image's ACES view")
    dev, nbytes = film.device("denoised")
    assert dev and nbytes == got.nbytes
    film.close()
    pt.close()


# ---------------------------------------------------------------- 7. the pinhole identity
def test_pinhole_film_is_the_context(cornell_scene):
    """Nothing on the right-hand side is new code: a flags-0 context's render, moments, guides and denoise."""
    sc = cornell_scene
    pt = tracer(sc)
    pt.set_moments(True)
    pt.render(1, 8, 0)
    info = pt.denoise(guide_frames=G)
    assert info["guided"]
    mom, n = pt.read_moments()
    want = dict(image=pt.read_rgba32f(), moments=mom, guides=pt.read_guides(), denoised=pt.read_denoised())
    assert n == 8
    film_ctx = tracer(sc)
    for cap in CAPS:
        cap_grid(cap)
        film = H.Film(film_ctx, CC.camera("pinhole", W, HH, sc["cam"]), G)
        film.expose(1, 8, 0)
        assert film.denoise(guide_frames=G)["guided"]
        for k in want:
            FC.same(film.read(k), want[k], "cap %d: %s" % (cap, k))
        film.close()
    FC.same(H.aces_rgba8_host(want["denoised"]), pt.read_denoised_rgba8(), "the context's own ACES view")
    pt.close()
    film_ctx.close()


# ---------------------------------------------------------------- 8. invisible, and the scene serial
def test_film_calls_are_invisible(cornell_scene):
    """Two tracers, one render sequence -- a long launch, short overlapped launches, a progressive replay -- and one of
    them exposes, summarises, filters and reads a film between the steps (tests/test_gpu_camera.py's pattern)."""
    sc = cornell_scene
    plain, trc = tracer(sc), tracer(sc)
    for pt in (plain, trc):
        pt.set_moments(True)
    c = scene_camera(sc, "thinlens")
    want = H.film_expose_host(sc, c, G, 1, 3, 0, max_bounce=B)
    film = H.Film(trc, c, G)

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

    def film_calls():
        cap_grid(CAPS[turn[0] % 3])
        turn[0] += 1
        film.expose(1, 3, 0)
        same_planes(planes(film), want, "a film exposed between renders")
        assert film.noise(0.1)["pixels"] == W * HH
        film.denoise(guide_frames=G)
        film.read("denoised_aces8")

    for pt in (plain, trc):
        pt.render(1, 40, 0)
    film_calls()
    check("a long launch")
    for pt in (plain, trc):
        for f in range(41, 49):
            pt.render_async(f, 1, 1)
            if pt is trc and f == 44:                    # between launches in flight, not synchronised
                film.expose(1, 3, 0)
        pt.sync()
    same_planes(planes(film), want, "a film exposed between launches in flight")
    film_calls()
    check("short overlapped launches")
    for pt in (plain, trc):
        pt.progressive_setup(2, 2)
    film_calls()                                         # the captured graph stays
    for pt in (plain, trc):
        pt.progressive_run(1)
    film_calls()
    for pt in (plain, trc):
        pt.progressive_run(1)
    check("a progressive replay")
    for pt in (plain, trc):
        pt.render(9, 20, 1)
    film_calls()
    check("a later render")
    film.close()
    plain.close()
    trc.close()


def test_scene_serial_and_set_camera(cornell_scene):
    other = QC.scene("fuzz300")
    c = scene_camera(cornell_scene, "thinlens")
    pt = tracer(cornell_scene)
    film = H.Film(pt, c, G)
    pt.render_async(1, 4, 0)                             # an exposure behind an unsynchronised render: that scene's
    film.expose(1, 8, 0)
    old = planes(film)
    same_planes(old, H.film_expose_host(cornell_scene, c, G, 1, 8, 0, max_bounce=B), "behind a render in flight")
    assert film.info() == (8, G)
    pt.upload(other)
    assert film.info() == (8, 0)                         # the guides were another scene's
    film.expose(4, 2, 1)                                 # holds no guide frame: the old planes stay ...
    assert film.info() == (10, 0)
    FC.same(film.read("guides"), old["guides"], "no guide frame in the range")
    film.expose(1, 8, 0)                                 # ... and this one gathers the new scene's
    same_planes(planes(film), H.film_expose_host(other, c, G, 1, 8, 0, max_bounce=B), "after an upload")
    assert film.info() == (8, G) and np.any(FC.words(film.read("guides")) != FC.words(old["guides"]))
    # a camera move: the viewer's restart
    moved = scene_camera(dict(cam=np.asarray(other["cam"], f32) + f32(0.25)), "thinlens")
    film.set_camera(moved)
    assert film.info() == (8, 0)
    film.expose(1, 4, 0)
    same_planes(planes(film), H.film_expose_host(other, moved, G, 1, 4, 0, max_bounce=B), "after a camera move")
    with pytest.raises(H.PTError) as e:
        film.set_camera(CC.camera("thinlens", W, HH + 1, other["cam"]))
    assert e.value.code == -1 and film.info() == (4, G)
    film.close()
    pt.close()


# ---------------------------------------------------------------- 9. the command line
def test_cli_film(tmp_path):
    obj, mtl = pt_scenes.write_scene("cornell", str(tmp_path))
    sc = H.setupBuffers(obj, mtl)
    c = CC.camera("thinlens", W, HH, sc["cam"], aperture=0.05, focus=5.5)
    # a target met strictly inside --max-spp, from the host twin's own sequence
    seq, state = [], None
    for k in range(6):
        state = H.film_expose_host(sc, c, G, 1 + 2 * k, 2, int(k > 0), state=state, max_bounce=B)
        seq.append(H.noise_host(state["moments"], state["frames"], 0.0)["sum_q"] // (W * HH))
    stop = next(k for k in range(1, 5) if seq[k] + 1 < min(seq[:k]))
    target = (seq[stop] + 1) / 65536.0
    pfm, dpfm = str(tmp_path / "film.pfm"), str(tmp_path / "film_dn.pfm")
    args = [EXE, obj, mtl, "--width", str(W), "--height", str(HH), "--bounces", str(B), "--ppm", str(tmp_path / "film.ppm")]
    out = subprocess.run(args + ["--camera-model", "thinlens", "--aperture", "0.05", "--focus", "5.5", "--film",
                                 "--noise-target", "%.20f" % target, "--batch", "2", "--max-spp", "12", "--denoise",
                                 "--guide-frames", str(G), "--denoise-pfm", dpfm, "--pfm", pfm, "--json"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    summary = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    pt = tracer(sc)
    film = H.Film(pt, c, G)
    done, last = film.expose_until(float(f32(target)), batch=2, max_frames=12)
    assert done == 2 * (stop + 1) and 2 < done < 12
    film.denoise(guide_frames=G)
    rgb = lambda a: np.ascontiguousarray(a[..., :3])
    FC.same(read_pfm(pfm), rgb(film.read("image")), "--pfm")
    FC.same(read_pfm(dpfm), rgb(film.read("denoised")), "--denoise-pfm")
    assert summary["frames"] == done and summary["frames_done"] == done
    assert summary["film"]["frames"] == done and summary["film"]["guides_held"] == G
    assert summary["film"]["sum_q"] == last["sum_q"] and summary["denoise"]["guided"] == 1
    film.close()
    pt.close()
    bad = subprocess.run(args + ["--film", "--spp", "2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--film needs --camera-model" in bad.stderr
    bad = subprocess.run(args + ["--camera-model", "thinlens", "--film", "--noise-target", "0.1", "--adaptive"],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--camera-model excludes --adaptive" in bad.stderr
