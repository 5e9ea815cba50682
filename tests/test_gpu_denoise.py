"""The denoised view on the GPU (pt_api.h: pt_denoise, pt_read_denoised_*, pt_read_guides; ptrace
--denoise).  The guides against the oracle's renders in display modes 2, 3 and 4,
the filter against the host twin (pt_denoise_host) and the numpy restatement of its definition
(tests/denoise_model.py) fed with the tracer's own image, guides and moments -- all bit for bit --
and a context that denoises against one that never does.  Cornell box, 8 bounces, unless a case
says otherwise."""
import json
import subprocess

import numpy as np
import pytest

import denoise_model as M
import fuzz_scenes
import oracle_lib as O
import pt_host as H
import pt_scenes
from test_gpu_cli import EXE, read_pfm
from test_gpu_noise import same_bits
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu

f32 = np.float32
B = 8


def tracer(sc, w, h, moments=False, max_bounce=B, **kw):
    pt = H.PathTracer(w, h, max_bounce=max_bounce, **kw)
    pt.upload(sc)
    if moments:
        pt.set_moments(True)
    return pt


def oracle_guides(sc, w, h, guide_frames, max_bounce=B, flags=0):
    """(h, w, 8) = N.rgb, Z, A.rgb, 0 from the oracle's mode-2/3/4 renders of guide_frames frames."""
    n, a, z = (O.render(sc, w, h, max_bounce=max_bounce, mode=m, n_frames=guide_frames, flags=flags) for m in (2, 3, 4))
    g = np.zeros((h, w, 8), f32)
    g[..., 0:3], g[..., 3], g[..., 4:7] = n[..., :3], z[..., 0], a[..., :3]
    return g


# ---------------------------------------------------------------- guides
@pytest.mark.parametrize("guide_frames", [1, 3])
def test_guides_cornell(cornell_scene, guide_frames):
    w, h = 61, 37
    pt = tracer(cornell_scene, w, h)
    pt.render(1, 2, 0)
    info = pt.denoise(guide_frames=guide_frames)
    assert info["guides_rendered"] and not info["guided"] and info["frames"] == 0
    same_bits(pt.read_guides(), oracle_guides(cornell_scene, w, h, guide_frames), "guides of %d frames" % guide_frames)
    pt.close()


def test_guides_counting_context(cornell_scene):
    """A counting context: the guide launches never count (their window clause and kernel follow the launch's own
    state, not the context's flag), so the guides are the oracle's and the counters stay those of the render."""
    w, h = 32, 24

    def counters():
        v = np.zeros(16, np.uint64)
        pt._check(H.lib().pt_stats_ex(pt.h, v))
        return v

    pt = tracer(cornell_scene, w, h)
    pt.set_counting(True)
    pt.render(1, 4, 0)
    before = counters()
    assert before[0] > 0, "the render counted nothing"
    assert pt.denoise(guide_frames=2)["guides_rendered"]
    same_bits(pt.read_guides(), oracle_guides(cornell_scene, w, h, 2), "guides on a counting context")
    pt.sync()
    assert np.array_equal(counters(), before)
    pt.close()


def test_guides_cache(cornell_scene):
    """Rendered by the first call, kept by the second; again after set_camera, upload and another guide_frames."""
    w, h = 40, 30
    pt = tracer(cornell_scene, w, h)
    pt.render(1, 1, 0)
    assert pt.denoise()["guides_rendered"] is True
    assert pt.denoise()["guides_rendered"] is False
    assert pt.denoise(iterations=2, sigma_lum=1.0)["guides_rendered"] is False
    cam = cornell_scene["cam"].copy()
    cam[0] += f32(0.5)
    pt.set_camera(cam)
    assert pt.denoise()["guides_rendered"] is True
    moved = dict(cornell_scene, cam=cam)
    same_bits(pt.read_guides(), oracle_guides(moved, w, h, 4), "guides after set_camera")
    assert pt.denoise()["guides_rendered"] is False
    pt.upload(cornell_scene)
    assert pt.denoise()["guides_rendered"] is True
    same_bits(pt.read_guides(), oracle_guides(cornell_scene, w, h, 4), "guides after upload")
    assert pt.denoise(guide_frames=2)["guides_rendered"] is True
    same_bits(pt.read_guides(), oracle_guides(cornell_scene, w, h, 2), "guides of 2 frames")
    assert pt.denoise(guide_frames=2)["guides_rendered"] is False
    pt.close()


def test_guides_ship(ship_scene):
    w, h = 48, 36
    pt = tracer(ship_scene, w, h, max_bounce=5)
    pt.render(1, 1, 0)
    pt.denoise(guide_frames=2)
    same_bits(pt.read_guides(), oracle_guides(ship_scene, w, h, 2, max_bounce=5), "ship guides")
    pt.close()


def test_guides_fuzz_scene():
    sc, kw = fuzz_scenes.random_case(21, n_tris=90)
    w, h = max(kw["W"], 9), max(kw["H"], 9)
    pt = tracer(sc, w, h, max_bounce=kw["max_bounce"], flags=kw["flags"])
    pt.render(1, 1, 0)
    pt.denoise(guide_frames=2)
    same_bits(pt.read_guides(), oracle_guides(sc, w, h, 2, max_bounce=kw["max_bounce"], flags=kw["flags"]),
              "fuzz scene guides")
    pt.close()


@pytest.mark.parametrize("flags", [H.PT_FLAG_NO_AA, H.PT_FLAG_REF_DISPATCH])
def test_guides_flags(cornell_scene, flags):
    w, h = 61, 37
    pt = tracer(cornell_scene, w, h, flags=flags)
    pt.render(1, 1, 0)
    pt.denoise(guide_frames=3)
    g = pt.read_guides()
    # (the oracle renders every pixel: the dispatch footprint is the product's flag)
    want = oracle_guides(cornell_scene, w, h, 3, flags=flags & ~H.PT_FLAG_REF_DISPATCH)
    if flags == H.PT_FLAG_REF_DISPATCH:
        fp = M.footprint_mask(w, h, True)
        want[~fp] = 0                                   # untouched outside the footprint
        assert g[fp].any()
    same_bits(g, want, "guides with flags %d" % flags)
    pt.close()


# ---------------------------------------------------------------- the filter
def check_filter(pt, what, ref_dispatch=False, **params):
    """The device result against the host twin and the numpy model on the tracer's own inputs."""
    w, h = pt.width, pt.height
    info = pt.denoise(**params)
    got, img, g = pt.read_denoised(), pt.read_rgba32f(), pt.read_guides()
    var = None
    if info["guided"]:
        mom, n = pt.read_moments()
        assert n == info["frames"] >= 2
        var = M.variance_of(mom, n)
    fp = M.footprint_mask(w, h, True) if ref_dispatch else None
    same_bits(got, H.denoise_host(img, var, g, fp, **params), what + ": device against the host twin")
    same_bits(got, M.denoise(img, var, g, fp, **params), what + ": device against the numpy model")
    assert info["iterations"] == params.get("iterations", 5)
    return info, got, img


@pytest.mark.parametrize("w,h", [(61, 37), (200, 120)])
@pytest.mark.parametrize("iterations", [1, 5, 8])
def test_filter_guided(cornell_scene, w, h, iterations):
    """61 x 37: one partial block on each edge; 200 x 120: many blocks, steps 1..16 cross their
    boundaries, and steps 32..128 take the direct loads."""
    pt = tracer(cornell_scene, w, h, moments=True)
    pt.render(1, 8, 0)
    info, got, img = check_filter(pt, "%dx%d, %d iterations" % (w, h, iterations), iterations=iterations)
    assert info["guided"] and info["frames"] == 8
    assert not np.array_equal(got[..., :3], img[..., :3])
    same_bits(got[..., 3], img[..., 3], "alpha")
    same_bits(pt.read_denoised_rgba8(), H.aces_rgba8_host(got), "ACES view of the result")
    pt.close()


@pytest.mark.parametrize("moments,frames", [(False, 8), (True, 1)])
def test_filter_unguided(cornell_scene, moments, frames):
    pt = tracer(cornell_scene, 61, 37, moments=moments)
    pt.render(1, frames, 0)
    info, got, img = check_filter(pt, "unguided")
    assert not info["guided"] and info["frames"] == (frames if moments else 0)
    pt.close()


def test_filter_sigmas_off(cornell_scene):
    pt = tracer(cornell_scene, 61, 37, moments=True)
    pt.render(1, 4, 0)
    check_filter(pt, "all factors off", iterations=3, sigma_lum=0.0, sigma_normal=0.0, sigma_albedo=-1.0,
                 sigma_depth=float("nan"))
    check_filter(pt, "other sigmas", iterations=4, sigma_lum=2.0, sigma_normal=0.5, sigma_albedo=0.3, sigma_depth=1.0)
    pt.close()


@pytest.mark.parametrize("w,h", [(61, 37), (200, 120)])
def test_filter_bad_pixels(cornell_scene, w, h):
    """An image seeded through write_rgba32f with NaN, inf and 1e30 pixels, corners among them."""
    pt = tracer(cornell_scene, w, h, moments=True)
    pt.render(1, 6, 0)
    img = pt.read_rgba32f()
    img[0, 0, 0] = np.nan
    img[h - 1, w - 1, 2] = np.inf
    img[h // 2, w // 3, 1] = np.nan
    img[h // 3, w - 1, :3] = f32(1e30)
    img[5, 7, :3] = f32(1e30)
    pt.write_rgba32f(img)
    info, got, _ = check_filter(pt, "bad pixels")
    assert info["guided"]
    assert np.isfinite(got).all()
    pt.close()


def test_filter_ref_dispatch(cornell_scene):
    w, h = 61, 37
    pt = tracer(cornell_scene, w, h, moments=True, flags=H.PT_FLAG_REF_DISPATCH)
    seed = np.full((h, w, 4), f32(0.25))
    pt.write_rgba32f(seed)                              # pixels outside the footprint keep this
    pt.render(1, 5, 0)
    info, got, img = check_filter(pt, "REF_DISPATCH footprint", ref_dispatch=True)
    fp = M.footprint_mask(w, h, True)
    same_bits(got[~fp], seed[~fp], "outside the footprint")
    assert info["guided"]
    pt.close()


def test_filter_after_adaptive_run(cornell_scene):
    """A restarting adaptive call, batches of 4, a target that retires some tiles and not others:
    the variance uses each tile's own frame count."""
    w, h = 64, 48
    pt = tracer(cornell_scene, w, h)
    done, stats = pt.render_adaptive(0.25, batch=4, max_frames=24)
    frames = pt.tile_frames()
    assert len(np.unique(frames)) >= 3 and stats["tiles_active"] >= 1, np.unique(frames)
    info = pt.denoise()
    assert info["guided"] and info["frames"] == done == frames.max()
    got, img, g = pt.read_denoised(), pt.read_rgba32f(), pt.read_guides()
    mom, _ = pt.read_moments()
    var = M.variance_of(mom, M.pixel_counts(frames, w, h))
    same_bits(got, M.denoise(img, var, g), "after an adaptive run: device against the numpy model")
    same_bits(got, H.denoise_host(img, var, g), "after an adaptive run: device against the host twin")
    uniform = M.denoise(img, M.variance_of(mom, done), g)
    assert not np.array_equal(uniform, got)             # one count for all tiles is another image
    pt.close()


# ---------------------------------------------------------------- invisibility
def test_denoise_is_invisible(cornell_scene):
    """Two tracers, one render sequence -- a long launch, short overlapped launches, a progressive
    replay -- and one of them denoises between the steps.  64 x 48: 48 tiles, one wave of the sort,
    so the tile order is the same from run to run."""
    w, h = 64, 48
    plain, den = tracer(cornell_scene, w, h, moments=True), tracer(cornell_scene, w, h, moments=True)

    def state(pt):
        mom, n = pt.read_moments()
        to = pt.tile_order()
        return dict(image=pt.read_rgba32f(), moments=mom, frames=n, sorts=to["sorts"], perm=to["perm"],
                    grid=(to["n_tiles"], to["tiles_x"]), launches=pt.launches(), sweep=pt.leaf_sweep(),
                    pooled=pt.pooled(), n_timed=pt.timing()[1], rgba8=pt.read_rgba8())

    def same(step):
        a, b = state(plain), state(den)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (step, k)
            else:
                assert a[k] == b[k], (step, k, a[k], b[k])

    def denoise(**kw):
        den.denoise(**kw)
        assert np.isfinite(den.read_denoised()).all()

    for pt in (plain, den):
        pt.render(1, 40, 0)
    denoise()
    same("a long launch")
    for pt in (plain, den):
        for f in range(41, 49):
            pt.render_async(f, 1, 1)
            if pt is den and f == 44:
                pt.denoise(sync=False, guide_frames=2)   # between launches in flight
        pt.sync()
    denoise(iterations=3)
    same("short overlapped launches")
    assert_bitwise(plain.read_rgba32f(), O.render(cornell_scene, w, h, max_bounce=B, n_frames=48), "48 frames")
    for pt in (plain, den):
        pt.progressive_setup(2, 2)
    denoise(guide_frames=1)                              # the captured graph stays
    for pt in (plain, den):
        pt.progressive_run(1)
    denoise()
    for pt in (plain, den):
        pt.progressive_run(1)
    same("a progressive replay")
    for pt in (plain, den):
        pt.render(9, 20, 1)
    denoise()
    same("a later render")
    assert_bitwise(plain.read_rgba32f(), O.render(cornell_scene, w, h, max_bounce=B, n_frames=28), "the final image")
    plain.close()
    den.close()


# ---------------------------------------------------------------- errors
def test_errors(cornell_scene):
    w, h = 32, 24
    pt = H.PathTracer(w, h, max_bounce=B)
    with pytest.raises(H.PTError) as e:
        pt.denoise()
    assert e.value.code == -6                           # PT_E_STATE: before an upload
    pt.upload(cornell_scene)
    pt.render(1, 1, 0)
    for read in (pt.read_denoised, pt.read_denoised_rgba8, pt.read_guides):
        with pytest.raises(H.PTError) as e:
            read()
        assert e.value.code == -6, read                 # ... a read before a denoise
    for bad in (dict(iterations=0), dict(iterations=9), dict(guide_frames=0), dict(guide_frames=-3)):
        with pytest.raises(H.PTError) as e:
            pt.denoise(**bad)
        assert e.value.code == -1, bad                  # PT_E_ARG
    pt.denoise()
    small = np.zeros(w * h * 4 - 1, f32)
    L = H.lib()
    assert L.pt_read_denoised_rgba32f(pt.h, small.ctypes.data, small.nbytes) == -1
    assert L.pt_read_denoised_rgba8_aces(pt.h, small.ctypes.data, w * h * 4 - 1) == -1
    assert L.pt_read_guides(pt.h, small.ctypes.data, w * h * 32 - 4) == -1
    assert L.pt_denoise(None, None, None) == -1
    assert L.pt_denoise(pt.h, None, None) == 0          # NULL parameters = the defaults, info optional
    pt.close()
    split = H.PathTracer(w, h, max_bounce=B, rank=1, world=2)
    split.upload(cornell_scene)
    split.render(1, 1, 0)
    with pytest.raises(H.PTError) as e:
        split.denoise()
    assert e.value.code == -6                           # a row-split context
    split.close()


# ---------------------------------------------------------------- the command line
@pytest.mark.parametrize("how", ["spp", "noise-target", "adaptive"])
def test_cli_denoise(tmp_path, how):
    obj, mtl = pt_scenes.write_scene("cornell", str(tmp_path))
    w, h = 64, 48
    run = {"spp": ["--spp", "5", "--chunk", "2"],
           "noise-target": ["--noise-target", "0.01", "--batch", "4", "--max-spp", "8"],
           "adaptive": ["--noise-target", "0.25", "--adaptive", "--batch", "4", "--max-spp", "16"]}[how]
    dpfm = str(tmp_path / "den.pfm")
    out = subprocess.run([EXE, obj, mtl, "--width", str(w), "--height", str(h), "--bounces", "8", *run, "--denoise",
                          "--denoise-iters", "4", "--guide-frames", "2", "--denoise-pfm", dpfm, "--json",
                          "--pfm", str(tmp_path / "out.pfm"), "--ppm", str(tmp_path / "out.ppm")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    pt = tracer(H.setupBuffers(obj, mtl), w, h)
    if how == "spp":
        pt.render(1, 5, 0)
    elif how == "noise-target":
        pt.render_until(0.01, batch=4, max_frames=8)
    else:
        pt.render_adaptive(0.25, batch=4, max_frames=16)
    info = pt.denoise(iterations=4, guide_frames=2)
    want = pt.read_denoised()
    assert_bitwise(read_pfm(str(tmp_path / "out.pfm")), np.ascontiguousarray(pt.read_rgba32f()[..., :3]), "the image")
    pt.close()
    assert_bitwise(read_pfm(dpfm), np.ascontiguousarray(want[..., :3]), "--denoise-pfm")
    d = line["denoise"]
    assert (d["guided"], d["guides_rendered"], d["iterations"], d["guide_frames"], d["frames"]) == \
        (int(info["guided"]), 1, 4, 2, info["frames"])
    assert d["guided"] == (0 if how == "spp" else 1) and d["ms"] > 0
