"""Traced rays on the host (pt_trace_host, pt_pixel_seeds) against the C++ oracle's renders, word for
word: every comparison is of uint32 words, with no tolerance.  No GPU.

Under PT_FLAG_NO_AA the reference draws no jitter, so pixel (x, y) of frame f is trace(cam.pos, pixel_ray,
seed(x, y, f)).  For cameras placed anywhere in a scene (tests/trace_cases.py) the oracle's render of a 4 x 3 image
is therefore an independent yardstick for tracing arbitrary origins and directions: the only product code on the
expected side is pt_pixel_rays, which the oracle's own camera must agree with for the images to match.
pt_trace_host packs the scene with ptp::pack_scene and runs ptt::trace_frames, the device kernel's own per-ray code.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import pt_host as H
import query_cases as QC
import trace_cases as TC

f32 = np.float32
SCENES = ["cornell", "ship", "fuzz24", "fuzz300", "top769", "spheres_only", "tiny300"]
N_CAMS = 32
NO_AA = H.PT_FLAG_NO_AA
FLAGS = [H.PT_FLAG_NO_SKY, H.PT_FLAG_NO_SPHERES, H.PT_FLAG_NO_TRIANGLES, H.PT_FLAG_MOLLER_TRUMBORE]


def oracle_images(sc, cams, **kw):
    """The oracle's NO_AA render of every camera's image, as (n_cams * W * H, 4) in camera_batch's order."""
    flags = kw.pop("flags", 0) | NO_AA
    return np.concatenate([oracle_lib.render(TC.with_cam(sc, cam), TC.CW, TC.CH, flags=flags, **kw).reshape(-1, 4)
                           for cam in cams])


def check_against_oracle(sc, cams, what, max_bounce=5, mode=1, flags=0):
    rays, seeds = TC.camera_batch(cams)
    kw = dict(max_bounce=max_bounce, mode=mode, flags=flags)
    got = H.trace_host(sc, rays, seeds, frame_first=1, n_frames=3, **kw)
    want = oracle_images(sc, cams, n_frames=3, **kw)
    TC.same(got, want, what + ": frames 1..3")
    # not vacuous: the images are not one colour, and the frames are not one sample
    assert len(np.unique(TC.words(want), axis=0)) > 1, what
    # frames 7..8 over a random prior, through the oracle's per-pixel entry
    rng = np.random.default_rng(5)
    prior = rng.random((len(rays), 4)).astype(f32)
    got = H.trace_host(sc, rays, seeds, frame_first=7, n_frames=2, prior=prior, **kw)
    xy = TC.image_xy(TC.CW, TC.CH)
    m = len(xy)
    want = np.concatenate([
        oracle_lib.render_pixels(TC.with_cam(sc, cam), TC.CW, TC.CH, xy[:, 0], xy[:, 1], max_bounce=max_bounce, mode=mode,
                                 frame_first=7, n_frames=2, acc_first=1, prior=prior[i * m:(i + 1) * m],
                                 flags=flags | NO_AA) for i, cam in enumerate(cams)])
    TC.same(got, want, what + ": frames 7..8 over a prior")


@pytest.mark.parametrize("name", SCENES)
def test_trace_host_equals_oracle(name, cornell_scene, ship_scene):
    sc = QC.scene(name, cornell_scene, ship_scene)
    check_against_oracle(sc, TC.cameras(sc, 31, N_CAMS), name)


@pytest.mark.parametrize("max_bounce", [0, 1, 8])
def test_max_bounce(max_bounce, cornell_scene):
    check_against_oracle(cornell_scene, TC.cameras(cornell_scene, 32, N_CAMS), "max_bounce %d" % max_bounce,
                         max_bounce=max_bounce)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_display_modes(mode, cornell_scene):
    check_against_oracle(cornell_scene, TC.cameras(cornell_scene, 33, N_CAMS), "mode %d" % mode, mode=mode)


@pytest.mark.parametrize("flags", FLAGS + [f | NO_AA for f in FLAGS])
def test_context_flags(flags, cornell_scene):
    """NO_AA means nothing to a trace: with and without it the result is the oracle's NO_AA render."""
    check_against_oracle(cornell_scene, TC.cameras(cornell_scene, 34, N_CAMS), "flags %d" % flags, flags=flags)


def test_frames_differ(cornell_scene):
    """The parity above is not that of a constant: frames draw different samples."""
    rays, seeds = TC.camera_batch(TC.cameras(cornell_scene, 31, N_CAMS))
    a = H.trace_host(cornell_scene, rays, seeds, frame_first=1)
    b = H.trace_host(cornell_scene, rays, seeds, frame_first=2)
    assert np.any(TC.words(a) != TC.words(b))


# ---------------------------------------------------------------- definition details
def test_pixel_seeds_are_the_reference_seed():
    rng = np.random.default_rng(1)
    xy = np.concatenate([rng.integers(0, 65536, (200, 2)), [[0, 0], [65535, 65535], [65535, 0], [0, 65535]]]).astype(np.int32)
    seeds = H.pixel_seeds(xy)
    L = oracle_lib.lib()
    for f in (1, 2, 1000, 5970, 2 ** 31 - 1):
        want = np.array([L.oracle_seed(int(x), int(y), f) for x, y in xy], np.uint32)
        got = seeds + np.uint32((f * 719393) & 0xFFFFFFFF)          # uint32 arithmetic wraps
        assert np.array_equal(got, want), f
    assert int(seeds[201]) == (65535 * 831266 + 65535 * 923766) % 2 ** 32     # wraps
    assert H.lib().pt_pixel_seeds(None, 0, None) == 0
    assert H.lib().pt_pixel_seeds(None, 1, seeds.ctypes.data) == -1
    assert H.lib().pt_pixel_seeds(xy.ctypes.data, 1, None) == -1
    assert H.lib().pt_pixel_seeds(xy.ctypes.data, -1, seeds.ctypes.data) == -1


def test_default_seeds_are_those_of_row_zero(cornell_scene):
    rays, _ = TC.camera_batch(TC.cameras(cornell_scene, 35, 8))
    xy = np.stack([np.arange(len(rays)), np.zeros(len(rays))], 1).astype(np.int32)
    TC.same(H.trace_host(cornell_scene, rays, None, n_frames=2),
            H.trace_host(cornell_scene, rays, H.pixel_seeds(xy), n_frames=2), "seeds=None")


def test_t_max_below_the_hit_is_the_sky(cornell_scene):
    rays, seeds = TC.camera_batch(TC.cameras(cornell_scene, 36, N_CAMS))
    h = H.intersect_host(cornell_scene, rays)
    hit = h["kind"] > 0
    assert hit.sum() > 50
    short = rays[hit].copy()
    short["t_max"] = h["t"][hit] * f32(0.5)
    got = H.trace_host(cornell_scene, short, seeds[hit], n_frames=2)
    sky = H.trace_host(cornell_scene, rays[hit], seeds[hit], n_frames=2,
                       flags=H.PT_FLAG_NO_SPHERES | H.PT_FLAG_NO_TRIANGLES)
    TC.same(got, sky, "t_max = t / 2")
    assert np.any(TC.words(got) != TC.words(H.trace_host(cornell_scene, rays[hit], seeds[hit], n_frames=2)))


def _host_call(sc, rays, seeds, n, frame_first, n_frames, acc, rgba, flags=0, max_bounce=5, mode=1, nodes=None):
    t, nd, m, s = (np.ascontiguousarray(sc[k], f32) for k in ("tris", "nodes", "mats", "spheres"))
    if nodes is not None:
        nd = nodes
    ptr = lambda a: None if a is None else a.ctypes.data
    return H.lib().pt_trace_host(t.reshape(-1), len(t), nd.reshape(-1), len(nd), m.reshape(-1), len(m), s.reshape(-1),
                                 len(s), flags, max_bounce, mode, ptr(rays), ptr(seeds), n, frame_first, n_frames, acc,
                                 ptr(rgba))


def test_overwriting_first_frame_never_reads_the_output(cornell_scene):
    rays, seeds = TC.camera_batch(TC.cameras(cornell_scene, 37, 8))
    nan = np.full((len(rays), 4), np.nan, f32)
    zero = np.zeros((len(rays), 4), f32)
    for out in (nan, zero):
        assert _host_call(cornell_scene, rays, seeds, len(rays), 1, 3, 0, out) == 0
    assert np.array_equal(nan.view(np.uint32), zero.view(np.uint32)) and not np.isnan(nan).any()
    assert np.all(nan[:, 3] == 1.0)


def test_errors(cornell_scene):
    rays, seeds = TC.camera_batch(TC.cameras(cornell_scene, 38, 1))
    n = len(rays)
    out = np.zeros((n, 4), f32)
    call = lambda *a, **kw: _host_call(cornell_scene, *a, **kw)
    assert call(rays, seeds, n, 1, 1, 0, out) == 0
    assert call(None, seeds, n, 1, 1, 0, out) == -1               # null rays with n > 0
    assert call(rays, seeds, n, 1, 1, 0, None) == -1              # null rgba with n > 0
    assert call(rays, seeds, -1, 1, 1, 0, out) == -1              # n < 0
    assert call(rays, seeds, n, 0, 1, 0, out) == -1               # frame_first < 1
    assert call(rays, seeds, n, -3, 1, 0, out) == -1
    assert call(rays, seeds, n, 1, 0, 0, out) == -1               # n_frames < 1
    assert call(rays, seeds, n, 2 ** 31 - 1, 1, 0, out) == -1     # frame_first + n_frames overflows int
    assert call(rays, seeds, n, 2 ** 30, 2 ** 30, 0, out) == -1
    assert call(rays, seeds, n, 1, 1, 2, out) == -1               # accumulate_first not 0 or 1
    assert call(rays, seeds, n, 1, 1, -1, out) == -1
    assert call(None, None, 0, 1, 1, 0, None) == 0                # n = 0
    assert call(rays, None, n, 1, 1, 0, out) == 0                 # seeds may be null
    assert call(rays, seeds, n, 2 ** 31 - 2, 1, 0, out) == 0      # the last frame an int holds
    assert call(rays, seeds, n, 1, 1, 0, out, flags=64) == -1
    assert call(rays, seeds, n, 1, 1, 0, out, max_bounce=-1) == -1
    assert call(rays, seeds, n, 1, 1, 0, out, mode=0) == -1 and call(rays, seeds, n, 1, 1, 0, out, mode=5) == -1
    # a rejected scene: the packer's code
    bad = np.array(cornell_scene["nodes"], f32)
    bad[0, 11] = 0.0                                              # the root's miss link back to the root: a cycle
    assert call(rays, seeds, n, 1, 1, 0, out, nodes=bad) == -4
    bad = np.array(cornell_scene["nodes"], f32)
    bad[3, 10] = np.nan
    assert call(rays, seeds, n, 1, 1, 0, out, nodes=bad) == -4
