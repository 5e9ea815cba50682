"""The denoising filter on the host (pt_api.h: pt_denoise_host) against the numpy
float32 restatement of its definition (tests/denoise_model.py), bit for bit, and its effect on
oracle renders of the Cornell box.  No device is touched: pt_denoise_host runs the per-tap code
of the device kernel (csrc/pt_denoise.h)."""
import numpy as np
import pytest

import denoise_model as M
import oracle_lib as O
import pt_host as H

f32 = np.float32
SHAPES = [(33, 21), (61, 37)]


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, "%s: %d of %d words differ, first at %s" % (what, len(bad), got.size, bad[0])


def inputs(w, h, seed):
    """A noisy image over piecewise-constant guides with a little noise: edges and flat regions."""
    r = np.random.default_rng(seed)
    region = (np.arange(w)[None, :] * 3 // w) + 3 * (np.arange(h)[:, None] * 2 // h)
    palette = r.random((6, 7)).astype(f32)
    g = np.zeros((h, w, 8), f32)
    g[..., :7] = palette[region] + (r.random((h, w, 7)).astype(f32) - f32(0.5)) * f32(0.02)
    g[..., 3] = g[..., 3] * f32(10)
    img = np.ones((h, w, 4), f32)
    img[..., :3] = palette[region][..., 4:7] + (r.random((h, w, 3)).astype(f32) - f32(0.5)) * f32(0.8)
    img[..., 3] = r.random((h, w)).astype(f32)
    var = (r.random((h, w)).astype(f32) * f32(0.3)) ** 2
    return img, var, g


def both(img, var, g, fp=None, **params):
    got = H.denoise_host(img, var, g, fp, **params)
    want = M.denoise(img, var, g, fp, **params)
    same_bits(got, want, "host twin against the numpy model %r" % (params,))
    assert np.array_equal(got[..., 3].view(np.uint32), img[..., 3].view(np.uint32))
    return got


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("iterations", [1, 5, 7, 8])
@pytest.mark.parametrize("guided", [True, False])
def test_random_images(w, h, iterations, guided):
    img, var, g = inputs(w, h, 7 * w + iterations)
    out = both(img, var if guided else None, g, iterations=iterations)
    assert np.isfinite(out).all()                      # a fully finite input gives a fully finite output
    assert not np.array_equal(out[..., :3], img[..., :3])


def test_far_taps_fall_outside():
    """At iterations 7 and 8 the steps are 64 and 128: every non-centre tap of a 61 x 37 image is
    outside it, so the last iterations change nothing."""
    img, var, g = inputs(61, 37, 3)
    six = both(img, var, g, iterations=6)
    same_bits(both(img, var, g, iterations=8), both(img, var, g, iterations=7), "iterations 8 and 7")
    seven = both(img, var, g, iterations=7)
    # the centre tap alone: c' = (w c) / w, which may round but stays within an ulp or two
    assert np.allclose(seven, six, rtol=1e-6, atol=0)


SIGMAS = ("sigma_lum", "sigma_normal", "sigma_albedo", "sigma_depth")


@pytest.mark.parametrize("off", list(SIGMAS) + ["all", "nan", "negative"])
def test_sigmas_off(off):
    img, var, g = inputs(33, 21, 11)
    if off == "all":
        params = {s: 0.0 for s in SIGMAS}
    elif off == "nan":
        params = dict(sigma_lum=float("nan"), sigma_depth=float("nan"))
    elif off == "negative":
        params = dict(sigma_normal=-1.0)
    else:
        params = {off: 0.0}
    out = both(img, var, g, iterations=3, **params)
    base = both(img, var, g, iterations=3)
    assert not np.array_equal(out, base)               # the factor did something while it was on
    if off == "all":                                   # the plain a-trous kernel: guides and variance do not matter
        g2 = g.copy()
        g2[..., :7] = g2[..., :7] + f32(0.25)          # (a NaN guide would still drop its taps: 0 * NaN)
        same_bits(both(img, var * f32(3), g2, iterations=3, **params), out, "all factors off")


@pytest.mark.parametrize("w,h", SHAPES)
def test_footprint_mask(w, h):
    """The dispatch footprint, cut to multiples of 10: pixels outside are copied through and are
    nobody's tap."""
    img, var, g = inputs(w, h, 5)
    fp = M.footprint_mask(w, h, True)
    assert not fp.all()
    out = both(img, var, g, fp, iterations=5)
    same_bits(out[~fp], img[~fp], "pixels outside the footprint")
    poisoned = img.copy()
    poisoned[~fp, :3] = f32(1e6)
    same_bits(both(poisoned, var, g, fp, iterations=5)[fp], out[fp], "the footprint with other pixels outside it")


@pytest.mark.parametrize("guided", [True, False])
def test_bad_pixels_are_repaired(guided):
    """NaN, +inf and finite-but-huge pixels (1e30: Y or t overflows), a corner among them: they are no
    tap of any neighbour, and take their neighbours' colour."""
    w, h = 33, 21
    img, var, g = inputs(w, h, 9)
    bad = [(0, 0, np.nan), (5, 7, np.inf), (12, 20, np.nan), (32, 10, np.inf)]
    huge = [(20, 4), (32, 20)]
    for x, y, val in bad:
        img[y, x, 1] = val
    for x, y in huge:
        img[y, x, :3] = f32(1e30)
    out = both(img, var if guided else None, g, iterations=5)
    assert np.isfinite(out).all()
    if guided:      # the luminance factor keeps the huge pixels to themselves: the repaired ones look like the image
        for x, y, _ in bad:
            assert abs(out[y, x, :3]).max() < 4.0, (x, y, out[y, x])
    # a huge pixel is usable: with the luminance factor its own weight dwarfs the others (or the taps overflow
    # and drop out); without it, it spreads.  Either way model and twin agree (above).


def test_nan_variance_and_guides():
    w, h = 33, 21
    img, var, g = inputs(w, h, 13)
    var[3, 4] = np.nan
    var[0, 32] = np.inf
    g[10, 10, 0] = np.nan                                  # a NaN normal: every tap of that pixel is dropped
    g[15, 20, 3] = np.nan                                  # a NaN distance
    g[20, 0, 5] = np.inf
    out = both(img, var, g, iterations=4)
    for x, y in ((10, 10), (20, 15), (0, 20)):
        same_bits(out[y, x], img[y, x], "a pixel with NaN guides keeps its input")
    assert np.isfinite(out[3, 4]).all() and np.isfinite(out[0, 32]).all()   # repaired from the neighbours
    assert np.isfinite(out).all()


def test_pixel_without_usable_tap_keeps_its_input():
    """Everything NaN but one pixel: the NaN pixels around it find it (and take its colour) only
    where a tap reaches it; those that never do keep their NaN."""
    w, h = 33, 21
    img, var, g = inputs(w, h, 17)
    keep = img[10, 16].copy()
    img[..., 0] = np.nan
    img[10, 16] = keep
    out = both(img, None, g, iterations=1)
    assert np.isfinite(out[8:13, 14:19]).all()
    far = np.ones((h, w), bool)
    far[8:13, 14:19] = False
    same_bits(out[far], img[far], "pixels no usable tap reaches")
    alone = img.copy()
    alone[10, 16, 0] = np.nan                               # now nothing is usable
    same_bits(both(alone, var, g, iterations=3), alone, "an image without a usable pixel")


def test_arguments():
    img, var, g = inputs(33, 21, 1)
    for bad in (dict(iterations=0), dict(iterations=9), dict(guide_frames=0)):
        with pytest.raises(H.PTError) as e:
            H.denoise_host(img, var, g, **bad)
        assert e.value.code == -1
    p = H.denoise_params()
    assert (p.iterations, p.guide_frames) == (5, 4)
    assert [f32(x) for x in (p.sigma_lum, p.sigma_normal, p.sigma_albedo, p.sigma_depth)] == \
        [f32(8), f32(0.1), f32(0.1), f32(0.05)]
    for n, _ in H.DenoiseParams._fields_:                  # the model's defaults are the library's
        assert f32(M.DEFAULTS[n]) == f32(getattr(p, n)), n


# ---------------------------------------------------------------- quality on oracle renders
QW, QH, QB = 96, 72, 8


@pytest.fixture(scope="module")
def cornell_renders(cornell_scene):
    """Cornell 96 x 72, 8 bounces: the 512-frame reference, frames 1..16 one by one, and the guides
    of 4 frames (display modes 2, 3, 4) -- rendered once by the oracle."""
    sc = cornell_scene
    ref = O.render(sc, QW, QH, max_bounce=QB, n_frames=512)
    frames = [O.render(sc, QW, QH, max_bounce=QB, frame_first=f, n_frames=1, acc_first=0) for f in range(1, 17)]
    modes = [O.render(sc, QW, QH, max_bounce=QB, mode=m, n_frames=4) for m in (2, 3, 4)]
    g = np.zeros((QH, QW, 8), f32)
    g[..., 0:3], g[..., 3], g[..., 4:7] = modes[0][..., :3], modes[2][..., 0], modes[1][..., :3]
    return ref, frames, g


@pytest.mark.parametrize("spp", [1, 4, 16])
def test_quality_on_cornell(cornell_scene, cornell_renders, spp):
    """relMSE against the 512-frame render at most half the unfiltered image's (a floor against a
    broken filter; DESIGN.md §11 records the measured ratios)."""
    ref, frames, g = cornell_renders
    img = O.render(cornell_scene, QW, QH, max_bounce=QB, n_frames=spp)
    var = None
    if spp >= 2:
        s1, s2 = np.zeros((QH, QW), f32), np.zeros((QH, QW), f32)
        for c in frames[:spp]:
            y = M.luminance(c)
            s1 = s1 + y
            s2 = s2 + y * y
        var = M.variance_of(np.stack([s1, s2], -1), spp)
    out = H.denoise_host(img, var, g)
    noisy, filtered = M.rel_mse(img, ref), M.rel_mse(out, ref)
    print("spp %d: noisy relMSE %.4g, filtered %.4g, ratio %.2f" % (spp, noisy, filtered, noisy / filtered))
    assert filtered <= 0.5 * noisy
