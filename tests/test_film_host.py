"""The film on the host (pt_api.h: pt_film_expose_host) against compositions of code that was there
before it: the image against pt_trace_camera_host, the moments against numpy binary32 folds of its one-frame colours,
the guides against pt_trace_camera_host in display modes 2, 3 and 4 -- word for word.  Then what the filter does to a
thin-lens Cornell box.  No device is touched: pt_film_expose_host runs the per-pixel code of the device kernel
(csrc/pt_film.h)."""
import numpy as np
import pytest

import camera_cases as CC
import denoise_model as M
import film_cases as FC
import pt_host as H
import query_cases as QC
import trace_cases as TC

f32 = np.float32
W, HH, B, G = 9, 7, 8, 3
# tests/test_camera_host.py's six, and a seventh outside the scene half of the exact-reciprocal guard
SCENES = ["cornell", "ship", "fuzz24", "fuzz300", "top769", "spheres_only", "tiny300"]


def camera_of(sc, model, aa=True):
    return CC.camera(model, W, HH, sc["cam"], aa=aa, aperture=0.1, focus=5.0, ortho_width=6.0)


def tracer_of(sc, flags=0, display_mode=1):
    """-> trace(camera, first, n, mode=None, prior=None): pt_trace_camera_host on the scene."""
    def trace(camera, first, n, mode=None, prior=None):
        return H.trace_camera_host(sc, camera, first, n, prior=prior, flags=flags, max_bounce=B,
                                   mode=display_mode if mode is None else mode)
    return trace


def expose(sc, c, first, n, acc=0, state=None, flags=0, mode=1, guide_frames=G):
    return H.film_expose_host(sc, c, guide_frames, first, n, acc, state=state, flags=flags, max_bounce=B, mode=mode)


def check_planes(film, trace, c, first, n, prior=None, guide_frames=G, what=""):
    """A film exposed (first, n) over `prior` (a film state, or None for a restart) against the compositions."""
    FC.same(film["image"], trace(c, first, n, prior=None if prior is None else prior["image"].reshape(-1, 4)), what + " image")
    colours = [trace(c, f, 1) for f in range(first, first + n)]
    FC.same(film["moments"], FC.fold_moments(colours, None if prior is None else prior["moments"]), what + " moments")
    held = FC.held_after(first, n, 0 if prior is None else prior["guides_held"], guide_frames)
    assert film["guides_held"] == held, what
    if held:
        FC.same(film["guides"], FC.guides_of(trace, c, held), what + " guides")


@pytest.mark.parametrize("name", SCENES)
def test_planes_are_the_compositions(name, cornell_scene, ship_scene):
    sc = QC.scene(name, cornell_scene, ship_scene)
    trace = tracer_of(sc)
    for k, model in enumerate(CC.MODELS):
        c = camera_of(sc, model, aa=k != 2)
        whole = expose(sc, c, 1, 5)
        check_planes(whole, trace, c, 1, 5, what="%s %s frames 1..5" % (name, model))
        assert whole["frames"] == 5 and whole["guides_held"] == G
        assert not np.isnan(whole["guides"]).any() and len(np.unique(FC.words(whole["guides"][..., :7]))) > 2
        # chunk invariance through frames_before / guides_held: 1..2 then 3..5
        a = expose(sc, c, 1, 2)
        assert (a["frames"], a["guides_held"]) == (2, 2)
        check_planes(a, trace, c, 1, 2, what="%s %s frames 1..2" % (name, model))
        b = expose(sc, c, 3, 3, 1, state=a)
        assert (b["frames"], b["guides_held"]) == (5, 3)
        for plane in ("image", "moments", "guides"):
            FC.same(b[plane], whole[plane], "%s %s %s in two chunks" % (name, model, plane))


def test_a_range_without_the_next_guide_frame_leaves_the_guides(cornell_scene):
    sc = cornell_scene
    trace = tracer_of(sc)
    c = camera_of(sc, "thinlens")
    late = expose(sc, c, 5, 2)                                   # frames 5..6 on a new film: frame 1 is not among them
    assert (late["frames"], late["guides_held"]) == (2, 0) and not late["guides"].any()
    check_planes(late, trace, c, 5, 2, what="frames 5..6")
    a = expose(sc, c, 1, 2)
    skipped = expose(sc, c, 4, 2, 1, state=a)                    # holds 1..2; 4..5 does not contain frame 3
    assert skipped["guides_held"] == 2
    FC.same(skipped["guides"], a["guides"], "guides after a range that skips frame 3")
    again = expose(sc, c, 1, 4, 0, state=skipped)                # 1..4 contains frame 3: folds frame 3 only
    assert (again["frames"], again["guides_held"]) == (4, 3)
    FC.same(again["guides"], FC.guides_of(trace, c, 3), "guides completed by a restarting exposure")
    full = expose(sc, c, 7, 3, 1, state=again)                   # complete: nothing moves
    FC.same(full["guides"], again["guides"], "complete guides")
    one = expose(sc, c, 1, 8, guide_frames=1)                    # guide_frames below the range
    assert one["guides_held"] == 1
    FC.same(one["guides"], FC.guides_of(trace, c, 1), "guide_frames = 1")
    many = expose(sc, c, 1, 2, guide_frames=9)                   # ... and above it
    assert many["guides_held"] == 2
    FC.same(many["guides"], FC.guides_of(trace, c, 2), "guide_frames = 9 after two frames")


@pytest.mark.parametrize("flags", [0, H.PT_FLAG_NO_SKY])
def test_sky_and_display_mode(flags, cornell_scene):
    """An equirect camera sees the sky; the context's display mode governs the radiance, never the guides."""
    sc = QC.scene("fuzz24")
    c = camera_of(sc, "equirect")
    for mode in (1, 3):
        film = expose(sc, c, 1, 4, flags=flags, mode=mode)
        trace = tracer_of(sc, flags=flags, display_mode=mode)
        check_planes(film, trace, c, 1, 4, what="flags %d mode %d" % (flags, mode))
    rays = H.camera_rays_host(H.Camera("equirect", W, HH, sc["cam"], aa=False), TC.image_xy(W, HH), 1)[0]
    kinds = H.intersect_host(sc, rays, flags=flags)["kind"]
    assert (kinds == H.PT_HIT_NONE).any() and (kinds != H.PT_HIT_NONE).any()      # misses and hits: both branches


def test_errors(cornell_scene):
    sc = cornell_scene
    c = camera_of(sc, "pinhole")
    for bad in (dict(first=0), dict(n=0), dict(first=2 ** 31 - 1), dict(acc=2), dict(guide_frames=0)):
        with pytest.raises(H.PTError) as e:
            expose(sc, c, **dict(dict(first=1, n=1), **bad))
        assert e.value.code == -1, bad
    with pytest.raises(H.PTError):
        expose(sc, c, 1, 1, state=dict(expose(sc, c, 1, 1), guides_held=G + 1))
    with pytest.raises(H.PTError):
        expose(sc, H.Camera("thinlens", W, HH, sc["cam"], aperture=-1.0), 1, 1)


# ---------------------------------------------------------------- quality through a thin lens
QW, QH = 96, 72


@pytest.fixture(scope="module")
def lens_renders(cornell_scene):
    """Cornell 96 x 72, 8 bounces, aperture 0.1 focused on the rear wall: the 256-frame reference and the films of 4
    and 16 frames, exposed once on the host."""
    sc = cornell_scene
    cam = np.asarray(sc["cam"], f32)
    centre = H.intersect_host(sc, H.camera_rays_host(H.Camera("pinhole", QW, QH, cam, aa=False),
                                                    np.array([[QW // 2, QH // 2]], np.int32), 1)[0])[0]
    assert centre["kind"] != H.PT_HIT_NONE
    focus = float(np.dot((centre["p"][0:3] - cam[0:3]).astype(np.float64), CC.normalize32(cam[4:7]).astype(np.float64)))
    c = CC.camera("thinlens", QW, QH, cam, aperture=0.1, focus=focus)
    ref = H.trace_camera_host(sc, c, 1, 256, max_bounce=8)
    films = {n: H.film_expose_host(sc, c, 4, 1, n, 0, max_bounce=8) for n in (4, 16)}
    return ref, films


@pytest.mark.parametrize("spp", [4, 16])
def test_quality_through_a_thin_lens(lens_renders, spp):
    """relMSE against the 256-frame exposure: the filtered image must be closer than the noisy one (DESIGN.md §15
    records the measured ratios)."""
    ref, films = lens_renders
    film = films[spp]
    assert film["guides_held"] == 4
    out = H.denoise_host(film["image"], M.variance_of(film["moments"], spp), film["guides"])
    noisy, filtered = M.rel_mse(film["image"], ref), M.rel_mse(out, ref)
    print("thin lens, spp %d: noisy relMSE %.4g, filtered %.4g, ratio %.2f" % (spp, noisy, filtered, noisy / filtered))
    assert filtered < noisy
