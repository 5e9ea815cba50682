"""The ray query on the host (pt_intersect_host, pt_pixel_rays) against the numpy model of the
reference (tests/query_model.py), word for word: every comparison is of uint32 words, with no tolerance.  No GPU.

pt_intersect_host packs the scene with ptp::pack_scene and runs ptq::cast, the device kernel's own per-ray code, so
the packer's layouts (kNodes in the top numbering, kTris, kSpheres, kLeafTris) get a CPU consumer here.  The model is
tied to the reference twice: with t_max = +inf its (hit, normal, hit point, material) must equal oracle/numpy_twin.py's
_collide on every test ray, and the hit records of every pixel's camera ray must reproduce the C++ oracle's
display-mode images (normals, albedo, distance; computeShader.c:454-481) under PT_FLAG_NO_AA.
"""
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib
import pt_host as H
import query_cases as QC
import query_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FLAGS = [0, H.PT_FLAG_NO_SPHERES, H.PT_FLAG_NO_TRIANGLES, H.PT_FLAG_MOLLER_TRUMBORE]


def _twin():
    spec = importlib.util.spec_from_file_location("numpy_twin", os.path.join(REPO, "oracle", "numpy_twin.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _words(h):
    return np.ascontiguousarray(h).view(np.uint32).reshape(len(h), 12)


def _same(got, want, what):
    bad = np.nonzero(np.any(_words(got) != _words(want), axis=1))[0]
    assert bad.size == 0, "%s: %d of %d hit records differ, first at ray %d: got %s, want %s" % (
        what, bad.size, len(want), bad[0], got[bad[0]], want[bad[0]])


@pytest.fixture(scope="module")
def twin():
    return _twin()


@pytest.mark.parametrize("name", QC.NAMES)
def test_host_query_equals_model(name, cornell_scene, ship_scene, twin):
    sc = QC.scene(name, cornell_scene, ship_scene)
    scale = 0.6 if name in ("fuzz2500", "fuzz700") else 1.0
    rays, fam, names = QC.ray_batch(sc, 7, lambda r: M.cast(sc, r), scale)
    n = len(rays)
    closest = M.cast(sc, rays)
    anyhit = M.cast(sc, rays, any_hit=True)
    n_tris, n_sph = len(sc["tris"]), len(sc["spheres"])

    # --- the conditions that keep the case from being vacuous, on the model
    kinds = np.bincount(closest["kind"], minlength=3) / n
    print("%s: %d rays, %d nodes, miss / sphere / triangle = %.3f / %.3f / %.3f" % (name, n, len(sc["nodes"]), *kinds))
    assert kinds[0] >= 0.05
    if n_tris:
        assert kinds[2] >= 0.05
    if n_sph:
        assert kinds[1] >= 0.05
    if n_tris > 24:
        differ = np.mean(np.any(_words(closest) != _words(anyhit), axis=1))
        print("  any-hit differs from closest-hit on %.3f" % differ)
        assert differ >= 0.01
    guard = M.in_guard(sc, rays)
    print("  inside the guard: %.3f" % guard.mean())
    if name in QC.GUARDED:
        assert guard.mean() >= 0.10 and (~guard).mean() >= 0.10
    elif len(sc["nodes"]):
        assert not guard.any()          # the scene with a 1e-14 coordinate fails the scene half
    if "tmax_at" in names:
        base = names.index("tmax_at")
        src_kind = closest["kind"][fam == base + 1]           # tmax_up: one ulp above the hit's t keeps it
        flips = sum(int(np.any(closest["kind"][fam == names.index(nm)] != src_kind))
                    for nm in names if nm.startswith("tmax_") and nm != "tmax_up")
        assert np.all(src_kind > 0) and flips >= 1, "the t_max family flips no verdict"

    # --- the model is the reference: numpy_twin's _collide on the rays that start at +inf
    inf = np.nonzero(np.isposinf(rays["t_max"]))[0]
    o = tuple(np.ascontiguousarray(rays["o"][inf, q]) for q in range(3))
    d = tuple(np.ascontiguousarray(rays["d"][inf, q]) for q in range(3))
    with np.errstate(all="ignore"):
        hit, normal, hp, mat = twin._collide(np.asarray(sc["tris"], f32).reshape(-1, 16),
                                             np.asarray(sc["nodes"], f32).reshape(-1, 12),
                                             np.asarray(sc["spheres"], f32).reshape(-1, 8), o, d)
    m = closest[inf]
    assert np.array_equal(hit, m["kind"] > 0)
    for q in range(3):
        assert np.array_equal(np.asarray(normal[q], f32).view(np.uint32)[hit], m["n"][hit, q].view(np.uint32))
        assert np.array_equal(np.asarray(hp[q], f32).view(np.uint32)[hit], m["p"][hit, q].view(np.uint32))
    assert np.array_equal(mat[hit], m["mat"][hit])

    # --- the host twin against the model: closest and any-hit, under each flag
    for flags in FLAGS:
        for any_hit in (False, True):
            want = (anyhit if any_hit else closest) if flags == 0 else M.cast(sc, rays, any_hit, flags)
            _same(H.intersect_host(sc, rays, any_hit, flags), want, "%s flags %d any %d" % (name, flags, any_hit))


def test_top_scenes_straddle_the_staged_nodes(cornell_scene, ship_scene):
    assert len(QC.scene("top767")["nodes"]) == 767 and len(QC.scene("top769")["nodes"]) == 769
    assert len(QC.scene("fuzz2500")["nodes"]) > 4 * 768 and len(QC.scene("spheres_only")["nodes"]) == 0


def _all_pixels(W, Hh):
    ys, xs = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], 1)


@pytest.mark.parametrize("name", ["cornell", "ship"])
def test_pixel_rays_equal_the_twins_camera_rays(name, cornell_scene, ship_scene, twin):
    sc = QC.scene(name, cornell_scene, ship_scene)
    W, Hh = 64, 48
    xy = _all_pixels(W, Hh)
    rays = H.pixel_rays(W, Hh, sc["cam"], xy)
    cam = np.asarray(sc["cam"], f32)
    T = twin
    fwd = T.normalize(tuple(np.full(1, cam[4 + i], f32) for i in range(3)))
    right = T.normalize(T.cross(fwd, (f32(0), f32(0), f32(1))))
    up = tuple(c / f32(W) for c in T.scale(T.normalize(T.cross(right, fwd)), f32(Hh)))
    u = (xy[:, 0].astype(f32) + f32(0)) / f32(W) - f32(0.5)
    v = (xy[:, 1].astype(f32) + f32(0)) / f32(Hh) - f32(0.5)
    d = T.normalize(T.add(T.add(tuple(np.broadcast_to(c, u.shape) for c in fwd), T.scale(right, u)), T.scale(up, v)))
    for q in range(3):
        assert np.array_equal(rays["d"][:, q].view(np.uint32), np.asarray(d[q], f32).view(np.uint32))
        assert np.all(rays["o"][:, q].view(np.uint32) == cam[q:q + 1].view(np.uint32))
    assert np.all(np.isposinf(rays["t_max"])) and np.all(rays["pad"].view(np.uint32) == 0)


@pytest.mark.parametrize("name", ["cornell", "ship"])
def test_hit_records_reproduce_the_oracles_display_modes(name, cornell_scene, ship_scene):
    """computeShader.c:454-481 from the hit records: the normal colour, the albedo, the distance value and the sky."""
    sc = QC.scene(name, cornell_scene, ship_scene)
    W, Hh = 64, 48
    rays = H.pixel_rays(W, Hh, sc["cam"], _all_pixels(W, Hh))
    h = H.intersect_host(sc, rays)
    hit = h["kind"] > 0
    assert 0.05 < hit.mean() < 0.999
    d = rays["d"]
    with np.errstate(all="ignore"):
        # getEnvironmentLight (:131-140) of a miss: incomingLight (0) + env * rayColor (1)
        r = f32(1.0) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        tt = f32(0.5) * (d[:, 2] * r + f32(1.0))
        omt = f32(1.0) - tt
        sky = np.stack([omt * f32(1.0) + tt * f32(c) for c in (0.5, 0.7, 1.0)], 1)
        sky = f32(0.0) + sky * f32(1.0)
        normal_colour = (h["n"][:, 0:3] + f32(1.0)) * f32(0.5)
        albedo = np.asarray(sc["mats"], f32).reshape(-1, 16)[np.maximum(h["mat"], 0), 0:3]
        v = h["p"][:, 0:3] - rays["o"]
        s = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        dist = f32(1.0) - np.sqrt(s + f32(1.0)) / (s + f32(1.0))
        distance = np.repeat((dist * dist)[:, None], 3, 1)
    for mode, colour in ((2, normal_colour), (3, albedo), (4, distance)):
        want = oracle_lib.render(sc, W, Hh, max_bounce=5, mode=mode, n_frames=1, flags=H.PT_FLAG_NO_AA)
        got = np.where(hit[:, None], colour, sky).astype(f32)
        assert np.array_equal(got.view(np.uint32), want.reshape(-1, 4)[:, 0:3].view(np.uint32)), "mode %d" % mode


def test_host_query_errors(cornell_scene):
    sc = cornell_scene
    rays = H.make_rays([[0, -6, 1]], [[0, 1, 0]])
    assert len(H.intersect_host(sc, rays[:0])) == 0
    bad = dict(sc, nodes=np.array(sc["nodes"], f32))
    bad["nodes"][3, 10] = 10 ** 6                         # a link out of range: the packer's error
    with pytest.raises(H.PTError) as e:
        H.intersect_host(bad, rays)
    assert e.value.code == -4                             # PT_E_SCENE
    L = H.lib()
    hits = np.zeros(1, H.HIT_DTYPE)
    t, n, m, s = (np.ascontiguousarray(sc[k], f32).reshape(-1) for k in ("tris", "nodes", "mats", "spheres"))
    args = (t, len(sc["tris"]), n, len(sc["nodes"]), m, len(sc["mats"]), s, len(sc["spheres"]))
    assert L.pt_intersect_host(*args, 0, rays.ctypes.data, 1, hits.ctypes.data, 2) == -1      # unknown query flag
    assert L.pt_intersect_host(*args, 0, None, 1, hits.ctypes.data, 0) == -1                  # null rays
    assert L.pt_intersect_host(*args, 0, None, 0, None, 0) == 0                               # n = 0
    assert L.pt_pixel_rays(0, 4, np.zeros(12, f32), None, 0, None) == -1
