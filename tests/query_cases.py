"""Scenes and ray batches of the ray-query tests (tests/test_query_host.py on the CPU against tests/query_model.py,
tests/test_gpu_query.py on the GPU against pt_intersect_host).

Scenes: Cornell, the reference's ship, tests/fuzz_scenes.py cases at 1, 2, 24, 300, 700 and 2,500 triangles (single-
triangle leaves, coplanar pairs, degenerate and duplicated triangles, extra spheres), a far-translated case (coordinates in the
thousands), a case with one coordinate of 1e-14, which fails the scene half of the exact-reciprocal guard so that every
ray takes the IEEE divisions, a spheres-only scene with no node, and trees either side of the 768 node records a
workgroup stages: the builder makes full binary trees over leaf pairs, so node counts are odd -- 767 and 769 are the
nearest on both sides.

Ray families of a batch (ray_batch): camera rays (pt_pixel_rays), uniform random and aimed rays with a share outside
the guard, rays aimed at the spheres, bounce-like rays (origin a previous hit's p, direction in the hemisphere of its
n), axis-parallel rays with one and two zero components, origins inside a sphere, zero and NaN directions and NaN
origins, and the t_max family: t_max at a known hit's t, one ulp either side, 1e-4, 0, negative and NaN.
"""
import numpy as np

import fuzz_scenes
import pt_host as H

f32 = np.float32
FUZZ = {"fuzz1": (908, 1), "fuzz2": (902, 2), "fuzz24": (903, 24), "fuzz300": (904, 300), "fuzz700": (905, 700),
        "fuzz2500": (906, 2500)}
TOP = {"top767": (911, 618), "top769": (911, 621)}      # triangles that give 767 / 769 nodes with this seed
NAMES = ["cornell", "ship"] + list(FUZZ) + ["far300", "tiny300", "spheres_only"] + list(TOP)
GUARDED = ["cornell", "ship", "far300"] + list(FUZZ) + list(TOP)   # scenes inside the scene half of the guard


def scene(name, cornell=None, ship=None):
    if name == "cornell":
        return cornell
    if name == "ship":
        return ship
    if name in FUZZ or name in TOP:
        seed, n = (FUZZ.get(name) or TOP.get(name))
        return fuzz_scenes.random_case(seed, n_tris=n, far=False)[0]
    if name == "far300":
        return fuzz_scenes.random_case(921, n_tris=300, far=True)[0]
    if name == "tiny300":
        sc = fuzz_scenes.random_case(922, n_tris=300, far=False)[0]
        tris = np.array(sc["tris"], f32)
        tris[:, [0, 4, 8]] += f32(50.0)                   # every x positive ...
        tris[0, 0] = 1e-14                                # ... so this one is the root box's min.x, below 2^-40
        out = H.scene_from_arrays(tris, sc["mats"][:sc["n_loaded_mats"]])
        out["spheres"], out["cam"] = np.array(sc["spheres"], f32), np.array(sc["cam"], f32)
        out["spheres"][:, 0] += f32(50.0)
        out["cam"][0] += f32(50.0)
        return out
    if name == "spheres_only":
        mats = np.zeros((2, 16), f32)
        mats[:, 0:3] = [[0.8, 0.2, 0.2], [0.2, 0.8, 0.2]]
        sph = np.array([[0, 0, 0, 1, 0, 0, 0, 0], [1.5, 0.5, 0.2, 0.7, 1, 0, 0, 0], [-2, 1, -0.5, 0.4, 1, 0, 0, 0]], f32)
        cam = np.array([0, -6, 1, 0, 0, 1, 0.1, 0, 0, 0, 0, 0], f32)
        return dict(tris=np.zeros((0, 16), f32), nodes=np.zeros((0, 12), f32), mats=mats, spheres=sph, cam=cam)
    raise KeyError(name)


def _bounds(sc):
    pts = [np.asarray(sc["spheres"], f32).reshape(-1, 8)[:, 0:3]]
    t = np.asarray(sc["tris"], f32).reshape(-1, 16)
    if len(t):
        pts += [t[:, 0:3], t[:, 4:7], t[:, 8:11]]
    p = np.concatenate(pts).astype(np.float64)
    # the soup's bulk, not its 80-unit floor triangles
    lo, hi = np.percentile(p, 5, axis=0), np.percentile(p, 95, axis=0)
    pad = 0.25 * np.maximum(hi - lo, 1.0)
    return lo - pad, hi + pad


def ray_batch(sc, seed, cast, scale=1.0):
    """-> (rays, family index per ray, family names).  `cast(rays)` answers closest-hit queries for the families
    built on earlier hits (the model on the CPU, the host twin on the GPU: the same bits)."""
    rng = np.random.default_rng(seed)
    lo, hi = _bounds(sc)
    tris = np.asarray(sc["tris"], f32).reshape(-1, 16)
    sph = np.asarray(sc["spheres"], f32).reshape(-1, 8)
    cam = np.asarray(sc["cam"], f32)
    k = lambda n: max(int(n * scale), 4)
    fam, names = [], []

    def add(name, o, d, t_max=np.inf):
        names.append(name)
        fam.append(H.make_rays(o, d, t_max))

    def targets(n):
        c = rng.uniform(lo, hi, (n, 3))
        if len(tris):
            t = tris[rng.integers(0, len(tris), n)]
            w = rng.dirichlet([1, 1, 1], n)
            on = w[:, 0:1] * t[:, 0:3] + w[:, 1:2] * t[:, 4:7] + w[:, 2:3] * t[:, 8:11]
            c = np.where(rng.random((n, 1)) < 0.6, on, c)
        return c

    W, Hh = 24, 18
    ys, xs = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    cam_rays = H.pixel_rays(W, Hh, cam, np.stack([xs.ravel(), ys.ravel()], 1))
    names.append("camera")
    fam.append(cam_rays)

    n = k(700)
    o = rng.uniform(lo - (hi - lo), hi + (hi - lo), (n, 3))
    d = targets(n) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.where(rng.random((n, 1)) < 0.3, rng.uniform(2.5, 9.0, (n, 1)), rng.uniform(0.6, 1.4, (n, 1)))   # |d_i| > 2: outside the guard
    away = rng.random(n) < 0.25
    d[away] = rng.standard_normal((int(away.sum()), 3))
    add("random", o, d)

    if len(sph):
        n = k(360)
        s = sph[rng.integers(0, len(sph), n)]
        u = rng.standard_normal((n, 3))
        o = s[:, 0:3] + s[:, 3:4] * rng.uniform(1.2, 3.0, (n, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)   # nearby: few occluders
        d = s[:, 0:3] + 0.9 * s[:, 3:4] * rng.uniform(-1, 1, (n, 3)) / np.sqrt(3.0) - o
        add("to_sphere", o, d / np.linalg.norm(d, axis=1, keepdims=True))
        n = k(40)
        s = sph[rng.integers(0, len(sph), n)]
        add("inside_sphere", s[:, 0:3] + 0.5 * s[:, 3:4] * rng.uniform(-1, 1, (n, 3)) / np.sqrt(3.0),
            rng.standard_normal((n, 3)))

    first = np.concatenate(fam)
    h = cast(first)
    hit = np.nonzero(h["kind"] > 0)[0]
    if hit.size:
        src = hit[rng.integers(0, hit.size, k(400))]
        nn = h["n"][src, 0:3]
        u = rng.standard_normal((len(src), 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        add("bounce", h["p"][src, 0:3], nn + 0.98 * u)

    n = k(240)
    tgt = targets(n)
    d = np.zeros((n, 3))
    ax = rng.integers(0, 3, n)
    d[np.arange(n), ax] = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.5, n)
    two = rng.random(n) < 0.5
    ax2 = (ax + 1 + rng.integers(0, 2, n)) % 3
    d[np.arange(n)[~two], ax2[~two]] = rng.uniform(-1, 1, int((~two).sum()))     # one zero component
    o = tgt - d * rng.uniform(0.5, 6.0, (n, 1))
    snap = rng.random(n) < 0.3                                                    # origins on a box plane's coordinate
    o[snap] = np.round(o[snap])
    add("axis", o, d)

    n = 24
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.standard_normal((n, 3))
    d[0:6] = 0.0
    d[6:12, rng.integers(0, 3)] = np.nan
    d[12:16] = np.nan
    o[16:20, 1] = np.nan
    d[20:22] = [np.inf, 1.0, -1.0]
    o[22:24] = np.inf
    add("zero_nan", o, d)

    if hit.size:
        src = hit[rng.integers(0, hit.size, k(40))]
        t = h["t"][src]
        for nm, tm in (("tmax_at", t), ("tmax_up", np.nextafter(t, f32(np.inf))), ("tmax_down", np.nextafter(t, f32(0))),
                       ("tmax_1e-4", np.full(len(src), 1e-4, f32)), ("tmax_0", np.zeros(len(src), f32)),
                       ("tmax_neg", np.full(len(src), -1.0, f32)), ("tmax_nan", np.full(len(src), np.nan, f32)),
                       ("tmax_half", t * f32(0.5))):
            names.append(nm)
            r = first[src].copy()
            r["t_max"] = tm
            fam.append(r)

    rays = np.concatenate(fam)
    index = np.concatenate([np.full(len(f), i, np.int32) for i, f in enumerate(fam)])
    return rays, index, names
