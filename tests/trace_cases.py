"""Cameras and ray batches of the traced-ray tests (tests/test_trace_host.py on the CPU against the oracle's renders,
tests/test_gpu_trace.py on the GPU against pt_trace_host).  The scenes are tests/query_cases.py's.

cameras(): seeded cameras placed inside and around a scene's bounds and looking anywhere on the sphere; a direction
within 1e-3 of +-z is rejected, where the reference's `right` = normalize(cross(fwd, z)) is 0/0.  A PT_FLAG_NO_AA
render of such a camera draws no jitter, so its pixel (x, y) at frame f is trace(cam.pos, pixel_ray, seed(x, y, f)):
the oracle's renders judge traced rays of any origin and direction, independently of any product code but
pt_pixel_rays.

ray_batch(): the families a GPU batch holds -- camera rays, an equirectangular panorama from inside the bounds,
shuffled bounce-like rays (from a hit's p into its n hemisphere), axis-parallel rays and rays with |d_i| > 2 (outside
the exact-reciprocal guard), unnormalised d, finite t_max below and above the hit, and a handful with NaN or zero
components.
"""
import numpy as np

import pt_host as H
import query_cases as QC

f32 = np.float32
CW, CH = 4, 3                       # a test camera's image


def cameras(sc, seed, n):
    """n (12,) float32 camera arrays {position.xyzw, direction.xyzw, data.xyzw}."""
    rng = np.random.default_rng(seed)
    lo, hi = QC._bounds(sc)
    out = []
    while len(out) < n:
        inside = len(out) % 2 == 0
        pos = rng.uniform(lo, hi) if inside else rng.uniform(lo - (hi - lo), hi + (hi - lo))
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        if abs(abs(d[2]) - 1.0) < 1e-3 or np.hypot(d[0], d[1]) < 1e-3:
            continue
        cam = np.zeros(12, f32)
        cam[0:3], cam[4:7] = pos, d
        out.append(cam)
    return out


def image_xy(W, Hh):
    ys, xs = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)


def camera_batch(cams, W=CW, Hh=CH):
    """The pixel rays and pixel seeds of every camera's W x H image, camera after camera, rows from the bottom."""
    xy = image_xy(W, Hh)
    rays = np.concatenate([H.pixel_rays(W, Hh, cam, xy) for cam in cams])
    seeds = np.tile(H.pixel_seeds(xy), len(cams))
    return rays, seeds


def with_cam(sc, cam):
    out = dict(sc)
    out["cam"] = cam
    return out


def panorama(origin, W, Hh):
    """Equirectangular directions: column = azimuth, row = elevation, pixel centres."""
    ys, xs = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    phi = (xs.ravel() + 0.5) / W * 2.0 * np.pi
    theta = ((ys.ravel() + 0.5) / Hh - 0.5) * np.pi
    d = np.stack([np.cos(theta) * np.cos(phi), np.cos(theta) * np.sin(phi), np.sin(theta)], 1)
    return H.make_rays(np.tile(np.asarray(origin, f32), (len(d), 1)), d)


def ray_batch(sc, seed, scale=1.0):
    """-> (rays, seeds): about 2,000 * scale rays of the families above, shuffled within the bounce family only (the
    others keep their coherent order, as a caller's would)."""
    rng = np.random.default_rng(seed)
    lo, hi = QC._bounds(sc)
    k = lambda n: max(int(n * scale), 4)
    cast = lambda r: H.intersect_host(sc, r)
    fam = []

    W = max(int(24 * np.sqrt(scale)), 4)
    Hh = max(int(18 * np.sqrt(scale)), 3)
    cam_rays = H.pixel_rays(W, Hh, np.asarray(sc["cam"], f32), image_xy(W, Hh))
    fam.append(cam_rays)
    centre = 0.5 * (lo + hi) + 0.1 * (hi - lo) * rng.uniform(-1, 1, 3)
    fam.append(panorama(centre, W, Hh))

    first = np.concatenate(fam)
    h = cast(first)
    hit = np.nonzero(h["kind"] > 0)[0]
    if hit.size:
        src = hit[rng.integers(0, hit.size, k(500))]
        u = rng.standard_normal((len(src), 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        fam.append(H.make_rays(h["p"][src, 0:3], h["n"][src, 0:3] + 0.98 * u))      # shuffled by the draw of src

    n = k(160)
    tgt = rng.uniform(lo, hi, (n, 3))
    d = np.zeros((n, 3))
    ax = rng.integers(0, 3, n)
    d[np.arange(n), ax] = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.5, n)
    two = rng.random(n) < 0.5
    ax2 = (ax + 1 + rng.integers(0, 2, n)) % 3
    d[np.arange(n)[~two], ax2[~two]] = rng.uniform(-1, 1, int((~two).sum()))
    fam.append(H.make_rays(tgt - d * rng.uniform(0.5, 6.0, (n, 1)), d))            # axis-parallel

    n = k(240)
    o = rng.uniform(lo - (hi - lo), hi + (hi - lo), (n, 3))
    d = rng.uniform(lo, hi, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    big = d * rng.uniform(2.5 * np.sqrt(3.0), 9.0, (n, 1))                          # some |d_i| > 2: outside the guard
    small = d * rng.uniform(0.05, 0.6, (n, 1))                                      # unnormalised, short
    fam.append(H.make_rays(o, np.where(rng.random((n, 1)) < 0.5, big, small)))

    if hit.size:
        src = hit[rng.integers(0, hit.size, k(120))]
        t = h["t"][src]
        for tm in (t * f32(0.5), t * f32(2.0), np.nextafter(t, f32(np.inf)), t):
            r = first[src].copy()
            r["t_max"] = tm
            fam.append(r)

    n = 24
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.standard_normal((n, 3))
    d[0:6] = 0.0
    d[6:12, rng.integers(0, 3)] = np.nan
    d[12:16] = np.nan
    o[16:20, 1] = np.nan
    d[20:22] = [np.inf, 1.0, -1.0]
    o[22:24] = np.inf
    fam.append(H.make_rays(o, d))

    rays = np.concatenate(fam)
    seeds = rng.integers(0, 1 << 32, len(rays), dtype=np.uint64).astype(np.uint32)
    return rays, seeds


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1, 4)


def same_device(got, want, what):
    """`same` between a device result and a host result.  Every word that is a number must be equal, and a NaN must
    stand where a NaN stands; which NaN is not compared.  IEEE 754 (2019, §6.2) leaves the sign and payload of a NaN
    that an invalid operation makes, or that an operation passes on, to the implementation: the host's SSE units make
    0xffc00000 and pass the first operand's payload on, gfx950 makes 0x7fc00000.  Only rays that are themselves NaN,
    infinite or zero reach one (ray_batch's last family), and the callers check that these are few."""
    canon = lambda a: np.where(np.isnan(np.asarray(a, np.float32)), np.float32(np.nan), np.asarray(a, np.float32))
    same(canon(got), canon(want), what)


def same(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero(np.any(g != w, axis=1))[0]
    assert bad.size == 0, "%s: %d of %d RGBA records differ, first at ray %d: got %s, want %s" % (
        what, bad.size, len(w), bad[0], np.asarray(got).reshape(-1, 4)[bad[0]], np.asarray(want).reshape(-1, 4)[bad[0]])
