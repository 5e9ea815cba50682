"""TEST INFRASTRUCTURE ONLY -- a numpy-float32 model of the ray query, written from the reference
text and sharing no code with the product or with oracle/numpy_twin.py.

A ray's result is computeShader.c's calculateRayCollision (:367-432) with t starting at the ray's t_max instead of
1./0.: hit_sphere (:209-226) over the spheres in index order, accepting 1e-4 < t_s < t; then the link walk from node 0
with bvh_intersect (:309-365) at the current t, and at every hit leaf hit_triangle (:274-307) -- or the Moller-Trumbore
RayIntersectsTriangle (:228-272) -- of both triangles and the 2-way choice of :411-428.  Any-hit stops a ray at its
first acceptance in that same order.  The reference arrays are read as uploaded (std140 records), not packed.

Arithmetic: numpy binary32 array operations are IEEE round-to-nearest without contraction, and '/' and np.sqrt are
correctly rounded -- DESIGN.md §3.2's pinning.  Vectorised over the rays with index sets; nothing is special-cased.
"""
import numpy as np

f32 = np.float32
NO_SPHERES, NO_TRIANGLES, MOLLER_TRUMBORE = 4, 8, 32
HIT = np.dtype([("t", f32), ("kind", np.int32), ("prim", np.int32), ("mat", np.int32), ("n", f32, 4), ("p", f32, 4)])
LOW = f32(0.0001)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _mul(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def _unit(a):
    return _mul(a, f32(1.0) / np.sqrt(_dot(a, a)))


def _verts(tris, idx):
    t = tris[idx]
    return (t[:, 0], t[:, 1], t[:, 2]), (t[:, 4], t[:, 5], t[:, 6]), (t[:, 8], t[:, 9], t[:, 10])


def _normal(v0, v1, v2):
    return _unit(_cross(_sub(v1, v0), _sub(v2, v0)))


def _hit_triangle(tris, idx, o, d):
    """:274-307 -> (distance or -1, normal)"""
    v0, v1, v2 = _verts(tris, idx)
    n = _normal(v0, v1, v2)
    dd = -_dot(n, v0)
    t = -(_dot(n, o) + dd) / _dot(n, d)
    p = _add(o, _mul(d, t))
    inside = ((_dot(n, _cross(_sub(v1, v0), _sub(p, v0))) > 0) & (_dot(n, _cross(_sub(v2, v1), _sub(p, v1))) > 0) &
              (_dot(n, _cross(_sub(v0, v2), _sub(p, v2))) > 0))
    return np.where(t < 0, f32(-1.0), np.where(inside, t, f32(-1.0))).astype(f32), n


def _moller_trumbore(tris, idx, o, d):
    """:228-272 -> (distance or -1, normal)"""
    eps = f32(0.0000001)
    v0, v1, v2 = _verts(tris, idx)
    e1, e2 = _sub(v1, v0), _sub(v2, v0)
    h = _cross(d, e2)
    a = _dot(e1, h)
    out = (a > -eps) & (a < eps)
    f = f32(1.0) / a
    s = _sub(o, v0)
    u = f * _dot(s, h)
    out |= (u < 0) | (u > 1)
    q = _cross(s, e1)
    v = f * _dot(d, q)
    out |= (v < 0) | (u + v > 1)
    t = f * _dot(e2, q)
    out |= ~(t > eps)
    return np.where(out, f32(-1.0), t).astype(f32), _normal(v0, v1, v2)


def _box(nd, o, d, t):
    """:309-365"""
    tmin = (nd[:, 0] - o[0]) / d[0]
    tmax = (nd[:, 4] - o[0]) / d[0]
    s = tmin > tmax
    tmin, tmax = np.where(s, tmax, tmin), np.where(s, tmin, tmax)
    tymin = (nd[:, 1] - o[1]) / d[1]
    tymax = (nd[:, 5] - o[1]) / d[1]
    s = tymin > tymax
    tymin, tymax = np.where(s, tymax, tymin), np.where(s, tymin, tymax)
    miss = (tmin > tymax) | (tymin > tmax)
    tmin = np.where(tymin > tmin, tymin, tmin)
    tmax = np.where(tymax < tmax, tymax, tmax)
    tzmin = (nd[:, 2] - o[2]) / d[2]
    tzmax = (nd[:, 6] - o[2]) / d[2]
    s = tzmin > tzmax
    tzmin, tzmax = np.where(s, tzmax, tzmin), np.where(s, tzmin, tzmax)
    miss |= (tmin > tzmax) | (tzmin > tmax)
    tmin = np.where(tzmin > tmin, tzmin, tmin)
    miss |= tmin > t
    return ~miss


def cast(sc, rays, any_hit=False, flags=0):
    """The hit records (HIT) of `rays` (fields o, t_max, d) against the scene dict `sc`."""
    with np.errstate(all="ignore"):
        return _cast(sc, rays, any_hit, flags)


def _cast(sc, rays, any_hit, flags):
    tris = np.asarray(sc["tris"], f32).reshape(-1, 16)
    nodes = np.asarray(sc["nodes"], f32).reshape(-1, 12)
    sph = np.asarray(sc["spheres"], f32).reshape(-1, 8)
    P = len(rays)
    o = tuple(np.ascontiguousarray(rays["o"][:, i], f32) for i in range(3))
    d = tuple(np.ascontiguousarray(rays["d"][:, i], f32) for i in range(3))
    t = np.array(rays["t_max"], f32)
    kind = np.zeros(P, np.int32)
    prim = np.full(P, -1, np.int32)
    mat = np.full(P, -1, np.int32)
    nrm = [np.zeros(P, f32) for _ in range(3)]
    pnt = [np.zeros(P, f32) for _ in range(3)]
    done = np.zeros(P, bool)

    def accept(idx, th, n, oo, dd, k, pr, mt):
        flip = _dot(n, dd) > 0
        hp = _add(oo, _mul(dd, th))
        for q in range(3):
            nrm[q][idx] = np.where(flip, f32(-1.0) * n[q], n[q])
            pnt[q][idx] = hp[q]
        t[idx], kind[idx], prim[idx], mat[idx] = th, k, pr, mt
        if any_hit:
            done[idx] = True

    if not flags & NO_SPHERES:
        for si, s in enumerate(sph):
            c = (s[0], s[1], s[2])
            oc = _sub(o, c)
            a = _dot(d, d)
            half_b = _dot(oc, d)
            cc = _dot(oc, oc) - s[3] * s[3]
            disc = half_b * half_b - a * cc
            ht = np.where(disc < 0, f32(-1.0), (-half_b - np.sqrt(disc)) / a).astype(f32)
            idx = np.nonzero((ht > LOW) & (ht < t) & ~done)[0]
            if idx.size:
                oo, dd = tuple(x[idx] for x in o), tuple(x[idx] for x in d)
                th = ht[idx]
                n = _unit(_sub(_add(oo, _mul(dd, th)), c))
                accept(idx, th, n, oo, dd, 1, si, int(s[4]))

    if not flags & NO_TRIANGLES and len(nodes):
        test = _moller_trumbore if flags & MOLLER_TRUMBORE else _hit_triangle
        bi = np.where(done, -1, 0).astype(np.int64)
        act = np.nonzero(bi > -1)[0]
        while act.size:
            nd = nodes[bi[act]]
            oo, dd = tuple(x[act] for x in o), tuple(x[act] for x in d)
            hb = _box(nd, oo, dd, t[act])
            nxt = np.where(hb, nd[:, 10], nd[:, 11]).astype(np.int64)
            li = np.nonzero(hb & (nd[:, 8] > -1))[0]
            if li.size:
                g = act[li]
                o2, d2 = tuple(x[li] for x in oo), tuple(x[li] for x in dd)
                i0, i1 = nd[li, 8].astype(np.int64), nd[li, 9].astype(np.int64)
                h1, n1 = test(tris, i0, o2, d2)
                h2, n2 = test(tris, i1, o2, d2)
                tg = t[g]
                c1 = (h1 > LOW) & (h1 < tg) & ((h1 < h2) | (h2 < LOW))
                c2 = ~c1 & (h2 > LOW) & (h2 < tg)
                sel = np.nonzero(c1 | c2)[0]
                if sel.size:
                    first = c1[sel]
                    n = tuple(np.where(first, a_[sel], b_[sel]) for a_, b_ in zip(n1, n2))
                    pr = np.where(first, i0[sel], i1[sel])
                    accept(g[sel], np.where(first, h1[sel], h2[sel]), n, tuple(x[sel] for x in o2),
                           tuple(x[sel] for x in d2), 2, pr, tris[pr, 12].astype(np.int32))
                    if any_hit:
                        nxt[li[sel]] = -1
            bi[act] = nxt
            act = act[nxt > -1]

    out = np.zeros(P, HIT)
    out["t"] = np.where(kind > 0, t, f32(np.inf))
    out["kind"], out["prim"], out["mat"] = kind, prim, mat
    for q in range(3):
        out["n"][:, q] = nrm[q]
        out["p"][:, q] = pnt[q]
    return out


def in_guard(sc, rays):
    """Which rays the exact-reciprocal guard holds: every box coordinate of the scene 0 or of
    magnitude in [2^-40, 2^60] with min <= max, every origin component the same, every direction component of
    magnitude in [2^-20, 2], and a t_max that is a number."""
    nodes = np.asarray(sc["nodes"], f32).reshape(-1, 12)
    with np.errstate(all="ignore"):
        def mag(v, lo, hi, zero):
            a = np.abs(v)
            return ((a >= f32(lo)) & (a <= f32(hi))) | (zero & (v == 0))
        box = nodes[:, [0, 1, 2, 4, 5, 6]]
        scene = bool(np.all(mag(box, 2.0 ** -40, 2.0 ** 60, True)) and np.all(nodes[:, 0:3] <= nodes[:, 4:7]))
        ok = np.all(mag(rays["o"], 2.0 ** -40, 2.0 ** 60, True), 1) & np.all(mag(rays["d"], 2.0 ** -20, 2.0, False), 1)
        return ok & scene & ~np.isnan(rays["t_max"])
