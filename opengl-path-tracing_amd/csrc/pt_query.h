// pt_query.h -- the ray query (include/pt_api.h: pt_intersect, pt_intersect_host, pt_pixel_rays): one
// ray against the packed scene, shared by the device kernel (pt_query_kernels.hip) and the host twin (pt_query.cpp), so
// the CPU suite checks the very per-ray code the GPU runs -- the idiom of pt_denoise.h.
//
// The result is the reference's calculateRayCollision (computeShader.c:367-432) with t starting at the ray's t_max
// instead of 1./0.: the spheres in index order (:372-385), then the stackless link walk from node 0 with bvh_intersect
// at the current t (:393-431) and the 2-way choice at every hit leaf (:411-428).  Any-hit stops at the first
// acceptance in that same order.  Nothing is special-cased: a NaN or too-small t_max, NaN or zero ray components and
// an origin inside a sphere fall out of the IEEE arithmetic as they do in the reference.
//
// Built on the pinned pieces (pt_isect.h, pt_math.h): pti::slab outside the exact-reciprocal guard and
// pti::slab_fast with rd = RN(1/d) inside it (equal verdicts there: tests/isect/isect_check.cpp), pti::tri_plane on
// the stored plane quad, pti::tri_mt in Moller-Trumbore mode.  Templated on the 16-byte quad type Q and on a scene
// accessor S over the packed buffers (ptp::SceneBuf):
//   int  n_nodes() / n_spheres();  bool scene_fast()        the scene's facts
//   void node(int i, Q& lo, Q& hi)                          kNodes, record i (axis-paired, top numbering)
//   Q    tri(int slot, int k)                               kTris, quad k of triangle slot `slot`
//   Q    sphere(int i, int k)                               kSpheres
//   Q    leaf_tris(int pair)                                kLeafTris
#pragma once

#include "pt_isect.h"
#include "pt_math.h"
#include "../../include/pt_api.h"

namespace ptq {

using pt::f3;
using pt::mk;

struct Hit {
    float t;
    int kind, prim, mat;
    f3 n, p;
};

PT_HD int ibits(float f) { return (int)pt::fbits(f); }

// The guard of a query: pti::ray_in_guard, and a t_max that is not a NaN (the caller's; min_tf_t orders numbers only).
// For every other t_max, of either sign, slab and slab_fast agree as for a render's t: it enters both in one last compare.
PT_HD bool ray_in_guard(bool scene_fast, f3 o, f3 d, float t_max) {
    return pti::ray_in_guard(scene_fast, o, d) & (t_max == t_max);
}

// The three edge tests (:299-306) at p with normal n.
// TWIN: tri_edges_at (pt_render_sm.h), whose remark says why the render keeps its own.
template <class Q>
PT_HD bool tri_edges(Q q1, Q q2, Q q3, f3 n, f3 p) {
    const f3 v0 = mk(q1.x, q1.y, q1.z), v1 = mk(q2.x, q2.y, q2.z), v2 = mk(q3.x, q3.y, q3.z);
    const float e0 = pt::dot(n, pt::cross(v1 - v0, p - v0));
    const float e1 = pt::dot(n, pt::cross(v2 - v1, p - v1));
    const float e2 = pt::dot(n, pt::cross(v0 - v2, p - v2));
    return (e0 > 0.0f) & (e1 > 0.0f) & (e2 > 0.0f);
}

// hit_triangle (:274-307) of slot `slot`, with the edge tests only where the leaf's choice can depend on them: the
// first triangle's distance matters only inside (1e-4, t), the second's only inside [1e-4, t) -- outside them -1 and
// the plane distance give the same c1 / c2 below, for every t, NaN included.  `closed`: the second.
template <class Q, class S>
PT_HD float tri_hit(const S& sc, int slot, f3 o, f3 d, float t, bool closed) {
    const Q nd = sc.tri(slot, 0);
    const float tp = pti::tri_plane(nd, o, d);
    const bool need = (closed ? tp >= 0.0001f : tp > 0.0001f) & (tp < t);
    float h = -1.0f;
    if (need) {
        if (tri_edges(sc.tri(slot, 1), sc.tri(slot, 2), sc.tri(slot, 3), mk(nd.x, nd.y, nd.z), o + d * tp)) h = tp;
    }
    return h;
}

template <class Q, class S>
PT_HD Hit cast(const S& sc, f3 o, f3 d, float t_max, int flags, bool any_hit) {
    float t = t_max;
    int kind = PT_HIT_NONE, prim = -1;      // prim: the sphere index, or the triangle's slot
    bool done = false;
    if (!(flags & PT_FLAG_NO_SPHERES)) {
        for (int si = 0; si < sc.n_spheres() && !done; si++) {
            const float ht = pti::sphere_t(sc.sphere(si, 0), o, d);
            if ((ht > 0.0001f) & (ht < t)) {
                t = ht;
                kind = PT_HIT_SPHERE;
                prim = si;
                done = any_hit;
            }
        }
    }
    if (!(flags & PT_FLAG_NO_TRIANGLES) && !done) {
        // the guard's verdict is fixed per ray; under it |d_i| is in [2^-20, 2]: rcp_fast is the exact RN(1/d_i)
        const bool fast = ray_in_guard(sc.scene_fast(), o, d, t_max);
        const f3 rd = fast ? mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z)) : mk(0, 0, 0);
        const bool mt = (flags & PT_FLAG_MOLLER_TRUMBORE) != 0;
        int w = sc.n_nodes() > 0 ? 0 : -1;
        // no step counter: an accepted scene's links are acyclic (pt_scene_pack.cpp, validate)
        while (w >= 0) {
            Q lo, hi;
            sc.node(w, lo, hi);
            const int a = ibits(hi.z), b = ibits(hi.w);   // internal: (hit, miss) links; leaf: (~code, next)
            const bool hb = fast ? pti::slab_fast(lo, hi, o, d, rd, t) : pti::slab(lo, hi, o, d, t);
            int next = hb ? (a >= 0 ? a : b) : b;
            if (hb & (a < 0)) {
                const int s0 = (~a >> 1) & ~1;            // code = pair << 2 | coplanar << 1 | single: slots 2k, 2k + 1
                float h1, h2;
                if (mt) {
                    h1 = pti::tri_mt(sc.tri(s0, 1), sc.tri(s0, 2), sc.tri(s0, 3), o, d);
                    h2 = pti::tri_mt(sc.tri(s0 + 1, 1), sc.tri(s0 + 1, 2), sc.tri(s0 + 1, 3), o, d);
                } else {
                    h1 = tri_hit<Q>(sc, s0, o, d, t, false);
                    h2 = tri_hit<Q>(sc, s0 + 1, o, d, t, true);
                }
                // TWIN: pti::leaf_choice (pt_isect.h), kept written out in this association
                const bool c1 = (h1 > 0.0001f) & (h1 < t) & ((h1 < h2) | (h2 < 0.0001f));
                const bool c2 = !c1 & (h2 > 0.0001f) & (h2 < t);
                if (c1 | c2) {
                    t = c1 ? h1 : h2;
                    kind = PT_HIT_TRIANGLE;
                    prim = s0 + (c1 ? 0 : 1);
                    if (any_hit) next = -1;
                }
            }
            w = next;
        }
    }
    // the hit record (:376-383, :413-427): the normal flipped against d, p = o + t*d rounded as hitPoint is
    Hit h = {__builtin_huge_valf(), PT_HIT_NONE, -1, -1, mk(0, 0, 0), mk(0, 0, 0)};
    if (kind != PT_HIT_NONE) {
        const f3 p = o + d * t;
        f3 n;
        if (kind == PT_HIT_SPHERE) {
            const Q s0 = sc.sphere(prim, 0);
            n = pt::normalize(p - mk(s0.x, s0.y, s0.z));
            h.mat = ibits(sc.sphere(prim, 1).x);
            h.prim = prim;
        } else {
            const Q nq = sc.tri(prim, 0);
            n = mk(nq.x, nq.y, nq.z);
            h.mat = ibits(sc.tri(prim, 2).w);
            const Q lt = sc.leaf_tris(prim >> 1);
            h.prim = ibits((prim & 1) ? lt.y : lt.x);
        }
        if (pt::dot(n, d) > 0.0f) n = n * -1.0f;
        h.t = t;
        h.kind = kind;
        h.n = n;
        h.p = p;
    }
    return h;
}

// The camera ray of pixel (x, y) as a render with PT_FLAG_NO_AA forms it (:536-540), from pti::camera_basis's basis.
inline void pixel_ray(const float basis[12], int W, int H, int x, int y, pt_ray* r) {
    const float fW = (float)W, fH = (float)H, rW = 1.0f / fW, rH = 1.0f / fH;
    const f3 pos = mk(basis[0], basis[1], basis[2]), fwd = mk(basis[3], basis[4], basis[5]);
    const f3 right = mk(basis[6], basis[7], basis[8]), up = mk(basis[9], basis[10], basis[11]);
    const float u = pti::film_coord((float)x + 0.0f, fW, rW);
    const float v = pti::film_coord((float)y + 0.0f, fH, rH);
    const f3 d = pt::normalize(pti::pinhole_dir(fwd, right, up, u, v));
    r->o[0] = pos.x, r->o[1] = pos.y, r->o[2] = pos.z, r->t_max = __builtin_huge_valf();
    r->d[0] = d.x, r->d[1] = d.y, r->d[2] = d.z, r->pad = 0.0f;
}

}  // namespace ptq
