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

// The ray half of the exact-reciprocal guard with the scene half (SceneFacts::scene_fast).
// TWIN: seg_in_guard (pt_render_phase.h), a device section of the render translation unit.
// A segment of a render starts at t = +inf; a query's t_max is the caller's, so the guard also asks that it is not a
// NaN (min_tf_t orders numbers only).  For every other t_max, of either sign, slab and slab_fast agree as they do
// for a render's t: t enters both in one last compare.
PT_HD bool ray_in_guard(bool scene_fast, f3 o, f3 d, float t_max) {
    return scene_fast & pt::in_guard(o.x, 0x1p-40f, 0x1p60f) & pt::in_guard(o.y, 0x1p-40f, 0x1p60f) &
           pt::in_guard(o.z, 0x1p-40f, 0x1p60f) & pt::in_range_abs(d.x, 0x1p-20f, 2.0f) &
           pt::in_range_abs(d.y, 0x1p-20f, 2.0f) & pt::in_range_abs(d.z, 0x1p-20f, 2.0f) & (t_max == t_max);
}

// hit_sphere (:209-226): the distance along o + d*t, or -1.
// TWIN: sphere_t (pt_render_phase.h).
template <class Q>
PT_HD float sphere_t(Q s0, f3 o, f3 d) {
    f3 oc = o - mk(s0.x, s0.y, s0.z);
    float a = pt::dot(d, d);
    float half_b = pt::dot(oc, d);
    float cq = pt::dot(oc, oc) - s0.w;
    float disc = half_b * half_b - a * cq;
    return disc < 0.0f ? -1.0f : (-half_b - pt::sqrt_g(disc)) / a;
}

// The three edge tests (:299-306) at p with normal n.
// TWIN: tri_edges_at (pt_render_sm.h).
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
            const float ht = sphere_t(sc.sphere(si, 0), o, d);
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

// The camera basis as pt_set_camera derives it (computeShader.c:519-522): {pos, fwd, right, up} from the 12 camera
// floats {position.xyzw, direction.xyzw, data.xyzw}.
// TWIN: pt_set_camera (pt_render.hip).
inline void camera_basis(const float cam[12], int W, int H, float out[12]) {
    const f3 pos = mk(cam[0], cam[1], cam[2]);
    const f3 fwd = pt::normalize(mk(cam[4], cam[5], cam[6]));
    const f3 right = pt::normalize(pt::cross(fwd, mk(0, 0, 1)));
    const f3 up = (pt::normalize(pt::cross(right, fwd)) * (float)H) / (float)W;
    const float v[12] = {pos.x, pos.y, pos.z, fwd.x, fwd.y, fwd.z, right.x, right.y, right.z, up.x, up.y, up.z};
    for (int i = 0; i < 12; i++) out[i] = v[i];
}

// The camera ray of pixel (x, y) as a render with PT_FLAG_NO_AA forms it (:536-540), from the basis above.
// TWIN: camera_ray (pt_render_phase.h), with zero jitter.
inline void pixel_ray(const float basis[12], int W, int H, int x, int y, pt_ray* r) {
    const float fW = (float)W, fH = (float)H, rW = 1.0f / fW, rH = 1.0f / fH;
    const f3 pos = mk(basis[0], basis[1], basis[2]), fwd = mk(basis[3], basis[4], basis[5]);
    const f3 right = mk(basis[6], basis[7], basis[8]), up = mk(basis[9], basis[10], basis[11]);
    const float u = pt::div_mk((float)x + 0.0f, fW, rW) - 0.5f;
    const float v = pt::div_mk((float)y + 0.0f, fH, rH) - 0.5f;
    const f3 d = pt::normalize((fwd + right * u) + up * v);
    r->o[0] = pos.x, r->o[1] = pos.y, r->o[2] = pos.z, r->t_max = __builtin_huge_valf();
    r->d[0] = d.x, r->d[1] = d.y, r->d[2] = d.z, r->pad = 0.0f;
}

}  // namespace ptq
