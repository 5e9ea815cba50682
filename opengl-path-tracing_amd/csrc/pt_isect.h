// pt_isect.h -- the per-ray arithmetic of the render kernels (box tests, triangle tests, the
// running mean, the tonemap), host- and device-callable like pt_math.h: the kernels of
// pt_render.hip run these functions, and tests/isect/isect_check.cpp and the CPU walk models
// (tests/wide/wide_sim.cpp, tests/cull/window_cull_sim.cpp) run the same source on the host.
// Everything they call (pt_math.h, pt_cull.h, pt_wide.h) is pinned the same way.
// Templated on the 16-byte quad type: the kernels pass float4, a host build ptp::Quad
// (pt_scene_pack.h) -- any struct with float members x, y, z, w.
#pragma once

#include "pt_cull.h"
#include "pt_math.h"

namespace pti {

using pt::f3;
using pt::mk;

// ------------------------------------------------------------------ intersection
// bvh_intersect (computeShader.c:309-365): the exact division/compare chain; NaN compares
// are false, which decides axis-parallel rays and zero-thickness boxes.
// (A, B) is the axis-paired node record: A = {min.x, max.x, min.y, max.y}, B = {min.z, max.z, ..}.
template <class Q>
PT_HD bool slab(Q A, Q B, f3 o, f3 d, float cur_t) {
    float tmin = (A.x - o.x) / d.x;
    float tmax = (A.y - o.x) / d.x;
    if (tmin > tmax) { float q = tmin; tmin = tmax; tmax = q; }
    float tymin = (A.z - o.y) / d.y;
    float tymax = (A.w - o.y) / d.y;
    if (tymin > tymax) { float q = tymin; tymin = tymax; tymax = q; }
    if ((tmin > tymax) || (tymin > tmax)) return false;
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    float tzmin = (B.x - o.z) / d.z;
    float tzmax = (B.y - o.z) / d.z;
    if (tzmin > tzmax) { float q = tzmin; tzmin = tzmax; tzmax = q; }
    if ((tmin > tzmax) || (tzmin > tmax)) return false;
    if (tzmin > tmin) tmin = tzmin;
    return !(tmin > cur_t);
}

// A ray with a NaN component in o or d can never hit: every triangle distance
// -(dot(n,o)+d0)/dot(n,d) and every sphere root is NaN, and NaN fails the `t < tbest` /
// `ht > 0.0001` acceptance tests (:297, :378, :411-428).  Its walk still visits up to every
// node -- a single lane crawling the whole tree (60-70 ms on the 69k-triangle stand-in,
// the tail of its launch) -- so the render kernels skip the walk; its result (no hit, t =
// +inf) is the reference's.  Counting builds still walk, to count the node visits.
PT_HD bool ray_has_nan(f3 o, f3 d) {
    return (o.x != o.x) | (o.y != o.y) | (o.z != o.z) | (d.x != d.x) | (d.y != d.y) | (d.z != d.z);
}

// RayIntersectsTriangle (computeShader.c:228-272), Moller-Trumbore with EPSILON 1e-7: the
// opt-in PT_FLAG_MOLLER_TRUMBORE mode (dead code in the reference, which runs hit_triangle).
// The same operations as the oracle's mt_triangle, evaluated branch-free (the early returns
// become a select); 1/a by the guarded exact reciprocal.  -1 for a miss.  The normal it
// would return, normalize(cross(v1-v0, v2-v0)), is the stored per-triangle n.
template <class Q>
PT_HD float tri_mt(Q q0, Q q1, Q q2, f3 o, f3 d) {
    const float EPS = 0.0000001f;
    const f3 v0 = mk(q0.x, q0.y, q0.z), v1 = mk(q1.x, q1.y, q1.z), v2 = mk(q2.x, q2.y, q2.z);
    const f3 e1 = v1 - v0, e2 = v2 - v0;
    const f3 h = pt::cross(d, e2);
    const float a = pt::dot(e1, h);
    bool ok = !(a > -EPS && a < EPS);
    const float f = pt::fast_range(__builtin_fabsf(a)) ? pt::rcp_fast(a) : 1.0f / a;
    const f3 s = o - v0;
    const float u = f * pt::dot(s, h);
    ok = ok && !(u < 0.0f || u > 1.0f);
    const f3 q = pt::cross(s, e1);
    const float v = f * pt::dot(d, q);
    ok = ok && !(v < 0.0f || u + v > 1.0f);
    const float t = f * pt::dot(e2, q);
    ok = ok && t > EPS;
    return ok ? t : -1.0f;
}
// :548-551 running mean, per component, no contraction.
template <class Q>
PT_HD Q mkq(float x, float y, float z, float w) {   // make_float4 for any quad type, in its form (a named local:
                                                    // with `return Q{..}` k_accum_frames allocates registers differently)
    Q r{x, y, z, w};
    return r;
}
template <class Q>
PT_HD Q accumulate(Q prev, f3 rgb, int frame, bool acc) {
    if (!acc) return mkq<Q>(rgb.x, rgb.y, rgb.z, 1.0f);
    float ff = (float)frame;
    float w = (ff - 1.0f) / ff;
    return mkq<Q>(prev.x * w + rgb.x / ff, prev.y * w + rgb.y / ff, prev.z * w + rgb.z / ff,
                  prev.w * w + 1.0f / ff);
}

PT_HD float qdiv(float a, float b, float rb) {
    float q = a * rb;
    float r = __builtin_fmaf(-q, b, a);
    return __builtin_fmaf(r, rb, q);
}

// The box tests' "tn <= tf && tn <= t" is evaluated as tn <= min(tf, t):
// one compare instead of two plus a scalar AND of their lane masks, which sat on the walk
// step's dependency chain (vector compare -> scalar AND -> vector select -> next LDS read):
// +1.5..2% on C2.  v_med3(tf, t, -inf) is min(tf, t) for non-NaN operands; inside the
// exact-reciprocal guard every quotient is finite, and t is finite or +inf.
// Scalar on purpose: packed f32 (v_pk_fma_f32) takes two passes on gfx950's SIMD-32, so
// it saves issue slots but no VALU cycles, and its broadcast operand pairs cost registers
// (measured: no gain, spills).  t is compared, not folded into the min3: fminf on a
// loop-carried value costs a canonicalizing v_max.
PT_HD float min_tf_t(float tf, float cur_t) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(tf, cur_t, -__builtin_huge_valf());   // as slab_oct_cons
#else
    return fminf(tf, cur_t);
#endif
}
template <class Q>
PT_HD bool slab_fast(Q A, Q B, f3 o, f3 d, f3 rd, float cur_t) {
    float x0 = qdiv(A.x - o.x, d.x, rd.x), x1 = qdiv(A.y - o.x, d.x, rd.x);
    float y0 = qdiv(A.z - o.y, d.y, rd.y), y1 = qdiv(A.w - o.y, d.y, rd.y);
    float z0 = qdiv(B.x - o.z, d.z, rd.z), z1 = qdiv(B.y - o.z, d.z, rd.z);
    float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    return tn <= min_tf_t(tf, cur_t);
}

// Slab test on an octant image of the LDS walk (WalkLinks): the node's bounds are stored
// near-first for the ray's direction signs, so the per-axis min/max of slab_fast is known
// in advance.  Equal to slab_fast for boxes with min <= max on every axis (checked at upload
// as part of the scene half of the guard): for d_i > 0 RN((min-o)/d) <= RN((max-o)/d) and for
// d_i < 0 the reverse (RN and the subtraction are monotone), so the near quotient IS the
// minimum; values only enter comparisons, where -0 == +0.
template <class Q>
PT_HD bool slab_oct(Q A, Q B, f3 o, f3 d, f3 rd, float cur_t) {
    float xn = qdiv(A.x - o.x, d.x, rd.x), xf = qdiv(A.y - o.x, d.x, rd.x);
    float yn = qdiv(A.z - o.y, d.y, rd.y), yf = qdiv(A.w - o.y, d.y, rd.y);
    float zn = qdiv(B.x - o.z, d.z, rd.z), zf = qdiv(B.y - o.z, d.z, rd.z);
    float tn = fmaxf(fmaxf(xn, yn), zn);
    float tf = fminf(fminf(xf, yf), zf);
    return tn <= min_tf_t(tf, cur_t);
}

// Conservative slab_oct of the culling walk (pt_cull.h has the test, its margins and the lemma of
// the window clause).  Only culling may use it: a node it accepts and the exact
// test rejects is walked in vain, and a leaf reached that way is rejected by the exact test
// of its own box, which the leaf phase runs before a triangle moves t.  (Measured forms:
// RN(b - o) * rd with a relative margin per node +2.2%, fma with a per-node margin +4.7%,
// this one +7.1% on C2 over the exact test.)
// ol / oh: the per-ray addends (ptc::cull_addends); c_lo: the window clause's constant
template <class Q>
PT_HD bool slab_oct_cons(Q A, Q B, f3 rd, f3 ol, f3 oh, float cur_t, float c_lo) {
    return ptc::cull_hit(A.x, A.y, A.z, A.w, B.x, B.y, rd, ol, oh, cur_t, c_lo);
}

// Byte offset of the ray's octant image in the LDS walk: image k = sx | sy << 1 | sz << 2
// holds the nodes with the bounds of each axis whose direction is negative swapped.  Only
// for rays inside the exact-reciprocal guard (d_i != 0, finite); other rays walk image 0
// (the reference order) with the reference slab.
PT_HD int oct_base(f3 d, int img_bytes) {
    const unsigned o = (pt::fbits(d.x) >> 31) | ((pt::fbits(d.y) >> 30) & 2u) |
                       ((pt::fbits(d.z) >> 29) & 4u);
    return (int)o * img_bytes;
}

// hit_triangle split in two for the leaf phase's edge-test compaction: the plane distance
// (:285-297) and the three edge tests at that distance (:299-306), the same operations as
// tri_hit_bf in the same order, so the same bits.
// (The edge tests read their vertices through the kernel's scene view: tri_edges_at, pt_render_sm.h.)
template <class Q>
PT_HD float tri_plane(Q nd, f3 o, f3 d) {    // nd: quad 0 {n, d0}
    const f3 n = mk(nd.x, nd.y, nd.z);
    return -(pt::dot(n, o) + nd.w) / pt::dot(n, d);
}

// The plane-window filter of a leaf pair at a segment's initial t0 ("Round 20"): whether a leaf
// visit of the pair could do more than clear its candidate bit.  The operations of the leaf phase's plane tests
// (leaf_pair_tests, pt_render_sm.h) in their order, so the same bits: the pair's 2-way choice depends on a triangle
// only when its plane distance is in (1e-4, t) for the first or [1e-4, t) for the second; outside both, h1 and h2
// cannot pass win_open and nothing moves.  Both windows only shrink while a segment runs (t never grows, 1e-4 is
// fixed), so a pair outside them at t0 is outside them at every later visit, and dropping its bit at set-up gives
// the same (t, triangle).  NaN and +-inf distances (a zero denominator) fail every compare: outside.
// nda / ndb: quad 0 {n, d0} of the pair's slots s0 / s0 + 1 (the slot's own quad, not the hit triangle's: a coplanar
// pair's two quads may differ in the sign of zero components); cop: the pair's coplanar flag (ndb is not read).
template <class Q>
PT_HD bool pair_in_window(Q nda, Q ndb, bool cop, f3 o, f3 d, float t0) {
    const float ta = tri_plane(nda, o, d);
    const float tb = cop ? ta : tri_plane(ndb, o, d);
    return pt::win_open(ta, t0) | pt::win_closed(tb, t0);
}

// ACES film tonemap (screenQuadFrag.c:12-26) of one pixel -> RGBA8, alpha 255.
// (U4: the kernels' uchar4, or any struct of four unsigned char)
template <class U4, class Q>
PT_HD U4 aces_px(Q v) {
    float c[3] = {v.x, v.y, v.z};
    unsigned char o[3];
    for (int k = 0; k < 3; k++) {
        float x = c[k];
        float tm = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
        tm = tm < 0.0f ? 0.0f : (tm > 1.0f ? 1.0f : tm);
        if (!(tm == tm)) tm = 0.0f;
        o[k] = (unsigned char)(int)(tm * 255.0f + 0.5f);
    }
    return U4{o[0], o[1], o[2], 255};
}

}  // namespace pti
