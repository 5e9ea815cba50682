// pt_isect.h -- the per-ray arithmetic of the render kernels (box tests, the guard, sphere and triangle
// tests, the leaf's choice, the camera ray, the sky and the bounce, the running mean, the tonemap),
// host- and device-callable like pt_math.h: the kernels of pt_render.hip and the ray-batch units
// (pt_query.h, pt_trace.h, pt_camera.h, pt_film.h, with their host twins) run these functions, and
// tests/isect/isect_check.cpp, the device twin (tests/device) and the CPU walk models
// (tests/wide/wide_sim.cpp, tests/cull/window_cull_sim.cpp) run the same source on the host.
// What the render still restates, and the compiler output that keeps it there: DESIGN.md §17.
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
// one component: prev * ((ff - 1) / ff) + s / ff with ff = (float)frame
PT_HD float accumulate_1(float prev, float s, float ff) {
    float w = (ff - 1.0f) / ff;
    return prev * w + s / ff;
}
template <class Q>
PT_HD Q accumulate(Q prev, f3 rgb, int frame, bool acc) {
    if (!acc) return mkq<Q>(rgb.x, rgb.y, rgb.z, 1.0f);
    float ff = (float)frame;
    return mkq<Q>(accumulate_1(prev.x, rgb.x, ff), accumulate_1(prev.y, rgb.y, ff), accumulate_1(prev.z, rgb.z, ff),
                  accumulate_1(prev.w, 1.0f, ff));
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

// The ray half of the exact-reciprocal guard with the scene half (ptp::SceneFacts::scene_fast): every origin component 0
// or in [2^-40, 2^60], every direction component in [2^-20, 2] (NaN fails).  No short-circuit: each && was an exec-mask
// branch.  ref::in_guard (tests/ref_walk.h) is the reference of its device-twin family.
PT_HD bool ray_in_guard(bool scene_fast, f3 o, f3 d) {
    return scene_fast & pt::in_guard(o.x, 0x1p-40f, 0x1p60f) & pt::in_guard(o.y, 0x1p-40f, 0x1p60f) &
           pt::in_guard(o.z, 0x1p-40f, 0x1p60f) & pt::in_range_abs(d.x, 0x1p-20f, 2.0f) &
           pt::in_range_abs(d.y, 0x1p-20f, 2.0f) & pt::in_range_abs(d.z, 0x1p-20f, 2.0f);
}

// hit_sphere (computeShader.c:209-226) of the sphere whose quad 0 is s0 = {centre, r^2}: the distance along o + d*t, or
// -1 (the caller keeps the closest in (1e-4, t)).
template <class Q>
PT_HD float sphere_t(Q s0, f3 o, f3 d) {
    f3 oc = o - mk(s0.x, s0.y, s0.z);
    float a = pt::dot(d, d);
    float half_b = pt::dot(oc, d);
    float cq = pt::dot(oc, oc) - s0.w;
    float disc = half_b * half_b - a * cq;
    // the IEEE division sequence, not div_g: its range guard's four compares
    // cost more than the sequence (same quotient; +0.6% on C2, round 5)
    return disc < 0.0f ? -1.0f : (-half_b - pt::sqrt_g(disc)) / a;
}

// A leaf's 2-way choice (:406-429) between its triangles' hits h1, h2 (-1: a miss) against the segment's t.
struct LeafChoice { bool c1, c2; };
PT_HD LeafChoice leaf_choice(float h1, float h2, float t) {
    const bool c1 = pt::win_open(h1, t) & ((h1 < h2) | (h2 < 0.0001f));
    const bool c2 = !c1 & pt::win_open(h2, t);
    const LeafChoice r = {c1, c2};
    return r;
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

// ------------------------------------------------------------------ camera and shade
// The camera basis (computeShader.c:519-522): {pos, fwd, right, up} from the camera floats {position.xyzw, direction.xyzw,
// data.xyzw}, once per dispatch on the host in the pinned operations the shader performs per invocation.  Host only.
inline void camera_basis(const float cam[12], int W, int H, float out[12]) {
    const f3 pos = mk(cam[0], cam[1], cam[2]);
    const f3 fwd = pt::normalize(mk(cam[4], cam[5], cam[6]));
    const f3 right = pt::normalize(pt::cross(fwd, mk(0, 0, 1)));
    const f3 up = (pt::normalize(pt::cross(right, fwd)) * (float)H) / (float)W;
    const float v[12] = {pos.x, pos.y, pos.z, fwd.x, fwd.y, fwd.z, right.x, right.y, right.z, up.x, up.y, up.z};
    for (int i = 0; i < 12; i++) out[i] = v[i];
}

// The film coordinate (x + jitter) / W - 0.5 of a pixel (:536-537) by rW = RN(1/W) and a Markstein correction: the
// numerator is 0 or in [2^-32, 2^17), W <= 2^16, so the quotient is correctly rounded (tests/test_exact_div.py).
PT_HD float film_coord(float px, float fW, float rW) { return pt::div_mk(px, fW, rW) - 0.5f; }
// The un-normalised pinhole direction (:539) at film coordinates (u, v).
PT_HD f3 pinhole_dir(f3 fwd, f3 right, f3 up, float u, float v) { return (fwd + right * u) + up * v; }

// The sky of a ray that left the scene (getEnvironmentLight, :131-140), black under PT_FLAG_NO_SKY (`no_sky`).  d by
// reference: by value the camera and film units' kernels commute one add.
PT_HD f3 sky(const f3& d, bool no_sky) {
    f3 env = mk(0, 0, 0);
    if (!no_sky) {
        f3 dir = pt::normalize(d);
        float tt = 0.5f * (dir.z + 1.0f);
        float omt = 1.0f - tt;
        env = mk(omt * 1.0f + tt * 0.5f, omt * 1.0f + tt * 0.7f, omt * 1.0f + tt * 1.0f);
    }
    return env;
}

// The grey of display mode 4 (:461-463) for a hit at hitp seen from o.
PT_HD float depth_term(f3 hitp, f3 o) {
    float s = pt::length(hitp - o);
    float dist = 1.0f - pt::fsqrt(s + 1.0f) / (s + 1.0f);
    return dist * dist;
}

// The two directions of a bounce (:468-471) off a surface with `normal` (flipped against d): the diffuse one takes its
// three normal draws from state, the specular one is reflect(d, normal), both normalised.
PT_HD void bounce_dirs(f3 normal, f3 d, uint32_t& state, f3& diffuse, f3& specular) {
    diffuse = pt::normalize(normal + pt::random_unit_vector(state));
    float kk = 2.0f * pt::dot(normal, d);
    specular = pt::normalize(d - normal * kk);
}

// The rest of the bounce (:483-493, and the loop's bound :447) from the material's quads m0 = {colour, smoothness},
// m1 = {emission, specular probability}, m2 = {specular colour}.  Returns whether the path ended at max_bounce, with its
// colour in rgb.  The quads come by value: read in here, by pointer or accessor, they move the render's assembly (§17).
template <class Q>
PT_HD bool bounce_mix(Q m0, Q m1, Q m2, f3 diffuse, f3 specular, int max_bounce, f3& d, f3& inc, f3& col, uint32_t& state,
                      int& bounce, f3& rgb) {
    float is_spec = (m1.w > pt::random01(state)) ? 1.0f : 0.0f;
    d = pt::mix(diffuse, specular, m0.w * is_spec);
    inc = inc + mk(m1.x, m1.y, m1.z) * col;
    col = col * pt::mix(mk(m0.x, m0.y, m0.z), mk(m2.x, m2.y, m2.z), is_spec);
    bounce++;
    if (bounce > max_bounce) {
        rgb = inc;
        return true;
    }
    return false;
}

// A finished segment that hit a surface (Trace :452-493), from the hit point, the normal already flipped against d and
// the material index: the return of display modes 2, 3 and 4, or the bounce.  Returns whether the path ended, with its
// colour in rgb; otherwise o, d, inc, col, state and bounce are the next segment's.  sc.mat(i, k): quad k of material i.
// TWIN: shade_segment (pt_render_phase.h) restates this dispatch around the same functions.
template <class Q, class S>
PT_HD bool shade_hit(const S& sc, int mat, f3 normal, f3 hitp, int mode, int max_bounce, f3& o, f3& d, f3& inc, f3& col,
                     uint32_t& state, int& bounce, f3& rgb) {
    if (mode == 2) {
        rgb = (normal + mk(1, 1, 1)) * 0.5f;
        return true;
    }
    if (mode == 4) {
        float q = depth_term(hitp, o);
        rgb = mk(q, q, q);
        return true;
    }
    o = hitp;
    f3 diffuse, specular;
    bounce_dirs(normal, d, state, diffuse, specular);
    const Q m0 = sc.mat(mat, 0), m1 = sc.mat(mat, 1), m2 = sc.mat(mat, 2);
    if (mode == 3) {
        rgb = mk(m0.x, m0.y, m0.z);
        return true;
    }
    return bounce_mix(m0, m1, m2, diffuse, specular, max_bounce, d, inc, col, state, bounce, rgb);
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
