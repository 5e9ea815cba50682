// TEST INFRASTRUCTURE: CPU model of the LDS culling walk with its window clause (pt_cull.h,
// DESIGN.md §5.6) against the reference's binary32 walk (calculateRayCollision,
// computeShader.c:367-432; bvh_intersect :309-365; hit_triangle :274-307; tests/ref_walk.h).  It
// runs the SAME node test, leaf re-test, per-ray addends and window slack the kernel and
// pt_upload_scene use (pti::slab_oct_cons / slab_oct, ptc::cull_addends / window_slack, compiled
// for the host) and fails on
//   (a) a segment whose final t (bitwise) or triangle differs from the reference's,
//   (b) a leaf at which the reference accepts a triangle while the culling test (with the
//       clause) rejects that leaf or one of its ancestors at the t of that moment,
//   (c) a node the reference's exact test accepts and the test without the clause rejects.
// It reports how many of the reference's leaf visits the clause alone removes.
//
// usage: window_cull_sim scene.bin [stride] [bounces] [adversarial_rays]
//   scene.bin: int32 n_tris, n_nodes, n_spheres, then float32 tris (16 per), nodes (12 per),
//   spheres (8 per), camera (12: pos, dir, 0...) -- written by tests/test_window_cull.py.
// Exit status 0 = no violation, 3 = the tree does not qualify for the culling walk.
// Output: one JSON line of statistics.
#include "../../opengl-path-tracing_amd/csrc/pt_cull.h"
#include "../../opengl-path-tracing_amd/csrc/pt_isect.h"
#include "../../opengl-path-tracing_amd/csrc/pt_scene_pack.h"
#include "../ref_walk.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

using pt::f3;
using pt::mk;
using namespace ref;   // the scene and the reference side

namespace {

std::vector<int> parent;
float cm[3], ws[3] = {0, 0, 0};

// the kernel's tests of node i: its bounds near-first for the ray's direction signs (the octant
// images of the LDS walk), with rd = pt::rcp_fast(d) as in the kernel's segment set-up
struct CRay { f3 rd, ol, oh; bool sx, sy, sz; };
CRay make_ray(f3 o, f3 d) {
    CRay r;
    r.rd = mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z));
    ptc::cull_addends(o, r.rd, cm, ws, r.ol, r.oh);
    r.sx = std::signbit(d.x); r.sy = std::signbit(d.y); r.sz = std::signbit(d.z);
    return r;
}
void node_oct(int i, const CRay& r, ptp::Quad& A, ptp::Quad& B) {   // the node's record in the ray's octant image
    const float* b = &nodes[12 * (size_t)i];
    A = {r.sx ? b[4] : b[0], r.sx ? b[0] : b[4], r.sy ? b[5] : b[1], r.sy ? b[1] : b[5]};
    B = {r.sz ? b[6] : b[2], r.sz ? b[2] : b[6], 0.0f, 0.0f};
}
bool node_cull(int i, const CRay& r, float t, float c_lo) {
    ptp::Quad A, B;
    node_oct(i, r, A, B);
    return pti::slab_oct_cons(A, B, r.rd, r.ol, r.oh, t, c_lo);
}
bool node_retest(int i, const CRay& r, f3 o, f3 d, float t) {   // the leaf phase's exact re-test
    ptp::Quad A, B;
    node_oct(i, r, A, B);
    return pti::slab_oct(A, B, o, d, r.rd, t);
}
bool chain_cull(int i, const CRay& r, float t, float c_lo) {   // node i and every ancestor
    for (; i >= 0; i = parent[i])
        if (!node_cull(i, r, t, c_lo)) return false;
    return true;
}

const float kNoWindow = -INFINITY;
float c_lo_on = ptc::kWindowLo;
long window_violations = 0, cons_violations = 0, mismatches = 0, slow = 0, near_hits = 0;
struct Acc { double segs = 0, ref_nodes = 0, ref_leaves = 0, removed = 0, off_nodes = 0, off_leaves = 0, on_nodes = 0, on_leaves = 0; };

typedef RefOut Out;
// The reference walk (tests/ref_walk.h); for guarded rays it also checks (b) / (c) at every node it
// visits and counts the leaf visits the clause alone removes.
Out checked_ref_walk(f3 o, f3 d, float t0, bool guarded, const CRay& cr, Acc& A) {
    return ref_walk(
        o, d, t0,
        [&](int bi, bool hb, float t) {
            if (guarded && hb && !node_cull(bi, cr, t, kNoWindow)) cons_violations++;
        },
        [&](int bi, float t, bool moves, float t2) {
            const bool kept = !guarded || chain_cull(bi, cr, t, c_lo_on);
            if (guarded && !kept && chain_cull(bi, cr, t, kNoWindow)) A.removed++;
            if (!moves) return;
            if (!kept) {
                if (window_violations < 10)
                    std::fprintf(stderr, "WINDOW o=(%a,%a,%a) d=(%a,%a,%a): leaf %d accepts t=%a, culled\n", o.x, o.y,
                                 o.z, d.x, d.y, d.z, bi, t2);
                window_violations++;
            }
            if (t2 < 4e-4f) near_hits++;
        });
}

// The culling walk of the kernel: the conservative test at every node, and at a leaf the
// reference's 2-way choice, whose winner moves t only if the leaf's own box passes the exact
// test (the leaf phase's re-test).
Out cull_walk(f3 o, f3 d, float t0, const CRay& cr, float c_lo) {
    Out r{t0, -1, 0, 0};
    for (int bi = 0; bi > -1;) {
        const float* b = &nodes[12 * (size_t)bi];
        const bool hb = node_cull(bi, cr, r.t, c_lo);
        r.nodes++;
        const int next = hb ? (int)b[10] : (int)b[11];
        if (hb && b[8] > -1.0f) {
            r.leaves++;
            float t2;
            int tri;
            if (leaf_choice(bi, o, d, r.t, t2, tri) && node_retest(bi, cr, o, d, r.t)) { r.t = t2; r.tri = tri; }
        }
        bi = next;
    }
    return r;
}

void segment(f3 o, f3 d, Acc& A, float* t_out, int* tri_out) {
    const float t0 = sphere_t(o, d);
    const bool guarded = pti::ray_in_guard(true, o, d);   // the kernel's own verdict
    CRay cr{};
    if (guarded) cr = make_ray(o, d);
    const Out ro = checked_ref_walk(o, d, t0, guarded, cr, A);
    *t_out = ro.t;
    *tri_out = ro.tri;
    if (!guarded) { slow++; return; }
    A.segs++;
    A.ref_nodes += ro.nodes;
    A.ref_leaves += ro.leaves;
    const Out off = cull_walk(o, d, t0, cr, kNoWindow), on = cull_walk(o, d, t0, cr, c_lo_on);
    A.off_nodes += off.nodes; A.off_leaves += off.leaves;
    A.on_nodes += on.nodes; A.on_leaves += on.leaves;
    for (const Out* w : {&off, &on}) {
        uint32_t a, b;
        std::memcpy(&a, &ro.t, 4);
        std::memcpy(&b, &w->t, 4);
        if (a != b || ro.tri != w->tri) {
            if (mismatches < 10)
                std::fprintf(stderr, "MISMATCH o=(%a,%a,%a) d=(%a,%a,%a): ref t=%a tri=%d, cull(%s) t=%a tri=%d\n", o.x, o.y,
                             o.z, d.x, d.y, d.z, ro.t, ro.tri, w == &on ? "on" : "off", w->t, w->tri);
            mismatches++;
        }
    }
}

float ulps(float v, int k) {   // v moved k units in the last place (k < 0: toward -inf)
    for (int i = 0; i < std::abs(k); i++) v = std::nextafterf(v, k > 0 ? INFINITY : -INFINITY);
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: window_cull_sim scene.bin [stride] [bounces] [adversarial]\n"); return 2; }
    if (!load_scene(argv[1]) || nt < 1 || nn < 1) return 2;
    const int stride = argc > 2 ? std::atoi(argv[2]) : 16;
    const int bounces = argc > 3 ? std::atoi(argv[3]) : 8;
    const long adversarial = argc > 4 ? std::atol(argv[4]) : 0;
    // a full binary tree threaded in preorder whose boxes nest, with the parents the ancestor checks need (parents
    // from the links: an internal node's children are its hit link and that child's miss link) -- the sim's own
    // restatement of pt_bvh_culling_ok, which keeps no parents
    parent.assign(nn, -1);
    bool nested = true;
    for (int i = 0; i < nn && nested; i++) {
        const float* b = &nodes[12 * (size_t)i];
        if (b[8] > -1.0f) {
            for (int k = 0; k < 2; k++)
                if (!(b[8 + k] > -1.0f && b[8 + k] < (float)nt)) nested = false;
            continue;
        }
        const int l = (int)b[10];
        if (l <= i || l >= nn) { nested = false; break; }
        const int r = (int)nodes[12 * (size_t)l + 11];
        if (r <= l || r >= nn) { nested = false; break; }
        for (int c : {l, r}) {
            parent[c] = i;
            const float* cb = &nodes[12 * (size_t)c];
            for (int q = 0; q < 3; q++)
                if (!(b[q] <= cb[q] && cb[4 + q] <= b[4 + q])) nested = false;
        }
    }
    for (int i = 1; i < nn; i++)
        if (parent[i] < 0) nested = false;
    if (!nested) {
        std::printf("{\"nested\": false}\n");
        return 3;
    }
    // the scene facts of the upload (pt_scene_pack.h): KParams::cons_m, the leaf containment and the window slack
    ptp::cons_margin(nodes.data(), cm);
    const bool win_ok = ptp::window_clause(true, ptp::leaves_contain_tris(nodes.data(), nn, tris.data()), nodes.data(), nn,
                                           tris.data(), ws);
    c_lo_on = win_ok ? ptc::kWindowLo : kNoWindow;   // a scene outside the lemma's conditions runs without the clause

    // diffuse paths: camera basis (computeShader.c:517-522), 1920x1080 grid sampled every `stride` pixels
    const int Wd = 1920, Hd = 1080;
    const f3 pos = mk(cam[0], cam[1], cam[2]);
    const f3 fwd = pt::normalize(mk(cam[4], cam[5], cam[6]));
    const f3 right = pt::normalize(pt::cross(fwd, mk(0, 0, 1)));
    const f3 up = (pt::normalize(pt::cross(right, fwd)) * (float)Hd) / (float)Wd;
    Acc P;
    if (stride > 0)
        for (int y = 0; y < Hd; y += stride)
            for (int x = 0; x < Wd; x += stride) {
                uint32_t st = pt::seed(x, y, 1);
                const float u = ((float)x + pt::random01(st)) / (float)Wd - 0.5f;
                const float v = ((float)y + pt::random01(st)) / (float)Hd - 0.5f;
                f3 o = pos, d = pt::normalize((fwd + right * u) + up * v);
                for (int bnc = 0; bnc <= bounces; bnc++) {
                    float t;
                    int tri;
                    segment(o, d, P, &t, &tri);
                    if (tri < 0) break;   // (a sphere hit ends the path here: the model follows triangles)
                    const float* tr = &tris[16 * (size_t)tri];
                    const f3 v0 = ld3(tr), v1 = ld3(tr + 4), v2 = ld3(tr + 8);
                    f3 n = pt::normalize(pt::cross(v1 - v0, v2 - v0));
                    if (pt::dot(n, d) > 0.0f) n = n * -1.0f;
                    o = o + d * t;
                    d = pt::normalize(n + pt::random_unit_vector(st));
                }
            }
    // adversarial rays.  Origins: on a triangle's plane (a point of the triangle, or of its
    // plane beside it), on a face / edge / corner of a node box, each also moved 1..4 ulps
    // either way on every axis.  Directions: toward a point of another triangle or box, random,
    // and grazing the origin's triangle with |n . d| = 2^-k, k = 0..20, on either side.
    Acc Q;
    uint32_t st = 2463534242u;
    auto rnd = [&]() { return pt::random01(st); };
    auto tri_point = [&](int ti, bool inside) {
        const float* tr = &tris[16 * (size_t)ti];
        const f3 v0 = ld3(tr), v1 = ld3(tr + 4), v2 = ld3(tr + 8);
        float a = rnd(), b = rnd();
        if (inside && a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
        if (!inside) { a = 2.0f * a - 0.5f; b = 2.0f * b - 0.5f; }
        const uint32_t r = pt::next_random(st) % 8u;
        if (r == 0) { a = 0.0f; }            // on an edge
        if (r == 1) { a = 0.0f; b = 0.0f; }  // a vertex
        return (v0 + (v1 - v0) * a) + (v2 - v0) * b;
    };
    auto box_point = [&](int ni) {
        const float* nd = &nodes[12 * (size_t)ni];
        float p[3];
        for (int q = 0; q < 3; q++) {
            const uint32_t r = pt::next_random(st) % 4u;
            p[q] = r == 0 ? nd[q] : r == 1 ? nd[4 + q] : nd[q] + (nd[4 + q] - nd[q]) * rnd();
        }
        return mk(p[0], p[1], p[2]);
    };
    for (long k = 0; k < adversarial; k++) {
        const int ta = (int)(pt::next_random(st) % (uint32_t)nt), tb = (int)(pt::next_random(st) % (uint32_t)nt);
        const uint32_t ok = pt::next_random(st) % 4u;
        f3 o = ok == 3 ? box_point((int)(pt::next_random(st) % (uint32_t)nn)) : tri_point(ta, ok != 2);
        if (pt::next_random(st) % 2u) {
            const int m = 1 + (int)(pt::next_random(st) % 4u);
            o.x = ulps(o.x, (pt::next_random(st) % 3u) == 0 ? 0 : ((pt::next_random(st) & 1u) ? m : -m));
            o.y = ulps(o.y, (pt::next_random(st) % 3u) == 0 ? 0 : ((pt::next_random(st) & 1u) ? m : -m));
            o.z = ulps(o.z, (pt::next_random(st) % 3u) == 0 ? 0 : ((pt::next_random(st) & 1u) ? m : -m));
        }
        f3 d;
        const uint32_t dk = pt::next_random(st) % 4u;
        if (dk == 0) {
            d = tri_point(tb, true) - o;
        } else if (dk == 1) {
            d = box_point((int)(pt::next_random(st) % (uint32_t)nn)) - o;
        } else if (dk == 2) {
            d = pt::random_unit_vector(st);
        } else {   // grazing triangle ta's plane
            const float* tr = &tris[16 * (size_t)ta];
            const f3 v0 = ld3(tr), v1 = ld3(tr + 4), v2 = ld3(tr + 8);
            const f3 n = pt::normalize(pt::cross(v1 - v0, v2 - v0));
            f3 tg = pt::normalize((v1 - v0) * (rnd() - 0.5f) + (v2 - v0) * (rnd() - 0.5f));
            const float s = std::ldexp((pt::next_random(st) & 1u) ? 1.0f : -1.0f, -(int)(pt::next_random(st) % 21u));
            d = tg + n * s;
        }
        if (!(pt::dot(d, d) > 0.0f)) continue;
        d = pt::normalize(d);
        float t;
        int tri;
        segment(o, d, Q, &t, &tri);
    }
    const auto frac = [](const Acc& a) { return a.ref_leaves > 0 ? a.removed / a.ref_leaves : 0.0; };
    const auto per = [](double v, const Acc& a) { return a.segs > 0 ? v / a.segs : 0.0; };
    std::printf("{\"nested\": true, \"window_on\": %s, \"n_tris\": %d, \"n_nodes\": %d, \"window_slack\": %.9g, \"path_segments\": %.0f, "
                "\"adv_segments\": %.0f, \"slow\": %ld, \"mismatches\": %ld, \"window_violations\": %ld, "
                "\"cons_violations\": %ld, \"near_hits\": %ld, "
                "\"path_ref_leaves\": %.4f, \"path_removed\": %.0f, \"path_removed_frac\": %.4f, \"path_ref_nodes\": %.4f, "
                "\"path_off_nodes\": %.4f, \"path_off_leaves\": %.4f, \"path_on_nodes\": %.4f, \"path_on_leaves\": %.4f, "
                "\"adv_ref_leaves\": %.4f, \"adv_removed\": %.0f, \"adv_removed_frac\": %.4f, \"adv_on_leaves\": %.4f}\n",
                win_ok ? "true" : "false", nt, nn, (double)std::fmax(ws[0], std::fmax(ws[1], ws[2])), P.segs, Q.segs, slow, mismatches, window_violations, cons_violations, near_hits,
                per(P.ref_leaves, P), P.removed, frac(P), per(P.ref_nodes, P), per(P.off_nodes, P), per(P.off_leaves, P),
                per(P.on_nodes, P), per(P.on_leaves, P), per(Q.ref_leaves, Q), Q.removed, frac(Q), per(Q.on_leaves, Q));
    return (mismatches || window_violations || cons_violations) ? 1 : 0;
}
