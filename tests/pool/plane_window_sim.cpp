// TEST INFRASTRUCTURE: CPU model of the path pool's plane-window filter (pti::pair_in_window, pt_isect.h; DESIGN.md
// §5.12, "Round 20") against the reference's binary32 walk (tests/ref_walk.h).  It runs the SAME code as the kernel and
// the uploader: the packer's sweep table and triangle quads (ptp::pack_scene), ptc::cull_addends / sweep_mask for the
// candidate mask, pti::pair_in_window on the packed quad 0 of the own pair's two slots for the filtered mask, and
// pti::slab_oct for the leaf phase's exact re-test.  The own pair of a bounce ray is the leaf the reference walk's hit
// came from (the kernel's hprim >> 1); the filter is an equivalence for any pair, so an adversarial ray names the leaf
// of the triangle its origin was drawn on, or a random one.  It fails on
//   (a) a segment whose final t (bitwise) or triangle through the filtered mask differs from the reference's,
//   (b) a filter verdict that differs from the plane tests of the leaf phase restated here on the same quads
//       (both distances outside their windows at t0).
// It reports per segment: the candidate visits, the visits the filter removes, the visits whose two plane distances
// are outside their windows at t0 (every bit, and the own pair's share) and at the t current at the visit, the share
// of the remaining visits that need edge tests with the needed (lane, triangle) pairs per visit, and the filtered
// candidate histogram (0, 1, 2, 3, 4+; the mean of the last bucket beside it).
//
// usage: plane_window_sim scene.bin [stride] [bounces] [adversarial_rays]
//   scene.bin as tests/ref_walk.h reads it (written by tests/test_plane_window.py).
// Exit status 0 = no violation, 1 = a violation, 3 = the scene has no sweep table.  Output: one JSON line.
#include "../../opengl-path-tracing_amd/csrc/pt_cull.h"
#include "../../opengl-path-tracing_amd/csrc/pt_isect.h"
#include "../../opengl-path-tracing_amd/csrc/pt_scene_pack.h"
#include "../../include/pt_api.h"
#include "../ref_walk.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// pt_scene.cpp (linked for pt_bvh_culling_ok) refers to the GPU builder; this binary is host-only
extern "C" int pt_bvh_build_gpu(const float*, int, float*, int, int*, int) { return PT_E_HIP; }

using pt::f3;
using pt::mk;
using namespace ref;

namespace {

ptp::PackedScene packed;
const ptp::Quad* table = nullptr;
const ptp::Quad* ptris = nullptr;   // the packed triangle slots: pair q at quads 8 q .. 8 q + 7
int n_sweep = 0;
std::vector<int> chain;             // reference node of chain position k
const float c_lo = ptc::kWindowLo;

long mismatches = 0, verdict_errors = 0, slow = 0;
struct Acc {
    double segs = 0, cand = 0, removed = 0, out_t0 = 0, out_t0_own = 0, out_cur = 0, left = 0, left_edges = 0, left_pairs = 0;
    double hist[5] = {0, 0, 0, 0, 0}, top_sum = 0;
};

struct Out { float t; int tri, leaf; };

int as_int(float v) { int i; std::memcpy(&i, &v, 4); return i; }

bool retest(int node, f3 o, f3 d, f3 rd, float t) {   // the leaf phase's exact re-test on the ray's octant image
    const float* b = &nodes[12 * (size_t)node];
    const bool sx = std::signbit(d.x), sy = std::signbit(d.y), sz = std::signbit(d.z);
    const ptp::Quad A = {sx ? b[4] : b[0], sx ? b[0] : b[4], sy ? b[5] : b[1], sy ? b[1] : b[5]};
    const ptp::Quad B = {sz ? b[6] : b[2], sz ? b[2] : b[6], 0.0f, 0.0f};
    return pti::slab_oct(A, B, o, d, rd, t);
}

// The kernel's leaf phase over a candidate mask: lowest bit first, the reference's 2-way choice, and its winner
// moves t only if the leaf's own box passes the exact test at the current t.
Out sweep_walk(unsigned mask, f3 o, f3 d, f3 rd, float t0) {
    Out r{t0, -1, -1};
    for (; mask; mask &= mask - 1) {
        const int k = __builtin_ctz(mask), node = chain[k];
        float t2;
        int tri;
        if (leaf_choice(node, o, d, r.t, t2, tri) && retest(node, o, d, rd, r.t)) { r.t = t2; r.tri = tri; r.leaf = k; }
    }
    return r;
}

// The packed quads of chain position k's pair, as the kernel's chain-order copy holds them at slots 2 k, 2 k + 1.
struct PairQuads { ptp::Quad a, b; bool cop; };
PairQuads pair_quads(int k) {
    const int pair = as_int(table[2 * k + 1].z);
    const ptp::Quad* q = ptris + 8 * (size_t)pair;
    return {q[0], q[4], as_int(q[5].w) != 0};
}
// The leaf phase's plane tests of that pair at t, restated: which of its two triangles need edge tests.
void plane_tests(int k, f3 o, f3 d, float t, bool& na, bool& nb) {
    const PairQuads pq = pair_quads(k);
    const float ta = pti::tri_plane(pq.a, o, d);
    const float tb = pq.cop ? ta : pti::tri_plane(pq.b, o, d);
    na = pt::win_open(ta, t);
    nb = pt::win_closed(tb, t);
}

// One segment.  own: the chain position of the pair the ray leaves, or -1.  Returns the chain position of the leaf
// the hit came from (-1: none, or a ray outside the guard, whose cold walk the filter does not touch).
int segment(f3 o, f3 d, int own, Acc& A, float* t_out, int* tri_out) {
    const float t0 = sphere_t(o, d);
    int hit_node = -1;
    const RefOut ro = ref_walk(
        o, d, t0, [](int, bool, float) {},
        [&](int bi, float, bool moves, float) { if (moves) hit_node = bi; });
    *t_out = ro.t;
    *tri_out = ro.tri;
    const int hit_leaf = hit_node < 0 ? -1 : (int)(std::find(chain.begin(), chain.end(), hit_node) - chain.begin());
    if (!pti::ray_in_guard(true, o, d)) { slow++; return hit_leaf; }   // the kernel's own verdict
    // the kernel's segment set-up: the candidate mask, then the own pair's bit
    const f3 rd = mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z));
    f3 ol, oh;
    ptc::cull_addends(o, rd, packed.facts.cons_m, packed.facts.win_slack, ol, oh);
    const ptc::SweepRay sr = ptc::sweep_ray(rd, ol, oh);
    const unsigned cand = ptc::sweep_root_hit(packed.facts.root_box, sr, t0, c_lo) ? ptc::sweep_mask(sr, t0, c_lo, table, n_sweep) : 0u;
    unsigned filtered = cand;
    if (own >= 0 && ((cand >> own) & 1u)) {
        const PairQuads pq = pair_quads(own);
        const bool keep = pti::pair_in_window(pq.a, pq.b, pq.cop, o, d, t0);
        bool na, nb;
        plane_tests(own, o, d, t0, na, nb);
        if (keep != (na | nb)) verdict_errors++;
        if (!keep) filtered &= ~(1u << own);
    }
    A.segs++;
    A.cand += __builtin_popcount(cand);
    A.removed += __builtin_popcount(cand ^ filtered);
    for (unsigned m = cand; m; m &= m - 1) {   // what a filter over every bit would remove
        const int k = __builtin_ctz(m);
        bool na, nb;
        plane_tests(k, o, d, t0, na, nb);
        if (!(na | nb)) { A.out_t0++; if (k == own) A.out_t0_own++; }
    }
    {   // the visits as the LEAF pass runs them, at the current t: over the full mask (what it finds today) ...
        float t = t0;
        for (unsigned m = cand; m; m &= m - 1) {
            const int k = __builtin_ctz(m);
            bool na, nb;
            plane_tests(k, o, d, t, na, nb);
            if (!(na | nb)) A.out_cur++;
            float t2;
            int tri;
            if (leaf_choice(chain[k], o, d, t, t2, tri) && retest(chain[k], o, d, rd, t)) t = t2;
        }
        t = t0;   // ... and over the filtered one: how dense the remaining visits' edge tests are
        for (unsigned m = filtered; m; m &= m - 1) {
            const int k = __builtin_ctz(m);
            bool na, nb;
            plane_tests(k, o, d, t, na, nb);
            A.left++;
            A.left_edges += (na | nb) ? 1 : 0;
            A.left_pairs += (na ? 1 : 0) + (nb ? 1 : 0);
            float t2;
            int tri;
            if (leaf_choice(chain[k], o, d, t, t2, tri) && retest(chain[k], o, d, rd, t)) t = t2;
        }
    }
    const int nf = __builtin_popcount(filtered);
    A.hist[std::min(nf, 4)]++;
    if (nf >= 4) A.top_sum += nf;
    const Out w = sweep_walk(filtered, o, d, rd, t0);
    uint32_t a, b;
    std::memcpy(&a, &ro.t, 4);
    std::memcpy(&b, &w.t, 4);
    if (a != b || ro.tri != w.tri) {
        if (mismatches < 10)
            std::fprintf(stderr, "MISMATCH o=(%a,%a,%a) d=(%a,%a,%a) own=%d: ref t=%a tri=%d, filtered t=%a tri=%d\n", o.x, o.y,
                         o.z, d.x, d.y, d.z, own, ro.t, ro.tri, w.t, w.tri);
        mismatches++;
    }
    return hit_leaf;
}

float ulps(float v, int k) {   // v moved k units in the last place (k < 0: toward -inf)
    for (int i = 0; i < std::abs(k); i++) v = std::nextafterf(v, k > 0 ? INFINITY : -INFINITY);
    return v;
}

// Hand-made cases of pti::pair_in_window (`plane_window_sim --cases`): the plane z = h seen along +z from the origin
// has the plane distance h exactly (n = (0, 0, 1), d0 = -h: -(0 + -h) / 1), so the window's ends can be hit bitwise.
int run_cases() {
    int n = 0, failed = 0;
    const auto check = [&](const char* what, bool got, bool want) {
        n++;
        if (got != want) { failed++; std::fprintf(stderr, "CASE %s: got %d, want %d\n", what, (int)got, (int)want); }
    };
    const auto plane_z = [](float h) { return ptp::Quad{0.0f, 0.0f, 1.0f, -h}; };
    const f3 o = mk(0, 0, 0), up = mk(0, 0, 1);
    const float lo = 0.0001f, inf = INFINITY;
    const ptp::Quad far_away = plane_z(-5.0f);   // behind the ray: never in a window
    // the lower end: open for the first triangle, closed for the second
    check("first at 1e-4", pti::pair_in_window(plane_z(lo), far_away, false, o, up, inf), false);
    check("first one ulp above 1e-4", pti::pair_in_window(plane_z(ulps(lo, 1)), far_away, false, o, up, inf), true);
    check("second at 1e-4", pti::pair_in_window(far_away, plane_z(lo), false, o, up, inf), true);
    check("second one ulp below 1e-4", pti::pair_in_window(far_away, plane_z(ulps(lo, -1)), false, o, up, inf), false);
    check("coplanar pair at 1e-4 (the second's closed end)", pti::pair_in_window(plane_z(lo), plane_z(lo), true, o, up, inf), true);
    check("coplanar pair one ulp below 1e-4", pti::pair_in_window(plane_z(ulps(lo, -1)), far_away, true, o, up, inf), false);
    // the upper end: t0 itself is outside for both
    check("first at t0", pti::pair_in_window(plane_z(2.0f), far_away, false, o, up, 2.0f), false);
    check("second at t0", pti::pair_in_window(far_away, plane_z(2.0f), false, o, up, 2.0f), false);
    check("first one ulp below t0", pti::pair_in_window(plane_z(ulps(2.0f, -1)), far_away, false, o, up, 2.0f), true);
    check("second one ulp below t0", pti::pair_in_window(far_away, plane_z(ulps(2.0f, -1)), false, o, up, 2.0f), true);
    check("beyond t0", pti::pair_in_window(plane_z(3.0f), plane_z(4.0f), false, o, up, 2.0f), false);
    // t0 = +inf: every finite distance above 1e-4 is inside, +inf is not
    check("t0 = inf, finite distance", pti::pair_in_window(plane_z(0x1p100f), far_away, false, o, up, inf), true);
    // a zero denominator: +-inf, and NaN where the origin is on the plane too
    const f3 along = mk(1, 0, 0);
    check("parallel ray below the plane (+inf)", pti::pair_in_window(plane_z(1.0f), plane_z(1.0f), true, o, along, inf), false);
    check("parallel ray above the plane (-inf)", pti::pair_in_window(plane_z(-1.0f), plane_z(-1.0f), true, o, along, inf), false);
    check("parallel ray in the plane (NaN)", pti::pair_in_window(plane_z(0.0f), plane_z(0.0f), true, o, along, inf), false);
    check("NaN first, +inf second", pti::pair_in_window(plane_z(0.0f), plane_z(1.0f), false, o, along, inf), false);
    check("zero first, second inside", pti::pair_in_window(plane_z(0.0f), plane_z(1.0f), false, o, mk(1, 0, 0x1p-30f), inf), true);
    check("NaN plane record", pti::pair_in_window(ptp::Quad{NAN, NAN, NAN, NAN}, far_away, false, o, up, inf), false);
    // a non-coplanar pair: only the second triangle's plane is in its window (the first is behind the ray) -- and the
    // coplanar flag would have dropped it
    const ptp::Quad tilted = {0.0f, 0.6f, 0.8f, -0.4f};
    check("only the second inside", pti::pair_in_window(far_away, tilted, false, o, up, inf), true);
    check("the same quads read as coplanar", pti::pair_in_window(far_away, tilted, true, o, up, inf), false);
    // a ray that starts on the pair's own plane z = 0.3, its origin moved 0..4 ulps either way, leaving at a grazing
    // 2^-12 on either side: the distance is -(RN(o.z - 0.3)) / d.z, a few 1e-4 around the window's lower end
    for (int k = -4; k <= 4; k++)
        for (int side = -1; side <= 1; side += 2) {
            const float h = 0.3f, oz = ulps(h, k), dz = side * 0x1p-12f;
            const volatile float num = oz + -h;      // dot(n, o) + d0 with n = (0, 0, 1): 0 + 0 + o.z, then + d0
            const volatile float want_t = -num / dz;
            const bool want = want_t >= lo && want_t < inf;   // a coplanar pair: the second's closed window is the wider
            char what[96];
            std::snprintf(what, sizeof what, "own plane, origin %+d ulps, d.z = %a (distance %a)", k, dz, (float)want_t);
            check(what, pti::pair_in_window(plane_z(h), plane_z(h), true, mk(0.25f, -0.5f, oz), mk(0.6f, 0.8f, dz), inf), want);
        }
    std::printf("{\"cases\": %d, \"failed\": %d}\n", n, failed);
    return failed ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--cases") == 0) return run_cases();
    if (argc < 2) { std::fprintf(stderr, "usage: plane_window_sim scene.bin [stride] [bounces] [adversarial]\n"); return 2; }
    if (!load_scene(argv[1]) || nt < 1 || nn < 1) return 2;
    const int stride = argc > 2 ? std::atoi(argv[2]) : 16;
    const int bounces = argc > 3 ? std::atoi(argv[3]) : 8;
    const long adversarial = argc > 4 ? std::atol(argv[4]) : 0;
    // the uploader's view of the scene: materials as many as the records name (the scene file carries none)
    int n_mats = 1;
    for (int i = 0; i < nt; i++) n_mats = std::max(n_mats, (int)tris[16 * (size_t)i + 12] + 1);
    for (int i = 0; i < ns; i++) n_mats = std::max(n_mats, (int)sph[8 * (size_t)i + 4] + 1);
    const std::vector<float> mats(16 * (size_t)n_mats, 0.0f);
    std::string err;
    const int rc = ptp::pack_scene(tris.data(), nt, nodes.data(), nn, mats.data(), n_mats, ns ? sph.data() : nullptr, ns, packed, err);
    if (rc) { std::fprintf(stderr, "pack_scene: %s\n", err.c_str()); return 2; }
    const ptl::SceneFacts& sf = packed.facts;
    if (!sf.sweep_ok) {
        std::printf("{\"sweep_ok\": false, \"n_leaves\": %d}\n", sf.n_leaves);
        return 3;
    }
    n_sweep = sf.n_leaves;
    table = reinterpret_cast<const ptp::Quad*>(packed.buf[ptp::kSweep].data());
    ptris = reinterpret_cast<const ptp::Quad*>(packed.buf[ptp::kTris].data());
    for (int i = 0; i > -1;) {   // the chain: an internal node leads to its hit link, a leaf to its miss link
        const float* b = &nodes[12 * (size_t)i];
        const bool leaf = b[8] > -1.0f;
        if (leaf) chain.push_back(i);
        i = (int)b[leaf ? 11 : 10];
    }
    if ((int)chain.size() != n_sweep || packed.buf[ptp::kTris].size() < 32 * (size_t)n_sweep) return 2;
    std::vector<int> leaf_of_tri(nt, -1);   // chain position of the leaf that holds a triangle
    int non_coplanar = 0;
    for (int k = 0; k < n_sweep; k++) {
        const float* b = &nodes[12 * (size_t)chain[k]];
        leaf_of_tri[(int)b[8]] = leaf_of_tri[(int)b[9]] = k;
        non_coplanar += pair_quads(k).cop ? 0 : 1;
    }

    // diffuse paths as tests/cull/leaf_sweep_sim.cpp draws them: the camera basis (computeShader.c:517-522), a
    // 1920x1080 grid sampled every `stride` pixels
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
                int own = -1;   // a camera ray has no own pair
                for (int bnc = 0; bnc <= bounces; bnc++) {
                    float t;
                    int tri;
                    own = segment(o, d, own, P, &t, &tri);
                    if (tri < 0) break;   // (a sphere hit ends the path here: the model follows triangles)
                    const float* tr = &tris[16 * (size_t)tri];
                    const f3 v0 = ld3(tr), v1 = ld3(tr + 4), v2 = ld3(tr + 8);
                    f3 n = pt::normalize(pt::cross(v1 - v0, v2 - v0));
                    if (pt::dot(n, d) > 0.0f) n = n * -1.0f;
                    o = o + d * t;
                    d = pt::normalize(n + pt::random_unit_vector(st));
                }
            }
    // adversarial rays, as tests/cull/leaf_sweep_sim.cpp draws them.  Origins: on a triangle's plane (a point of the
    // triangle, or of its plane beside it), on a face / edge / corner of a node box, each also moved 1..4 ulps either
    // way on every axis.  Directions: toward a point of another triangle or box, random, and grazing the origin's
    // triangle with |n . d| = 2^-k, k = 0..20, on either side.  The own pair is the origin triangle's leaf.
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
        // (a triangle no leaf holds has no pair: any pair is a valid subject of the filter)
        const int own = leaf_of_tri[ta] >= 0 ? leaf_of_tri[ta] : (int)(pt::next_random(st) % (uint32_t)n_sweep);
        float t;
        int tri;
        segment(o, d, own, Q, &t, &tri);
    }
    const auto per = [](double v, const Acc& a) { return a.segs > 0 ? v / a.segs : 0.0; };
    const auto of = [](double v, double n) { return n > 0 ? v / n : 0.0; };
    std::printf("{\"sweep_ok\": true, \"n_leaves\": %d, \"non_coplanar_pairs\": %d, \"path_segments\": %.0f, \"adv_segments\": %.0f, "
                "\"slow\": %ld, \"mismatches\": %ld, \"verdict_errors\": %ld, "
                "\"path_candidates\": %.4f, \"path_removed\": %.4f, \"path_outside_t0\": %.4f, \"path_outside_t0_own\": %.4f, "
                "\"path_outside_current\": %.4f, \"path_left\": %.4f, \"path_left_edge_share\": %.4f, "
                "\"path_left_pairs_per_visit\": %.4f, \"path_hist\": [%.4f, %.4f, %.4f, %.4f, %.4f], \"path_hist_top_mean\": %.4f, "
                "\"adv_candidates\": %.4f, \"adv_removed\": %.4f, \"adv_outside_t0\": %.4f, \"adv_left_edge_share\": %.4f}\n",
                n_sweep, non_coplanar, P.segs, Q.segs, slow, mismatches, verdict_errors, per(P.cand, P), per(P.removed, P),
                per(P.out_t0, P), per(P.out_t0_own, P), per(P.out_cur, P), per(P.left, P), of(P.left_edges, P.left),
                of(P.left_pairs, P.left), per(P.hist[0], P), per(P.hist[1], P), per(P.hist[2], P), per(P.hist[3], P),
                per(P.hist[4], P), of(P.top_sum, P.hist[4]), per(Q.cand, Q), per(Q.removed, Q), per(Q.out_t0, Q),
                of(Q.left_edges, Q.left));
    return (mismatches || verdict_errors) ? 1 : 0;
}
