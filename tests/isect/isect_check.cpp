// TEST INFRASTRUCTURE: the per-ray arithmetic of the render kernels (csrc/pt_isect.h), run on the
// host and compared bit for bit -- no tolerance -- with its references:
//   slab_fast, slab_oct   against slab (the IEEE division chain of bvh_intersect) on triples built
//                         inside the exact-reciprocal guard, rd = pt::rcp_fast(d);
//   tri_plane + edge tests against oracle_hit_triangle, tri_mt against oracle_mt_triangle;
//   aces_px               against oracle_aces_rgba8;
//   accumulate            against prev*w + rgb/ff, w = (ff-1)/ff, each operation in double and
//                         rounded to binary32 (exact for + - * / of binary32 operands).
// Build: g++ -O2 -std=c++17 -ffp-contract=off -march=x86-64-v3 tests/isect/isect_check.cpp oracle/pt_oracle.cpp
// usage: isect_check [slab_triples] [triangle_pairs] [pixels]
// Prints one JSON line; exit status 0 = no mismatch (the first mismatches go to stderr).
#include "../../opengl-path-tracing_amd/csrc/pt_isect.h"
#include "../../opengl-path-tracing_amd/csrc/pt_scene_pack.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

extern "C" float oracle_hit_triangle(const float* o, const float* d, const float* tri, float* normal);
extern "C" float oracle_mt_triangle(const float* o, const float* d, const float* tri, float* normal);
extern "C" void oracle_aces_rgba8(const float* rgba, int n_pixels, unsigned char* out);

using pt::f3;
using pt::mk;
using ptp::Quad;

namespace {

uint64_t rs = 88172645463325252ull;
uint64_t nx() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
float uni() { return (float)((nx() >> 40) * 0x1p-24); }   // [0, 1)
float sym() { return 2.0f * uni() - 1.0f; }
float sgn() { return (nx() & 1u) ? 1.0f : -1.0f; }
float ulps(float v, int k) {   // v moved k units in the last place
    for (int i = 0; i < std::abs(k); i++) v = std::nextafterf(v, k > 0 ? INFINITY : -INFINITY);
    return v;
}
// +-m * 2^e with e uniform in [lo, hi) and m in [1, 2); the upper end 2^hi itself now and then
float mag(int lo, int hi) {
    if (nx() % 64 == 0) return sgn() * std::ldexp(1.0f, hi);
    return sgn() * std::ldexp(1.0f + uni(), lo + (int)(nx() % (uint64_t)(hi - lo)));
}
// a coordinate of the guard's scene / origin half: 0 or |v| in [2^-40, 2^60]
float gcoord() { return nx() % 16 == 0 ? 0.0f : mag(-40, 60); }
float gclamp(float v) {
    const float a = std::fabs(v);
    if (a < 0x1p-40f) return 0.0f;
    return a > 0x1p60f ? std::copysign(0x1p60f, v) : v;
}
float gedge() { return sgn() * ((nx() & 1u) ? 0x1p-40f : 0x1p60f); }   // a guard edge
// a direction component: |d| in [2^-20, 2]
float dcoord() { return mag(-20, 1); }
float dclamp(float v) {
    if (!(std::fabs(v) >= 0x1p-20f)) return std::copysign(0x1p-20f, v);
    return std::fabs(v) > 2.0f ? std::copysign(2.0f, v) : v;
}

bool same_bits(float a, float b) { return pt::fbits(a) == pt::fbits(b); }

long fails_shown = 0;
bool show() { return fails_shown++ < 10; }

// ------------------------------------------------------------------ slab tests
struct SlabStats { long triples = 0, hits = 0, fast_bad = 0, oct_bad = 0, outside = 0; };

void slab_case(const float lo[3], const float hi[3], f3 o, f3 d, float t, SlabStats& S) {
    // inside the guard by construction: counted, never skipped
    bool in = true;
    const float ov[3] = {o.x, o.y, o.z}, dv[3] = {d.x, d.y, d.z};
    for (int q = 0; q < 3; q++)
        in = in && lo[q] <= hi[q] && pt::in_guard(lo[q], 0x1p-40f, 0x1p60f) && pt::in_guard(hi[q], 0x1p-40f, 0x1p60f) &&
             pt::in_guard(ov[q], 0x1p-40f, 0x1p60f) && pt::in_range_abs(dv[q], 0x1p-20f, 2.0f);
    if (!in || t != t) { S.outside++; return; }
    const f3 rd = mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z));
    const Quad A{lo[0], hi[0], lo[1], hi[1]}, B{lo[2], hi[2], 0.0f, 0.0f};
    // the octant image's record: each axis near bound first for the sign of d
    const bool sx = std::signbit(d.x), sy = std::signbit(d.y), sz = std::signbit(d.z);
    const Quad An{sx ? hi[0] : lo[0], sx ? lo[0] : hi[0], sy ? hi[1] : lo[1], sy ? lo[1] : hi[1]};
    const Quad Bn{sz ? hi[2] : lo[2], sz ? lo[2] : hi[2], 0.0f, 0.0f};
    const bool want = pti::slab(A, B, o, d, t);
    const bool fast = pti::slab_fast(A, B, o, d, rd, t), oct = pti::slab_oct(An, Bn, o, d, rd, t);
    S.triples++;
    S.hits += want;
    if (fast != want || oct != want) {
        if (show())
            std::fprintf(stderr, "SLAB lo=(%a,%a,%a) hi=(%a,%a,%a) o=(%a,%a,%a) d=(%a,%a,%a) t=%a: slab %d fast %d oct %d\n",
                         lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], o.x, o.y, o.z, d.x, d.y, d.z, t, want, fast, oct);
        S.fast_bad += fast != want;
        S.oct_bad += oct != want;
    }
}

// the largest of the three near quotients in IEEE division (the reference's entry distance)
float near_quotient(const float lo[3], const float hi[3], f3 o, f3 d, int axis) {
    const float ov[3] = {o.x, o.y, o.z}, dv[3] = {d.x, d.y, d.z};
    float tn = -INFINITY;
    for (int q = 0; q < 3; q++) {
        if (axis >= 0 && q != axis) continue;
        const float a = (lo[q] - ov[q]) / dv[q], b = (hi[q] - ov[q]) / dv[q];
        tn = std::fmax(tn, std::fmin(a, b));
    }
    return tn;
}

void slab_random(long n, SlabStats& S) {
    for (long k = 0; k < n; k++) {
        float lo[3], hi[3], ov[3], dv[3];
        const bool wild = nx() % 4 == 0;
        if (wild) {   // every coordinate with an exponent of its own
            for (int q = 0; q < 3; q++) { lo[q] = gcoord(); hi[q] = gcoord(); ov[q] = gcoord(); }
        } else {      // a box, and an origin inside it, on a face, near it or far from it, at one scale
            const float s = std::ldexp(1.0f, (int)(nx() % 61) - 20);
            const float spread = nx() % 4 == 0 ? 16.0f : 1.0f;
            const uint64_t place = nx() % 4;
            const int face = (int)(nx() % 3);
            for (int q = 0; q < 3; q++) {
                const float c = s * spread * sym();
                lo[q] = c + s * sym();
                hi[q] = c + s * sym();
                if (lo[q] > hi[q]) std::swap(lo[q], hi[q]);
                if (place == 0) ov[q] = lo[q] + (hi[q] - lo[q]) * uni();          // inside
                else if (place == 1) ov[q] = c + 4.0f * s * sym();                // near
                else if (place == 2) ov[q] = c + 1024.0f * s * sym();             // far
                else ov[q] = q == face ? ((nx() & 1u) ? lo[q] : hi[q]) : lo[q] + (hi[q] - lo[q]) * (1.5f * uni() - 0.25f);
            }
        }
        if (nx() % 4 == 0)                                   // flat on one, two or three axes
            for (int q = 0, m = 1 + (int)(nx() % 7); q < 3; q++)
                if ((m >> q) & 1) hi[q] = lo[q];
        for (int q = 0; q < 3; q++) {                        // boxes and origins at the guard's edges
            if (nx() % 32 == 0) lo[q] = gedge();
            if (nx() % 32 == 0) hi[q] = gedge();
            if (nx() % 32 == 0) ov[q] = gedge();
            if (nx() % 16 == 0) ov[q] = (nx() & 1u) ? lo[q] : hi[q];   // origin on a face: numerator 0
            lo[q] = gclamp(lo[q]); hi[q] = gclamp(hi[q]); ov[q] = gclamp(ov[q]);
            if (lo[q] > hi[q]) std::swap(lo[q], hi[q]);
        }
        const f3 o = mk(ov[0], ov[1], ov[2]);
        if (wild || nx() % 4 == 0) {
            for (int q = 0; q < 3; q++) dv[q] = dcoord();
        } else {      // aimed at a point of the box (or of its faces)
            f3 tg = mk(0, 0, 0);
            float* tv[3] = {&tg.x, &tg.y, &tg.z};
            for (int q = 0; q < 3; q++) {
                const uint64_t r = nx() % 4;
                *tv[q] = r == 0 ? lo[q] : r == 1 ? hi[q] : lo[q] + (hi[q] - lo[q]) * uni();
            }
            f3 dd = tg - o;
            if (!(pt::dot(dd, dd) > 0.0f) || !(pt::dot(dd, dd) < INFINITY)) dd = mk(sym(), sym(), sym());
            dd = pt::normalize(dd);
            dv[0] = dclamp(dd.x); dv[1] = dclamp(dd.y); dv[2] = dclamp(dd.z);
            if (dv[0] != dv[0] || dv[1] != dv[1] || dv[2] != dv[2]) { dv[0] = dcoord(); dv[1] = dcoord(); dv[2] = dcoord(); }
        }
        const f3 d = mk(dv[0], dv[1], dv[2]);
        // t: +inf, the entry distance and one ulp either side, one axis's near quotient likewise, or any scale
        float t;
        const uint64_t tk = nx() % 8;
        if (tk == 0) t = INFINITY;
        else if (tk <= 3) t = ulps(near_quotient(lo, hi, o, d, -1), (int)tk - 2);
        else if (tk == 4) t = ulps(near_quotient(lo, hi, o, d, (int)(nx() % 3)), (int)(nx() % 3) - 1);
        else t = std::fabs(mag(-30, 70));
        slab_case(lo, hi, o, d, t, S);
    }
}

// ------------------------------------------------------------------ triangle tests
struct TriStats { long pairs = 0, hits = 0, plane_bad = 0, mt_hits = 0, mt_bad = 0; };

// hit_triangle as the kernel composes it: the stored plane (ptp::tri_plane, quad 0 of the device
// record), the plane distance (pti::tri_plane), t < 0 -> -1, the three edge tests at o + d t.
// The edge tests restate tri_edges_at (csrc/pt_render_sm.h), which reads its vertices through the
// kernel's scene view and so cannot be called here; the expressions are its three, in its order.
float kernel_hit_triangle(const float* tr, f3 o, f3 d) {
    const Quad nd = ptp::tri_plane(tr);
    const float t = pti::tri_plane(nd, o, d);
    if (t < 0.0f) return -1.0f;
    const f3 n = mk(nd.x, nd.y, nd.z), p = o + d * t;
    const f3 v0 = mk(tr[0], tr[1], tr[2]), v1 = mk(tr[4], tr[5], tr[6]), v2 = mk(tr[8], tr[9], tr[10]);
    const float e0 = pt::dot(n, pt::cross(v1 - v0, p - v0));
    const float e1 = pt::dot(n, pt::cross(v2 - v1, p - v1));
    const float e2 = pt::dot(n, pt::cross(v0 - v2, p - v2));
    return ((e0 > 0.0f) & (e1 > 0.0f) & (e2 > 0.0f)) ? t : -1.0f;
}

void tri_random(long n, TriStats& S) {
    for (long k = 0; k < n; k++) {
        const float s = std::ldexp(1.0f, (int)(nx() % 24) - 8);
        const f3 c = mk(s * sym(), s * sym(), s * sym()) * (nx() % 4 == 0 ? 64.0f : 1.0f);
        f3 v[3];
        for (int i = 0; i < 3; i++) v[i] = mk(c.x + s * sym(), c.y + s * sym(), c.z + s * sym());
        const int flat = (int)(nx() % 6);            // 0..2: axis-aligned (one coordinate shared)
        if (flat < 3)
            for (int i = 1; i < 3; i++) (flat == 0 ? v[i].x : flat == 1 ? v[i].y : v[i].z) = (flat == 0 ? v[0].x : flat == 1 ? v[0].y : v[0].z);
        const uint64_t degen = nx() % 16;             // zero area: repeated vertices, collinear
        if (degen == 0) v[1] = v[0];
        if (degen == 1) v[2] = v[1];
        if (degen == 2) v[1] = v[2] = v[0];
        if (degen == 3) v[2] = v[0] + (v[1] - v[0]) * 2.0f;
        float tr[16] = {v[0].x, v[0].y, v[0].z, 0, v[1].x, v[1].y, v[1].z, 0, v[2].x, v[2].y, v[2].z, 0, 0, 0, 0, 0};
        // the target: an interior point, a point of an edge, a vertex, or a point beside the triangle
        float a = uni(), b = uni();
        if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
        const uint64_t aim = nx() % 8;
        if (aim == 0) a = 0.0f;                       // on the edge v0-v2
        if (aim == 1) b = 0.0f;                       // on the edge v0-v1
        if (aim == 2) b = 1.0f - a;                   // on the edge v1-v2
        if (aim == 3) { a = (float)(nx() % 2); b = a == 0.0f ? (float)(nx() % 2) : 0.0f; }   // a vertex
        if (aim == 4) { a = 2.0f * a - 0.5f; b = 2.0f * b - 0.5f; }
        const f3 tg = (v[0] + (v[1] - v[0]) * a) + (v[2] - v[0]) * b;
        const float dist = std::ldexp(1.0f, (int)(nx() % 12) - 4) * s;
        f3 o = mk(tg.x + dist * sym(), tg.y + dist * sym(), tg.z + dist * sym());
        f3 d = tg - o;
        const uint64_t par = nx() % 16;
        if (par == 0) d = v[1] - v[0];                // parallel to the plane: quotient +-inf ...
        if (par == 1) { d = v[2] - v[0]; o = tg; }    // ... or 0/0 from an origin in the plane
        if (par == 2 && flat < 3) (flat == 0 ? d.x : flat == 1 ? d.y : d.z) = 0.0f;
        if (par == 3) { uint32_t st = (uint32_t)nx(); d = pt::random_unit_vector(st); }
        if (nx() % 2) d = pt::normalize(d);
        const float ov[3] = {o.x, o.y, o.z}, dv[3] = {d.x, d.y, d.z};
        float nrm[3];
        const float want = oracle_hit_triangle(ov, dv, tr, nrm), got = kernel_hit_triangle(tr, o, d);
        S.pairs++;
        S.hits += want >= 0.0f;
        if (!same_bits(want, got)) {
            if (show())
                std::fprintf(stderr, "TRI v0=(%a,%a,%a) v1=(%a,%a,%a) v2=(%a,%a,%a) o=(%a,%a,%a) d=(%a,%a,%a): oracle %a, kernel %a\n",
                             tr[0], tr[1], tr[2], tr[4], tr[5], tr[6], tr[8], tr[9], tr[10], o.x, o.y, o.z, d.x, d.y, d.z, want, got);
            S.plane_bad++;
        }
        const Quad q0{tr[0], tr[1], tr[2], 0.0f}, q1{tr[4], tr[5], tr[6], 0.0f}, q2{tr[8], tr[9], tr[10], 0.0f};
        const float mt_want = oracle_mt_triangle(ov, dv, tr, nrm), mt_got = pti::tri_mt(q0, q1, q2, o, d);
        S.mt_hits += mt_want >= 0.0f;
        if (!same_bits(mt_want, mt_got)) {
            if (show())
                std::fprintf(stderr, "MT v0=(%a,%a,%a) v1=(%a,%a,%a) v2=(%a,%a,%a) o=(%a,%a,%a) d=(%a,%a,%a): oracle %a, kernel %a\n",
                             tr[0], tr[1], tr[2], tr[4], tr[5], tr[6], tr[8], tr[9], tr[10], o.x, o.y, o.z, d.x, d.y, d.z, mt_want, mt_got);
            S.mt_bad++;
        }
    }
}

// ------------------------------------------------------------------ tonemap
struct Rgba8 { unsigned char x, y, z, w; };

unsigned char aces_byte(float x) {
    unsigned char out[4];
    const float px[4] = {x, x, x, 1.0f};
    oracle_aces_rgba8(px, 1, out);
    return out[0];
}

long aces_check(long n, long& boundaries) {
    std::vector<float> px;
    px.reserve(4 * (size_t)n);
    // the least x >= 0 that maps to byte k (the curve rises on x >= 0 and passes 1), and 3 ulps either side
    boundaries = 0;
    for (int k = 1; k <= 255; k++) {
        uint32_t lo = 0u, hi = pt::fbits(64.0f);   // aces_byte(0) = 0, aces_byte(64) = 255
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            (aces_byte(pt::bitsf(mid)) >= k ? hi : lo) = mid;
        }
        for (int u = -3; u <= 3; u++) px.push_back(pt::bitsf(hi + (uint32_t)u));
        boundaries++;
    }
    const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, INFINITY, -INFINITY, NAN, -NAN, 0x1p-149f, -0x1p-149f, 0x1.fffffep127f,
                             -0x1.fffffep127f, 0x1p-126f, 1e-3f, 0.18f, 10.0f};
    for (float s : special) px.push_back(s);
    while (px.size() < 4 * (size_t)n) {
        const uint64_t kind = nx() % 4;
        px.push_back(kind == 0 ? pt::bitsf((uint32_t)nx()) : kind == 1 ? 4.0f * uni() : kind == 2 ? uni() * uni() : mag(-20, 20));
    }
    px.resize(4 * (size_t)n);
    std::vector<unsigned char> want(4 * (size_t)n);
    oracle_aces_rgba8(px.data(), (int)n, want.data());
    long bad = 0;
    for (long i = 0; i < n; i++) {
        const Rgba8 g = pti::aces_px<Rgba8>(Quad{px[4 * i], px[4 * i + 1], px[4 * i + 2], px[4 * i + 3]});
        const unsigned char* w = &want[4 * (size_t)i];
        if (g.x != w[0] || g.y != w[1] || g.z != w[2] || g.w != w[3]) {
            if (show())
                std::fprintf(stderr, "ACES (%a,%a,%a,%a): oracle %d %d %d %d, kernel %d %d %d %d\n", px[4 * i], px[4 * i + 1],
                             px[4 * i + 2], px[4 * i + 3], w[0], w[1], w[2], w[3], g.x, g.y, g.z, g.w);
            bad++;
        }
    }
    return bad;
}

// ------------------------------------------------------------------ running mean
// one binary32 operation, computed in double and rounded once more: exact for + - * / of
// binary32 operands (53 >= 2 * 24 + 2 bits)
float mul32(float a, float b) { return (float)((double)a * (double)b); }
float div32(float a, float b) { return (float)((double)a / (double)b); }
float add32(float a, float b) { return (float)((double)a + (double)b); }

long accumulate_check(long& cases) {
    const int frames[] = {1, 2, 3, 2986, (1 << 24) + 1};
    long bad = 0;
    cases = 0;
    for (int acc = 0; acc < 2; acc++)
        for (int frame : frames)
            for (int k = 0; k < 20000; k++) {
                float pv[4], c[3];
                for (float& x : pv) x = nx() % 8 == 0 ? mag(-60, 60) : 4.0f * uni();
                for (float& x : c) x = nx() % 8 == 0 ? mag(-60, 60) : 4.0f * uni();
                if (nx() % 16 == 0) pv[nx() % 4] = 0.0f;
                if (nx() % 16 == 0) c[nx() % 3] = 0.0f;
                const Quad got = pti::accumulate(Quad{pv[0], pv[1], pv[2], pv[3]}, mk(c[0], c[1], c[2]), frame, acc != 0);
                float want[4];
                if (!acc) {
                    want[0] = c[0]; want[1] = c[1]; want[2] = c[2]; want[3] = 1.0f;
                } else {
                    const float ff = (float)(double)frame;
                    const float w = div32(add32(ff, -1.0f), ff);
                    const float in[4] = {c[0], c[1], c[2], 1.0f};
                    for (int q = 0; q < 4; q++) want[q] = add32(mul32(pv[q], w), div32(in[q], ff));
                }
                cases++;
                if (!same_bits(got.x, want[0]) || !same_bits(got.y, want[1]) || !same_bits(got.z, want[2]) || !same_bits(got.w, want[3])) {
                    if (show())
                        std::fprintf(stderr, "ACCUM prev=(%a,%a,%a,%a) rgb=(%a,%a,%a) frame %d acc %d: want (%a,%a,%a,%a), got (%a,%a,%a,%a)\n",
                                     pv[0], pv[1], pv[2], pv[3], c[0], c[1], c[2], frame, acc, want[0], want[1], want[2], want[3], got.x, got.y, got.z, got.w);
                    bad++;
                }
            }
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    const long n_slab = argc > 1 ? std::atol(argv[1]) : 2000000;
    const long n_tri = argc > 2 ? std::atol(argv[2]) : 1000000;
    const long n_px = argc > 3 ? std::atol(argv[3]) : 1000000;
    SlabStats S;
    slab_random(n_slab, S);
    TriStats T;
    tri_random(n_tri, T);
    long boundaries = 0, accum_cases = 0;
    const long aces_bad = aces_check(n_px, boundaries);
    const long accum_bad = accumulate_check(accum_cases);
    std::printf("{\"slab_triples\": %ld, \"slab_hits\": %ld, \"slab_outside_guard\": %ld, \"slab_fast_mismatches\": %ld, "
                "\"slab_oct_mismatches\": %ld, \"tri_pairs\": %ld, \"tri_hits\": %ld, \"tri_mismatches\": %ld, \"mt_hits\": %ld, "
                "\"mt_mismatches\": %ld, \"aces_pixels\": %ld, \"aces_boundaries\": %ld, \"aces_mismatches\": %ld, "
                "\"accum_cases\": %ld, \"accum_mismatches\": %ld}\n",
                S.triples, S.hits, S.outside, S.fast_bad, S.oct_bad, T.pairs, T.hits, T.plane_bad, T.mt_hits, T.mt_bad, n_px,
                boundaries, aces_bad, accum_cases, accum_bad);
    return (S.outside || S.fast_bad || S.oct_bad || T.plane_bad || T.mt_bad || aces_bad || accum_bad) ? 1 : 0;
}
