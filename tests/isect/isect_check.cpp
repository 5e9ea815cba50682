// TEST INFRASTRUCTURE: the per-ray arithmetic of the render kernels (csrc/pt_isect.h), run on the
// host and compared bit for bit -- no tolerance -- with its references:
//   slab_fast, slab_oct   against slab (the IEEE division chain of bvh_intersect) on triples built
//                         inside the exact-reciprocal guard, rd = pt::rcp_fast(d);
//   tri_plane + edge tests against oracle_hit_triangle, tri_mt against oracle_mt_triangle;
//   aces_px               against oracle_aces_rgba8;
//   accumulate            against prev*w + rgb/ff, w = (ff-1)/ff, each operation in double and
//                         rounded to binary32 (exact for + - * / of binary32 operands).
// The cases come from tests/isect/isect_cases.h, which tests/device/device_twin.hip runs on the device.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -march=x86-64-v3 tests/isect/isect_check.cpp oracle/pt_oracle.cpp
// usage: isect_check [slab_triples] [triangle_pairs] [pixels]
// Prints one JSON line; exit status 0 = no mismatch (the first mismatches go to stderr).
#include "isect_cases.h"

#include <cstdio>
#include <cstring>

extern "C" float oracle_hit_triangle(const float* o, const float* d, const float* tri, float* normal);
extern "C" float oracle_mt_triangle(const float* o, const float* d, const float* tri, float* normal);

using pt::f3;
using pt::mk;
using ptp::Quad;

namespace {

bool same_bits(float a, float b) { return pt::fbits(a) == pt::fbits(b); }

long fails_shown = 0;
bool show() { return fails_shown++ < 10; }

// ------------------------------------------------------------------ slab tests
struct SlabStats { long triples = 0, hits = 0, fast_bad = 0, oct_bad = 0, outside = 0; };

void slab_check(const std::vector<isc::SlabCase>& cases, SlabStats& S) {
    for (const isc::SlabCase& c : cases) {
        const f3 o = c.o, d = c.d;
        const f3 rd = mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z));
        Quad A, B, An, Bn;
        isc::slab_quads(c, A, B);
        isc::slab_oct_quads(c, An, Bn);
        const bool want = pti::slab(A, B, o, d, c.t);
        const bool fast = pti::slab_fast(A, B, o, d, rd, c.t), oct = pti::slab_oct(An, Bn, o, d, rd, c.t);
        S.triples++;
        S.hits += want;
        if (fast != want || oct != want) {
            if (show())
                std::fprintf(stderr, "SLAB lo=(%a,%a,%a) hi=(%a,%a,%a) o=(%a,%a,%a) d=(%a,%a,%a) t=%a: slab %d fast %d oct %d\n",
                             c.lo[0], c.lo[1], c.lo[2], c.hi[0], c.hi[1], c.hi[2], o.x, o.y, o.z, d.x, d.y, d.z, c.t, want, fast, oct);
            S.fast_bad += fast != want;
            S.oct_bad += oct != want;
        }
    }
}

// ------------------------------------------------------------------ triangle tests
struct TriStats { long pairs = 0, hits = 0, plane_bad = 0, mt_hits = 0, mt_bad = 0; };

void tri_check(const std::vector<isc::TriCase>& cases, TriStats& S) {
    for (const isc::TriCase& c : cases) {
        float tr[16];
        isc::tri_record(c, tr);
        const f3 o = c.o, d = c.d;
        const f3 v0 = mk(tr[0], tr[1], tr[2]), v1 = mk(tr[4], tr[5], tr[6]), v2 = mk(tr[8], tr[9], tr[10]);
        const float ov[3] = {o.x, o.y, o.z}, dv[3] = {d.x, d.y, d.z};
        float nrm[3];
        // (the edge tests of isc::kernel_hit_triangle are the twin of tri_edges_at, csrc/pt_render_sm.h)
        const float want = oracle_hit_triangle(ov, dv, tr, nrm), got = isc::kernel_hit_triangle(ptp::tri_plane(tr), v0, v1, v2, o, d);
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

long aces_check(const std::vector<float>& px) {
    const long n = (long)(px.size() / 4);
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
long accumulate_check(const std::vector<isc::AccumCase>& cases) {
    long bad = 0;
    for (const isc::AccumCase& a : cases) {
        const float *pv = a.pv, *c = a.c;
        const Quad got = pti::accumulate(Quad{pv[0], pv[1], pv[2], pv[3]}, mk(c[0], c[1], c[2]), a.frame, a.acc != 0);
        float want[4];
        isc::accumulate_definition(a, want);
        if (!same_bits(got.x, want[0]) || !same_bits(got.y, want[1]) || !same_bits(got.z, want[2]) || !same_bits(got.w, want[3])) {
            if (show())
                std::fprintf(stderr, "ACCUM prev=(%a,%a,%a,%a) rgb=(%a,%a,%a) frame %d acc %d: want (%a,%a,%a,%a), got (%a,%a,%a,%a)\n",
                             pv[0], pv[1], pv[2], pv[3], c[0], c[1], c[2], a.frame, a.acc, want[0], want[1], want[2], want[3], got.x, got.y, got.z, got.w);
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
    // the generators draw from one stream, in this order
    std::vector<isc::SlabCase> slabs;
    std::vector<isc::TriCase> tris;
    std::vector<float> px;
    std::vector<isc::AccumCase> accums;
    SlabStats S;
    S.outside = isc::slab_random(n_slab, slabs);
    isc::tri_random(n_tri, tris);
    const long boundaries = isc::aces_pixels(n_px, px);
    isc::accumulate_cases(accums);
    slab_check(slabs, S);
    TriStats T;
    tri_check(tris, T);
    const long aces_bad = aces_check(px);
    const long accum_bad = accumulate_check(accums);
    const long accum_cases = (long)accums.size();
    std::printf("{\"slab_triples\": %ld, \"slab_hits\": %ld, \"slab_outside_guard\": %ld, \"slab_fast_mismatches\": %ld, "
                "\"slab_oct_mismatches\": %ld, \"tri_pairs\": %ld, \"tri_hits\": %ld, \"tri_mismatches\": %ld, \"mt_hits\": %ld, "
                "\"mt_mismatches\": %ld, \"aces_pixels\": %ld, \"aces_boundaries\": %ld, \"aces_mismatches\": %ld, "
                "\"accum_cases\": %ld, \"accum_mismatches\": %ld}\n",
                S.triples, S.hits, S.outside, S.fast_bad, S.oct_bad, T.pairs, T.hits, T.plane_bad, T.mt_hits, T.mt_bad, n_px,
                boundaries, aces_bad, accum_cases, accum_bad);
    return (S.outside || S.fast_bad || S.oct_bad || T.plane_bad || T.mt_bad || aces_bad || accum_bad) ? 1 : 0;
}
