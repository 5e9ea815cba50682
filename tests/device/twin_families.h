// TEST INFRASTRUCTURE: the families of the device twin.  A family names a case type and
//   eval(case, ctx, words)   the pinned header functions, called as the render kernels call them, their results
//                            written as W 32-bit words.  PT_HD: tests/device/device_twin.hip compiles it for the
//                            device (one case per thread) and for the host; tests/device/twin_host.cpp for the host;
//   ref(case, ctx, self, r)  host only: the words an independent reference expects (DESIGN.md §3.2 names them).
//                            `self` is the result under judgement: a word no reference covers is copied from it, and
//                            a claim that two results of one evaluation agree is judged on `self` alone;
//   positive(case, words)    the verdict counted in `positives`;
//   nudge(case)              the smallest step of one operand (the sensitivity run of device_twin --nudge);
//   show(case)               the operands in %a, for a mismatch report.
// Float words are bit patterns, with every NaN written as 0x7fc00000: the payload and sign of a NaN that an
// operation makes differ between the CPU and the GPU, and nothing in the headers reads them.
#pragma once

#include "twin_cases.h"
#include "../ref_walk.h"

#include <cstdio>

extern "C" float oracle_hit_sphere(const float* o, const float* d, const float* sphere);
extern "C" float oracle_hit_triangle(const float* o, const float* d, const float* tri, float* normal);
extern "C" float oracle_mt_triangle(const float* o, const float* d, const float* tri, float* normal);

namespace twf {

using pt::f3;
using pt::mk;
using ptp::Quad;

PT_HD uint32_t fw(float f) { return f != f ? 0x7fc00000u : pt::fbits(f); }
// one unit in the last place (from inf or NaN: down)
inline float step(float f) {
    const uint32_t u = pt::fbits(f);
    return pt::bitsf((u & 0x7fffffffu) >= 0x7f800000u ? u - 1u : u + 1u);
}
PT_HD f3 rcp3(f3 d) { return mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z)); }   // the kernels' rd inside the guard

struct NoCtx {};
struct Rgba8 { unsigned char x, y, z, w; };

// ------------------------------------------------------------------ slab: the three box tests inside the guard
struct Slab {
    using Case = isc::SlabCase;
    using Ctx = NoCtx;
    static constexpr int W = 1;
    static constexpr bool boolean = true, has_ref = true;
    static const char* name() { return "slab"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        const f3 rd = rcp3(c.d);
        const bool sx = pt::fbits(c.d.x) >> 31, sy = pt::fbits(c.d.y) >> 31, sz = pt::fbits(c.d.z) >> 31;
        const Quad A{c.lo[0], c.hi[0], c.lo[1], c.hi[1]}, B{c.lo[2], c.hi[2], 0.0f, 0.0f};
        const Quad An{sx ? c.hi[0] : c.lo[0], sx ? c.lo[0] : c.hi[0], sy ? c.hi[1] : c.lo[1], sy ? c.lo[1] : c.hi[1]};
        const Quad Bn{sz ? c.hi[2] : c.lo[2], sz ? c.lo[2] : c.hi[2], 0.0f, 0.0f};
        r[0] = (uint32_t)pti::slab(A, B, c.o, c.d, c.t) | (uint32_t)pti::slab_fast(A, B, c.o, c.d, rd, c.t) << 1 |
               (uint32_t)pti::slab_oct(An, Bn, c.o, c.d, rd, c.t) << 2;
    }
    // slab_fast and slab_oct against the host's IEEE chain
    static void ref(const Case& c, const Ctx&, const uint32_t*, uint32_t* r) {
        Quad A, B;
        isc::slab_quads(c, A, B);
        r[0] = pti::slab(A, B, c.o, c.d, c.t) ? 7u : 0u;
    }
    static bool positive(const Case&, const uint32_t* r) { return r[0] & 1u; }
    static void nudge(Case& c) { c.t = step(c.t); }
    static void show(const Case& c) {
        std::fprintf(stderr, "lo=(%a,%a,%a) hi=(%a,%a,%a) o=(%a,%a,%a) d=(%a,%a,%a) t=%a", c.lo[0], c.lo[1], c.lo[2], c.hi[0], c.hi[1],
                     c.hi[2], c.o.x, c.o.y, c.o.z, c.d.x, c.d.y, c.d.z, c.t);
    }
};

// ------------------------------------------------------------------ slab_wild: the IEEE chain on any binary32
struct SlabWild {
    using Case = isc::SlabCase;
    using Ctx = NoCtx;
    static constexpr int W = 1;
    static constexpr bool boolean = true, has_ref = false;
    static const char* name() { return "slab_wild"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        const Quad A{c.lo[0], c.hi[0], c.lo[1], c.hi[1]}, B{c.lo[2], c.hi[2], 0.0f, 0.0f};
        r[0] = (uint32_t)pti::slab(A, B, c.o, c.d, c.t);
    }
    static void ref(const Case&, const Ctx&, const uint32_t* self, uint32_t* r) { r[0] = self[0]; }
    static bool positive(const Case&, const uint32_t* r) { return r[0] & 1u; }
    static void nudge(Case& c) { c.t = step(c.t); }
    static void show(const Case& c) { Slab::show(c); }
};

// ------------------------------------------------------------------ cull: slab_oct_cons and sweep_hit
struct Cull {
    using Case = twc::CullCase;
    using Ctx = NoCtx;
    static constexpr int W = 7;
    static constexpr bool boolean = true, has_ref = true;
    static const char* name() { return "cull"; }
    PT_HD static void eval(const Case& k, const Ctx&, uint32_t* r) {
        const isc::SlabCase& c = k.s;
        const f3 rd = rcp3(c.d);
        f3 ol, oh;
        ptc::cull_addends(c.o, rd, k.cm, k.ws, ol, oh);
        const bool sx = pt::fbits(c.d.x) >> 31, sy = pt::fbits(c.d.y) >> 31, sz = pt::fbits(c.d.z) >> 31;
        const Quad An{sx ? c.hi[0] : c.lo[0], sx ? c.lo[0] : c.hi[0], sy ? c.hi[1] : c.lo[1], sy ? c.lo[1] : c.hi[1]};
        const Quad Bn{sz ? c.hi[2] : c.lo[2], sz ? c.lo[2] : c.hi[2], 0.0f, 0.0f};
        const bool cons = pti::slab_oct_cons(An, Bn, rd, ol, oh, c.t, k.c_lo);
        const ptc::SweepRay sr = ptc::sweep_ray(rd, ol, oh);
        const bool sweep = ptc::sweep_hit(c.lo[0], c.hi[0], c.lo[1], c.hi[1], c.lo[2], c.hi[2], sr, c.t, k.c_lo);
        r[0] = (uint32_t)cons | (uint32_t)sweep << 1;
        r[1] = fw(ol.x), r[2] = fw(ol.y), r[3] = fw(ol.z), r[4] = fw(oh.x), r[5] = fw(oh.y), r[6] = fw(oh.z);
    }
    // pt_cull.h: the sweep's test on the reference order is cull_hit's on the octant image, "up to the sign of a
    // zero, which only enters comparisons": the two verdicts of one evaluation are each other's reference
    static void ref(const Case&, const Ctx&, const uint32_t* self, uint32_t* r) {
        for (int i = 0; i < W; i++) r[i] = self[i];
        r[0] = (self[0] >> 1 & 1u) | (self[0] & 1u) << 1;
    }
    static bool positive(const Case&, const uint32_t* r) { return r[0] & 1u; }
    static void nudge(Case& k) { k.s.t = step(k.s.t); }
    static void show(const Case& k) {
        Slab::show(k.s);
        std::fprintf(stderr, " cm=(%a,%a,%a) ws=(%a,%a,%a) c_lo=%a", k.cm[0], k.cm[1], k.cm[2], k.ws[0], k.ws[1], k.ws[2], k.c_lo);
    }
};

// ------------------------------------------------------------------ sweep: the candidate mask over one table
struct SweepCtx {
    const Quad* table;   // device memory in the kernel: one table for all rays of a launch, read as the kernel reads it
    int n;
    float cm[3], ws[3];
    int flip;            // --nudge: the verdict fed to sweep_push is inverted
};
struct Sweep {
    using Case = twc::SweepRayCase;
    using Ctx = SweepCtx;
    static constexpr int W = 2;
    static constexpr bool boolean = true, has_ref = true;
    static const char* name() { return "sweep"; }
    PT_HD static void eval(const Case& c, const Ctx& x, uint32_t* r) {
        const f3 rd = rcp3(c.d);
        f3 ol, oh;
        ptc::cull_addends(c.o, rd, x.cm, x.ws, ol, oh);
        const ptc::SweepRay sr = ptc::sweep_ray(rd, ol, oh);
        r[0] = ptc::sweep_mask(sr, c.t, c.c_lo, x.table, x.n);
        unsigned m = 0u;   // sweep_push on its own, so that --nudge can reach its operand
        for (int k = x.n - 1; k >= 0; k--) {
            const Quad a = x.table[2 * k], b = x.table[2 * k + 1];
            m = ptc::sweep_push(m, ptc::sweep_hit(a.x, a.y, a.z, a.w, b.x, b.y, sr, c.t, c.c_lo) != (x.flip != 0));
        }
        r[1] = m;
    }
    // the mask assembled from the host's sweep_hit verdicts, bit k = entry k (x.table: the host copy)
    static void ref(const Case& c, const Ctx& x, const uint32_t*, uint32_t* r) {
        const f3 rd = mk(1.0f / c.d.x, 1.0f / c.d.y, 1.0f / c.d.z);
        f3 ol, oh;
        ptc::cull_addends(c.o, rd, x.cm, x.ws, ol, oh);
        const ptc::SweepRay sr = ptc::sweep_ray(rd, ol, oh);
        unsigned m = 0u;
        for (int k = 0; k < x.n; k++) {
            const Quad a = x.table[2 * k], b = x.table[2 * k + 1];
            if (ptc::sweep_hit(a.x, a.y, a.z, a.w, b.x, b.y, sr, c.t, c.c_lo)) m |= 1u << k;
        }
        r[0] = r[1] = m;
    }
    static bool positive(const Case&, const uint32_t* r) { return r[0] != 0u; }
    static void nudge(Case& c) { c.t = step(c.t); }
    static void show(const Case& c) {
        std::fprintf(stderr, "o=(%a,%a,%a) d=(%a,%a,%a) t=%a c_lo=%a", c.o.x, c.o.y, c.o.z, c.d.x, c.d.y, c.d.z, c.t, c.c_lo);
    }
};

// ------------------------------------------------------------------ tri: hit_triangle, Moller-Trumbore, the certificate
struct TriK {
    isc::TriCase c;
    Quad nd;      // the stored plane, as the packer makes it (ptp::tri_plane)
};
inline TriK tri_k(const isc::TriCase& c) {
    float tr[16];
    isc::tri_record(c, tr);
    return TriK{c, ptp::tri_plane(tr)};
}
struct Tri {
    using Case = TriK;
    using Ctx = NoCtx;
    static constexpr int W = 3;
    static constexpr bool boolean = true, has_ref = true;
    static const char* name() { return "tri"; }
    PT_HD static void eval(const Case& k, const Ctx&, uint32_t* r) {
        const float* v = k.c.v;
        const f3 v0 = mk(v[0], v[1], v[2]), v1 = mk(v[3], v[4], v[5]), v2 = mk(v[6], v[7], v[8]), o = k.c.o, d = k.c.d;
        // (the edge tests inside are the twin of tri_edges_at, csrc/pt_render_sm.h)
        r[0] = fw(isc::kernel_hit_triangle(k.nd, v0, v1, v2, o, d));
        const Quad q0{v[0], v[1], v[2], 0.0f}, q1{v[3], v[4], v[5], 0.0f}, q2{v[6], v[7], v[8], 0.0f};
        r[1] = fw(pti::tri_mt(q0, q1, q2, o, d));
        // the certificate tri_edges_at evaluates at the same point, with the kernel's omax = max_j |o_j|
        const f3 p = o + d * pti::tri_plane(k.nd, o, d);
        r[2] = (uint32_t)ptw::leaf_certificate(p, mk(k.nd.x, k.nd.y, k.nd.z), v0, v1, v2, ptw::abs_max3(o));
    }
    static void ref(const Case& k, const Ctx&, const uint32_t* self, uint32_t* r) {
        float tr[16], nrm[3];
        isc::tri_record(k.c, tr);
        const float ov[3] = {k.c.o.x, k.c.o.y, k.c.o.z}, dv[3] = {k.c.d.x, k.c.d.y, k.c.d.z};
        r[0] = fw(oracle_hit_triangle(ov, dv, tr, nrm));
        r[1] = fw(oracle_mt_triangle(ov, dv, tr, nrm));
        r[2] = self[2];
    }
    static bool positive(const Case&, const uint32_t* r) { return pt::bitsf(r[0]) >= 0.0f; }
    static void nudge(Case& k) { k.c.o.x = step(k.c.o.x); }
    static void show(const Case& k) {
        const float* v = k.c.v;
        std::fprintf(stderr, "v0=(%a,%a,%a) v1=(%a,%a,%a) v2=(%a,%a,%a) o=(%a,%a,%a) d=(%a,%a,%a)", v[0], v[1], v[2], v[3], v[4], v[5],
                     v[6], v[7], v[8], k.c.o.x, k.c.o.y, k.c.o.z, k.c.d.x, k.c.d.y, k.c.d.z);
    }
};

// ------------------------------------------------------------------ aces
struct Aces {
    using Case = Quad;
    using Ctx = NoCtx;
    static constexpr int W = 1;
    static constexpr bool boolean = false, has_ref = true;
    static const char* name() { return "aces"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        const Rgba8 g = pti::aces_px<Rgba8>(c);
        r[0] = (uint32_t)g.x | (uint32_t)g.y << 8 | (uint32_t)g.z << 16 | (uint32_t)g.w << 24;
    }
    static void ref(const Case& c, const Ctx&, const uint32_t*, uint32_t* r) {
        unsigned char b[4];
        oracle_aces_rgba8(&c.x, 1, b);
        r[0] = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    }
    static bool positive(const Case&, const uint32_t* r) { return (r[0] & 0xffffffu) != 0u; }
    static void nudge(Case& c) { c.x = step(c.x); }
    static void show(const Case& c) { std::fprintf(stderr, "px=(%a,%a,%a,%a)", c.x, c.y, c.z, c.w); }
};

// ------------------------------------------------------------------ accumulate
struct Accum {
    using Case = isc::AccumCase;
    using Ctx = NoCtx;
    static constexpr int W = 4;
    static constexpr bool boolean = false, has_ref = true;
    static const char* name() { return "accumulate"; }
    PT_HD static void eval(const Case& a, const Ctx&, uint32_t* r) {
        const Quad g = pti::accumulate(Quad{a.pv[0], a.pv[1], a.pv[2], a.pv[3]}, mk(a.c[0], a.c[1], a.c[2]), a.frame, a.acc != 0);
        r[0] = fw(g.x), r[1] = fw(g.y), r[2] = fw(g.z), r[3] = fw(g.w);
    }
    static void ref(const Case& a, const Ctx&, const uint32_t*, uint32_t* r) {
        float want[4];
        isc::accumulate_definition(a, want);
        for (int q = 0; q < 4; q++) r[q] = fw(want[q]);
    }
    static bool positive(const Case& a, const uint32_t*) { return a.acc != 0; }
    static void nudge(Case& a) { a.pv[0] = step(a.pv[0]); a.c[0] = step(a.c[0]); }
    static void show(const Case& a) {
        std::fprintf(stderr, "prev=(%a,%a,%a,%a) rgb=(%a,%a,%a) frame %d acc %d", a.pv[0], a.pv[1], a.pv[2], a.pv[3], a.c[0], a.c[1],
                     a.c[2], a.frame, a.acc);
    }
};

// ------------------------------------------------------------------ noise
struct Quant {
    using Case = twc::QuantCase;
    using Ctx = NoCtx;
    static constexpr int W = 1;
    static constexpr bool boolean = true, has_ref = true;
    static const char* name() { return "noise_quantise"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) { r[0] = ptn::quantise(c.s1, c.s2, c.n); }
    // pt_noise.h: every operation a separately rounded binary32 operation -- each computed in double and rounded
    // once more (exact for + - * / and the square root of binary32 operands)
    static void ref(const Case& c, const Ctx&, const uint32_t*, uint32_t* r) {
        const float nf = (float)(double)c.n, m = isc::div32(c.s1, nf);
        const float d = isc::add32(isc::div32(c.s2, nf), -isc::mul32(m, m));
        const float v = d < 0.0f ? 0.0f : d;
        const float sem = (float)std::sqrt((double)isc::div32(v, (float)(double)(c.n - 1)));
        float rel = isc::div32(sem, isc::add32(m, 0.01f));
        if (!(rel >= 0.0f && rel <= 64.0f)) rel = 64.0f;
        r[0] = (unsigned)(double)isc::mul32(rel, 65536.0f);
    }
    static bool positive(const Case&, const uint32_t* r) { return r[0] < (64u << 16); }   // below the cap
    static void nudge(Case& c) { c.s2 = step(c.s2); }
    static void show(const Case& c) { std::fprintf(stderr, "s1=%a s2=%a n=%d", c.s1, c.s2, c.n); }
};
struct Target {
    using Case = twc::TargetCase;
    using Ctx = NoCtx;
    static constexpr int W = 2;
    static constexpr bool boolean = true, has_ref = false;
    static const char* name() { return "noise_target"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        r[0] = ptn::target_q(c.x);
        r[1] = c.q > r[0];       // the pixel counts as above the target
    }
    static void ref(const Case&, const Ctx&, const uint32_t* self, uint32_t* r) { r[0] = self[0], r[1] = self[1]; }
    static bool positive(const Case&, const uint32_t* r) { return r[1] != 0u; }
    static void nudge(Case& c) { c.q += 1u; }
    static void show(const Case& c) { std::fprintf(stderr, "x=%a q=%u", c.x, c.q); }
};
struct Retire {
    using Case = twc::RetireCase;
    using Ctx = NoCtx;
    static constexpr int W = 1;
    static constexpr bool boolean = true, has_ref = false;
    static const char* name() { return "noise_retire"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) { r[0] = ptn::tile_retires(c.sum_q, c.pixels, c.tq); }
    static void ref(const Case&, const Ctx&, const uint32_t* self, uint32_t* r) { r[0] = self[0]; }
    static bool positive(const Case&, const uint32_t* r) { return r[0] != 0u; }
    static void nudge(Case& c) { c.sum_q += 1ull; }
    static void show(const Case& c) { std::fprintf(stderr, "sum_q=%llu pixels=%llu tq=%u", c.sum_q, c.pixels, c.tq); }
};
struct Fold {
    using Case = twc::FoldCase;
    using Ctx = NoCtx;
    static constexpr int W = 2;
    static constexpr bool boolean = false, has_ref = true;
    static const char* name() { return "noise_fold"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        float s1 = 0.0f, s2 = 0.0f;
        for (int i = 0; i < 64; i++) ptn::add_sample(s1, s2, ptn::luminance(c.rgb[i][0], c.rgb[i][1], c.rgb[i][2]));
        r[0] = fw(s1), r[1] = fw(s2);
    }
    static void ref(const Case& c, const Ctx&, const uint32_t*, uint32_t* r) {
        float s1 = 0.0f, s2 = 0.0f;
        for (int i = 0; i < 64; i++) {
            const float y = isc::add32(isc::add32(isc::mul32(c.rgb[i][0], 0.2126f), isc::mul32(c.rgb[i][1], 0.7152f)), isc::mul32(c.rgb[i][2], 0.0722f));
            s1 = isc::add32(s1, y);
            s2 = isc::add32(s2, isc::mul32(y, y));
        }
        r[0] = fw(s1), r[1] = fw(s2);
    }
    static bool positive(const Case&, const uint32_t* r) { return pt::bitsf(r[0]) > 1.0f; }
    static void nudge(Case& c) { c.rgb[63][1] = step(c.rgb[63][1]); }
    static void show(const Case& c) { std::fprintf(stderr, "rgb[0]=(%a,%a,%a) ...", c.rgb[0][0], c.rgb[0][1], c.rgb[0][2]); }
};

// ------------------------------------------------------------------ wide
struct WideHits {
    using Case = twc::WideHitsCase;
    using Ctx = NoCtx;
    static constexpr int W = 10;
    static constexpr bool boolean = true, has_ref = false;
    static const char* name() { return "wide_hits"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        const f3 rd = rcp3(c.d);
        const ptw::WRay wr = ptw::make_wray(c.o, rd, c.cw, rd.x < 0.0f, rd.y < 0.0f, rd.z < 0.0f);
        r[0] = ptw::wide_hits(c.O[0], c.O[1], c.O[2], c.w, c.a[0], c.a[1], c.a[2], c.a[3], c.b[0], c.b[1], wr, c.t, c.s);
        r[1] = fw(wr.olx), r[2] = fw(wr.oly), r[3] = fw(wr.olz), r[4] = fw(wr.ohx), r[5] = fw(wr.ohy), r[6] = fw(wr.ohz);
        r[7] = fw(wr.rdx), r[8] = fw(wr.rdy), r[9] = fw(wr.rdz);
    }
    static void ref(const Case&, const Ctx&, const uint32_t* self, uint32_t* r) {
        for (int i = 0; i < W; i++) r[i] = self[i];
    }
    static bool positive(const Case&, const uint32_t* r) { return r[0] != 0u; }
    static void nudge(Case& c) { c.t = step(c.t); }
    static void show(const Case& c) {
        std::fprintf(stderr, "o=(%a,%a,%a) d=(%a,%a,%a) cw=(%a,%a,%a) O=(%a,%a,%a) w=%08x a=%08x %08x %08x %08x b=%08x %08x t=%a s=%d", c.o.x,
                     c.o.y, c.o.z, c.d.x, c.d.y, c.d.z, c.cw[0], c.cw[1], c.cw[2], c.O[0], c.O[1], c.O[2], c.w, c.a[0], c.a[1], c.a[2],
                     c.a[3], c.b[0], c.b[1], c.t, c.s);
    }
};
struct WideNext {
    using Case = twc::WideNextCase;
    using Ctx = NoCtx;
    static constexpr int K = ptw::kStack, W = K + 2;
    static constexpr bool boolean = false, has_ref = false;   // (positives: the flushing steps, at least 1%)
    static const char* name() { return "wide_next"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        uint32_t e[K];
        for (int k = 0; k < K; k++) e[k] = c.e[k];
        int R = c.R;
        // two call sites, as in the kernels: wide_visit in the record loop, wide_pop after a leaf
        int next;
        if (c.op == 0) next = ptw::wide_visit<K>(c.cur, c.pend, c.cbase, c.exit_, e, R);
        else next = ptw::wide_pop<K>(e, R);
        for (int k = 0; k < K; k++) r[k] = e[k];
        r[K] = (uint32_t)R;
        r[K + 1] = (uint32_t)next;
    }
    static void ref(const Case&, const Ctx&, const uint32_t* self, uint32_t* r) {
        for (int i = 0; i < W; i++) r[i] = self[i];
    }
    static bool positive(const Case& c, const uint32_t*) { return c.flush != 0; }
    static void nudge(Case& c) { c.pend ^= 1u; }
    static void show(const Case& c) {
        std::fprintf(stderr, "op=%d cur=%d pend=%02x cbase=%d exit=%d R=%d e=", c.op, c.cur, c.pend, c.cbase, c.exit_, c.R);
        for (int k = 0; k < K; k++) std::fprintf(stderr, "%08x ", c.e[k]);
    }
};

// ------------------------------------------------------------------ math
struct Rng {
    using Case = twc::RngCase;
    using Ctx = NoCtx;
    static constexpr int W = 10;
    static constexpr bool boolean = false, has_ref = false;
    static const char* name() { return "math_rng"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        r[0] = pt::seed(c.x, c.y, c.frame);
        uint32_t s = c.s;
        r[1] = pt::next_random(s);
        r[2] = s;
        s = c.s;
        r[3] = fw(pt::random01(s));
        s = c.s;
        r[4] = fw(pt::random_normal(s));
        r[5] = s;
        s = c.s;
        const f3 u = pt::random_unit_vector(s);
        r[6] = fw(u.x), r[7] = fw(u.y), r[8] = fw(u.z);
        r[9] = s;
    }
    static void ref(const Case&, const Ctx&, const uint32_t* self, uint32_t* r) {
        for (int i = 0; i < W; i++) r[i] = self[i];
    }
    static bool positive(const Case&, const uint32_t* r) { return pt::bitsf(r[4]) > 0.0f; }
    static void nudge(Case& c) { c.s ^= 1u; c.x ^= 1; }
    static void show(const Case& c) { std::fprintf(stderr, "s=%08x x=%d y=%d frame=%d", c.s, c.x, c.y, c.frame); }
};
struct Vec {
    using Case = twc::VecCase;
    using Ctx = NoCtx;
    static constexpr int W = 10;
    static constexpr bool boolean = false, has_ref = false;   // (positives: dot(a, a) inside the fast forms' guard)
    static const char* name() { return "math_vec"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        const f3 n = pt::normalize(c.a);
        r[0] = fw(n.x), r[1] = fw(n.y), r[2] = fw(n.z);
        r[3] = fw(pt::length(c.a));
        r[4] = fw(pt::sqrt_g(pt::dot(c.b, c.b)));
        r[5] = fw(pt::div_g(c.a.x, c.b.x));
        r[6] = fw(pt::div_g(c.b.y, c.a.y));
        const f3 m = pt::mix(c.a, c.b, c.s);
        r[7] = fw(m.x), r[8] = fw(m.y), r[9] = fw(m.z);
    }
    static void ref(const Case&, const Ctx&, const uint32_t* self, uint32_t* r) {
        for (int i = 0; i < W; i++) r[i] = self[i];
    }
    static bool positive(const Case& c, const uint32_t*) { return pt::fast_range(pt::dot(c.a, c.a)); }
    static void nudge(Case& c) { c.a.x = step(c.a.x); c.a.y = step(c.a.y); }
    static void show(const Case& c) {
        std::fprintf(stderr, "a=(%a,%a,%a) b=(%a,%a,%a) s=%a", c.a.x, c.a.y, c.a.z, c.b.x, c.b.y, c.b.z, c.s);
    }
};

// ------------------------------------------------------------------ what the render shares with the ray-batch units
struct Guard {
    using Case = twc::GuardCase;
    using Ctx = NoCtx;
    static constexpr int W = 1;
    static constexpr bool boolean = true, has_ref = true;
    static const char* name() { return "guard"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) { r[0] = (uint32_t)pti::ray_in_guard(c.scene_fast != 0, c.o, c.d); }
    // the float compares of tests/ref_walk.h against the bit-pattern windows
    static void ref(const Case& c, const Ctx&, const uint32_t*, uint32_t* r) { r[0] = c.scene_fast != 0 && ref::in_guard(c.o, c.d); }
    static bool positive(const Case&, const uint32_t* r) { return r[0] & 1u; }
    static void nudge(Case& c) { c.d.x = step(c.d.x); c.o.y = step(c.o.y); }
    static void show(const Case& c) {
        std::fprintf(stderr, "o=(%a,%a,%a) d=(%a,%a,%a) scene_fast=%d", c.o.x, c.o.y, c.o.z, c.d.x, c.d.y, c.d.z, c.scene_fast);
    }
};
struct Sphere {
    using Case = twc::SphereCase;
    using Ctx = NoCtx;
    static constexpr int W = 1;   // t as a word
    // boolean only in that its positives (a distance a segment at t = +inf takes) are held to the 1%-99% check
    static constexpr bool boolean = true, has_ref = true;
    static const char* name() { return "sphere"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        r[0] = fw(pti::sphere_t(Quad{c.c[0], c.c[1], c.c[2], c.r * c.r}, c.o, c.d));   // r * r: the packer's quad 0
    }
    static void ref(const Case& c, const Ctx&, const uint32_t*, uint32_t* r) {
        const float ov[3] = {c.o.x, c.o.y, c.o.z}, dv[3] = {c.d.x, c.d.y, c.d.z}, sp[4] = {c.c[0], c.c[1], c.c[2], c.r};
        r[0] = fw(oracle_hit_sphere(ov, dv, sp));
    }
    static bool positive(const Case&, const uint32_t* r) { return pt::bitsf(r[0]) > 0.0001f; }   // a hit a segment at t = +inf takes
    static void nudge(Case& c) { c.o.x = step(c.o.x); c.o.y = step(c.o.y); }
    static void show(const Case& c) {
        std::fprintf(stderr, "c=(%a,%a,%a) r=%a o=(%a,%a,%a) d=(%a,%a,%a)", c.c[0], c.c[1], c.c[2], c.r, c.o.x, c.o.y, c.o.z, c.d.x, c.d.y, c.d.z);
    }
};
struct LeafChoice {
    using Case = twc::LeafChoiceCase;
    using Ctx = NoCtx;
    static constexpr int W = 1;
    static constexpr bool boolean = true, has_ref = true;
    static const char* name() { return "leaf_choice"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        const pti::LeafChoice lc = pti::leaf_choice(c.h1, c.h2, c.t);
        r[0] = (uint32_t)lc.c1 | (uint32_t)lc.c2 << 1;
    }
    // the reference's two ifs (tests/ref_walk.h)
    static void ref(const Case& c, const Ctx&, const uint32_t*, uint32_t* r) { r[0] = (uint32_t)ref::choose(c.h1, c.h2, c.t); }
    static bool positive(const Case&, const uint32_t* r) { return r[0] != 0u; }
    static void nudge(Case& c) { c.t = step(c.t); }
    static void show(const Case& c) { std::fprintf(stderr, "h1=%a h2=%a t=%a", c.h1, c.h2, c.t); }
};
struct Pinhole {
    using Case = twc::PinholeCase;
    using Ctx = NoCtx;
    static constexpr int W = 5;
    static constexpr bool boolean = false, has_ref = true;
    static const char* name() { return "pinhole"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        const float u = pti::film_coord((float)c.x + c.ax, (float)c.W, c.rW);
        const float v = pti::film_coord((float)c.y + c.ay, (float)c.H, c.rH);
        const f3 D = pti::pinhole_dir(c.fwd, c.right, c.up, u, v);
        r[0] = fw(u), r[1] = fw(v), r[2] = fw(D.x), r[3] = fw(D.y), r[4] = fw(D.z);
    }
    // the film coordinates by the division the reference writes (:536-537) and the direction of :539, every
    // operation computed in double and rounded once
    static void ref(const Case& c, const Ctx&, const uint32_t*, uint32_t* r) {
        const float u = isc::add32(isc::div32(isc::add32((float)c.x, c.ax), (float)c.W), -0.5f);
        const float v = isc::add32(isc::div32(isc::add32((float)c.y, c.ay), (float)c.H), -0.5f);
        const float f[3] = {c.fwd.x, c.fwd.y, c.fwd.z}, rt[3] = {c.right.x, c.right.y, c.right.z}, up[3] = {c.up.x, c.up.y, c.up.z};
        r[0] = fw(u), r[1] = fw(v);
        for (int q = 0; q < 3; q++) r[2 + q] = fw(isc::add32(isc::add32(f[q], isc::mul32(rt[q], u)), isc::mul32(up[q], v)));
    }
    static bool positive(const Case&, const uint32_t* r) { return pt::bitsf(r[0]) > 0.0f; }   // right of the centre column
    static void nudge(Case& c) { c.x ^= 1; c.up.z = step(c.up.z); }
    static void show(const Case& c) {
        std::fprintf(stderr, "x=%d y=%d W=%d H=%d ax=%a ay=%a fwd=(%a,%a,%a) right=(%a,%a,%a) up=(%a,%a,%a)", c.x, c.y, c.W, c.H, c.ax, c.ay,
                     c.fwd.x, c.fwd.y, c.fwd.z, c.right.x, c.right.y, c.right.z, c.up.x, c.up.y, c.up.z);
    }
};
struct SkyDepth {
    using Case = twc::SkyDepthCase;
    using Ctx = NoCtx;
    static constexpr int W = 4;
    static constexpr bool boolean = false, has_ref = false;
    static const char* name() { return "sky_depth"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        const f3 env = pti::sky(c.d, c.no_sky != 0);
        r[0] = fw(env.x), r[1] = fw(env.y), r[2] = fw(env.z);
        r[3] = fw(pti::depth_term(c.hitp, c.o));
    }
    static void ref(const Case&, const Ctx&, const uint32_t* self, uint32_t* r) {
        for (int i = 0; i < W; i++) r[i] = self[i];
    }
    static bool positive(const Case& c, const uint32_t*) { return c.no_sky == 0; }
    static void nudge(Case& c) { c.d.z = step(c.d.z); c.hitp.y = step(c.hitp.y); }
    static void show(const Case& c) {
        std::fprintf(stderr, "d=(%a,%a,%a) hitp=(%a,%a,%a) o=(%a,%a,%a) no_sky=%d", c.d.x, c.d.y, c.d.z, c.hitp.x, c.hitp.y, c.hitp.z, c.o.x,
                     c.o.y, c.o.z, c.no_sky);
    }
};
// the twin's material table: quads {colour, smoothness}, {emission, specular probability}, {specular colour, 0}
struct TwinMats {
    PT_HD Quad mat(int i, int k) const {
        const float T[twc::kTwinMats][12] = {
            {0.73f, 0.73f, 0.73f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, 0.0f},          // diffuse white
            {0.65f, 0.05f, 0.05f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, 0.0f},          // diffuse red
            {0.0f, 0.0f, 0.0f, 0.0f, 15.0f, 15.0f, 15.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f},          // a light
            {0.9f, 0.9f, 0.9f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.95f, 0.95f, 0.95f, 0.0f},          // a mirror
            {0.12f, 0.45f, 0.15f, 0.6f, 0.0f, 0.0f, 0.0f, 0.5f, 1.0f, 0.9f, 0.8f, 0.0f},          // glossy, half the bounces
            {0.5f, 0.5f, 0.5f, 0.25f, 0.3f, 0.2f, 0.1f, 0x1p-32f, 0.5f, 0.5f, 0.5f, 0.0f}};       // specular at one draw only
        return Quad{T[i][4 * k], T[i][4 * k + 1], T[i][4 * k + 2], T[i][4 * k + 3]};
    }
};
struct Bounce {
    using Case = twc::BounceCase;
    using Ctx = NoCtx;
    static constexpr int W = 18;
    static constexpr bool boolean = false, has_ref = false;
    static const char* name() { return "bounce"; }
    PT_HD static void eval(const Case& c, const Ctx&, uint32_t* r) {
        f3 o = c.o, d = c.d, inc = c.inc, col = c.col, rgb = c.inc;      // rgb = inc: as the callers enter it
        uint32_t state = c.state;
        int bounce = c.bounce;
        const bool finished = pti::shade_hit<Quad>(TwinMats(), c.mat, c.normal, c.hitp, c.mode, c.max_bounce, o, d, inc, col, state, bounce, rgb);
        r[0] = fw(o.x), r[1] = fw(o.y), r[2] = fw(o.z), r[3] = fw(d.x), r[4] = fw(d.y), r[5] = fw(d.z);
        r[6] = fw(inc.x), r[7] = fw(inc.y), r[8] = fw(inc.z), r[9] = fw(col.x), r[10] = fw(col.y), r[11] = fw(col.z);
        r[12] = state, r[13] = (uint32_t)bounce, r[14] = (uint32_t)finished;
        r[15] = fw(rgb.x), r[16] = fw(rgb.y), r[17] = fw(rgb.z);
    }
    static void ref(const Case&, const Ctx&, const uint32_t* self, uint32_t* r) {
        for (int i = 0; i < W; i++) r[i] = self[i];
    }
    static bool positive(const Case&, const uint32_t* r) { return r[14] != 0u; }   // the path ended
    static void nudge(Case& c) { c.state ^= 1u; c.normal.x = step(c.normal.x); c.hitp.x = step(c.hitp.x); }
    static void show(const Case& c) {
        std::fprintf(stderr, "normal=(%a,%a,%a) hitp=(%a,%a,%a) o=(%a,%a,%a) d=(%a,%a,%a) inc=(%a,%a,%a) col=(%a,%a,%a) state=%08x bounce=%d max=%d mode=%d mat=%d",
                     c.normal.x, c.normal.y, c.normal.z, c.hitp.x, c.hitp.y, c.hitp.z, c.o.x, c.o.y, c.o.z, c.d.x, c.d.y, c.d.z, c.inc.x,
                     c.inc.y, c.inc.z, c.col.x, c.col.y, c.col.z, c.state, c.bounce, c.max_bounce, c.mode, c.mat);
    }
};

// ------------------------------------------------------------------ the whole case set
struct Cases {
    std::vector<isc::SlabCase> slab, slab_wild;
    std::vector<twc::CullCase> cull;
    twc::SweepTable sweep[twc::kSweepTables];
    std::vector<TriK> tri;
    std::vector<Quad> aces;
    std::vector<isc::AccumCase> accum;
    std::vector<twc::QuantCase> quant;
    std::vector<twc::TargetCase> target;
    std::vector<twc::RetireCase> retire;
    std::vector<twc::FoldCase> fold;
    std::vector<twc::WideHitsCase> wide_hits;
    std::vector<twc::WideNextCase> wide_next;
    std::vector<twc::RngCase> rng;
    std::vector<twc::VecCase> vec;
    std::vector<twc::GuardCase> guard;
    std::vector<twc::SphereCase> sphere;
    std::vector<twc::LeafChoiceCase> leaf_choice;
    std::vector<twc::PinholeCase> pinhole;
    std::vector<twc::SkyDepthCase> sky_depth;
    std::vector<twc::BounceCase> bounce;
    long dropped = 0, aces_boundaries = 0;   // cases a generator left its domain with (asserted 0)
};
// `div`: every count divided by it (the CPU test runs a fraction of the set; the device twin all of it)
inline void generate(Cases& C, long div) {
    isc::rs = isc::kSeed;
    auto cnt = [div](long n) { return (n + div - 1) / div | 1; };
    C.dropped += isc::slab_random(cnt(twc::kSlab), C.slab);
    std::vector<isc::TriCase> tris;
    isc::tri_random(cnt(twc::kTri), tris);
    for (const isc::TriCase& t : tris) C.tri.push_back(tri_k(t));
    std::vector<float> px;
    C.aces_boundaries = isc::aces_pixels(cnt(twc::kAces), px);
    for (size_t i = 0; i + 3 < px.size(); i += 4) C.aces.push_back(Quad{px[i], px[i + 1], px[i + 2], px[i + 3]});
    isc::accumulate_cases(C.accum, (int)cnt(twc::kAccumPerFrame));
    twc::slab_wild(cnt(twc::kSlabWild), C.slab_wild);
    C.dropped += twc::cull_cases(cnt(twc::kCull), C.cull);
    for (int w = 0; w < twc::kSweepTables; w++) C.dropped += twc::sweep_table(w, cnt(twc::kSweepRays), C.sweep[w]);
    twc::quant_cases(cnt(twc::kQuant), C.quant);
    twc::target_cases(cnt(twc::kTarget), C.target);
    twc::retire_cases(cnt(twc::kRetire), C.retire);
    twc::fold_cases(cnt(twc::kFold), C.fold);
    C.dropped += twc::wide_hits_cases(cnt(twc::kWideHits), C.wide_hits);
    twc::wide_next_cases(cnt(twc::kWideNext), C.wide_next);
    twc::rng_cases(cnt(twc::kRng), C.rng);
    twc::vec_cases(cnt(twc::kVec), C.vec);
    twc::guard_cases(cnt(twc::kGuard), C.guard);
    twc::sphere_cases(cnt(twc::kSphere), C.sphere);
    twc::leaf_choice_cases(cnt(twc::kLeafChoice), C.leaf_choice);
    twc::pinhole_cases(cnt(twc::kPinhole), C.pinhole);
    twc::sky_depth_cases(cnt(twc::kSkyDepth), C.sky_depth);
    twc::bounce_cases(cnt(twc::kBounce), C.bounce);
}
inline SweepCtx sweep_ctx(const twc::SweepTable& T, const Quad* table, bool flip) {
    SweepCtx x;
    x.table = table;
    x.n = T.n;
    for (int q = 0; q < 3; q++) x.cm[q] = T.cm[q], x.ws[q] = T.ws[q];
    x.flip = flip ? 1 : 0;
    return x;
}

}  // namespace twf
