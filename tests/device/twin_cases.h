// TEST INFRASTRUCTURE: the cases of the device twin (tests/device/device_twin.hip) beyond those of
// tests/isect/isect_cases.h: boxes and rays outside every guard for pti::slab, the culling test and the
// leaf sweep (pt_cull.h), the noise estimate (pt_noise.h), the wide walk (pt_wide.h), the guarded
// forms and the RNG of pt_math.h, and the per-ray arithmetic the render shares with the ray-batch units
// (pt_isect.h: the guard, the sphere distance, the leaf's choice, the camera ray, the sky and the bounce).  Plain C++, no HIP: tests/device/twin_host.cpp runs them on the CPU.
// Every generator seeds the stream itself, so its cases do not depend on what ran before it, and no expression draws
// twice, so they do not depend on the compiler either (isect_cases.h).
#pragma once

#include "../isect/isect_cases.h"
#include "../../opengl-path-tracing_amd/csrc/pt_noise.h"
#include "../../opengl-path-tracing_amd/csrc/pt_wide.h"

namespace twc {

using isc::gcoord;
using isc::mag;
using isc::nx;
using isc::sgn;
using isc::sym;
using isc::ulps;
using isc::uni;
using pt::f3;
using pt::mk;
using ptp::Quad;

inline void reseed(uint64_t k) { isc::rs = isc::kSeed ^ (k * 0x9e3779b97f4a7c15ull); }

// The default case counts of the device twin.  None is a multiple of 64: the last wave of every launch is partial.
constexpr long kSlab = 2000003, kTri = 1000003, kAces = 1000003, kAccumPerFrame = 20003, kAccum = 10 * (long)kAccumPerFrame;
constexpr long kSlabWild = 500009, kCull = 1000003, kSweepRays = 100003, kQuant = 300007, kTarget = 100003, kRetire = 100003;
constexpr long kFold = 20011, kWideHits = 500009, kWideNext = 1000003, kRng = (1l << 20) + 3, kVec = 500009;
constexpr long kGuard = 100003, kSphere = 100003, kLeafChoice = 100003, kPinhole = 100003, kSkyDepth = 100003, kBounce = 100003;
constexpr int kSweepTables = 5;
constexpr int kSweepN[kSweepTables] = {1, 2, 17, 24, 32};
constexpr bool partial(long n) { return n % 64 != 0; }
static_assert(partial(kSlab) && partial(kTri) && partial(kAces) && partial(kAccum) && partial(kSlabWild) && partial(kCull) &&
                  partial(kSweepRays) && partial(kQuant) && partial(kTarget) && partial(kRetire) && partial(kFold) &&
                  partial(kWideHits) && partial(kWideNext) && partial(kRng) && partial(kVec) && partial(kGuard) &&
                  partial(kSphere) && partial(kLeafChoice) && partial(kPinhole) && partial(kSkyDepth) && partial(kBounce),
              "a partial last wave in every launch");

// ------------------------------------------------------------------ slab_wild: pti::slab on any binary32
// Domain: every binary32 in every operand.  (slab is the IEEE chain the rays outside the guard run.)
inline float wild_value() {
    switch (nx() % 12) {
        case 0: return 0.0f;
        case 1: return -0.0f;
        case 2: return INFINITY;
        case 3: return -INFINITY;
        case 4: return NAN;
        case 5: { const float sg = sgn(); return sg * pt::bitsf(1u + (uint32_t)(nx() % 0x7fffffu)); }   // subnormal
        case 6: return sgn() * 0x1p-149f;
        case 7: { const float sg = sgn(), m = 1.0f + uni(); return sg * std::ldexp(m, 100 + (int)(nx() % 27)); }
        case 8: return sgn() * 0x1p127f;
        case 9: return sgn() * 0x1.fffffep127f;
        default: return mag(-126, 127);
    }
}
inline void slab_wild(long n, std::vector<isc::SlabCase>& out) {
    reseed(1);
    for (long k = 0; k < n; k++) {
        isc::SlabCase c;
        // a sane box and ray at one scale ...
        const float s = std::ldexp(1.0f, (int)(nx() % 41) - 20);
        float ov[3], dv[3];
        for (int q = 0; q < 3; q++) {
            c.lo[q] = s * sym();
            c.hi[q] = c.lo[q] + s * uni();
            ov[q] = 4.0f * s * sym();
            dv[q] = (c.lo[q] + (c.hi[q] - c.lo[q]) * uni()) - ov[q];
        }
        const uint64_t tk = nx() % 3;     // t: +inf, any, or (below) the entry distance and one ulp either side
        bool t_set = false;
        c.t = tk == 0 ? INFINITY : 8.0f * uni();
        // ... with up to four operands replaced: wild values, a zero numerator, a zero thickness
        for (int r = (int)(nx() % 5); r > 0; r--) {
            const int q = (int)(nx() % 3);
            switch (nx() % 8) {
                case 0: c.lo[q] = wild_value(); break;
                case 1: c.hi[q] = wild_value(); break;
                case 2: ov[q] = wild_value(); break;
                case 3: case 4: dv[q] = wild_value(); break;
                case 5: ov[q] = nx() % 2 ? c.lo[q] : c.hi[q]; break;     // the numerator is exactly 0
                case 6: c.hi[q] = c.lo[q]; break;                        // zero thickness
                default: c.t = nx() % 2 ? NAN : (nx() % 2 ? INFINITY : wild_value()); t_set = true; break;
            }
        }
        c.o = mk(ov[0], ov[1], ov[2]);
        c.d = mk(dv[0], dv[1], dv[2]);
        if (tk == 2 && !t_set) c.t = ulps(isc::near_quotient(c.lo, c.hi, c.o, c.d, -1), (int)(nx() % 3) - 1);
        out.push_back(c);
    }
}

// ------------------------------------------------------------------ cull: slab_oct_cons and sweep_hit
// Domain: a triple inside the exact-reciprocal guard, cm as the packer derives it (ptp::cons_margin) from a root
// box that contains the case's box, ws finite and >= 0, c_lo = ptc::kWindowLo or -inf.
struct CullCase {
    isc::SlabCase s;
    float cm[3], ws[3], c_lo;
};
inline void margins_of(const float lo[3], const float hi[3], float cm[3], float ws[3]) {
    float bvh[12] = {0};
    for (int q = 0; q < 3; q++) {       // a root box around the case's box, up to 8 times as far out
        const float grow = 1.0f + 7.0f * uni();
        bvh[q] = std::fmin(lo[q], -std::fabs(lo[q]) * grow);
        bvh[4 + q] = std::fmax(hi[q], std::fabs(hi[q]) * grow);
    }
    ptp::cons_margin(bvh, cm);
    for (int q = 0; q < 3; q++)         // the window slack: 0, or of the order window_slack gives (a few u M)
        ws[q] = nx() % 4 == 0 ? 0.0f : 0x1p-20f * uni() * std::fmax(std::fabs(bvh[q]), std::fabs(bvh[4 + q]));
}
// the near value of a box for a ray, as cull_hit and sweep_hit form it (lo, hi in the reference order): the t at
// which the conservative verdict turns
inline float cons_near(const float lo[3], const float hi[3], const float cm[3], const float ws[3], f3 o, f3 d, float c_lo) {
    const f3 rd = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    f3 ol, oh;
    ptc::cull_addends(o, rd, cm, ws, ol, oh);
    const ptc::SweepRay r = ptc::sweep_ray(rd, ol, oh);
    const float xn = __builtin_fmaf(lo[0], r.rp.x, __builtin_fmaf(hi[0], r.rn.x, r.ol.x));
    const float yn = __builtin_fmaf(lo[1], r.rp.y, __builtin_fmaf(hi[1], r.rn.y, r.ol.y));
    const float zn = __builtin_fmaf(lo[2], r.rp.z, __builtin_fmaf(hi[2], r.rn.z, r.ol.z));
    return fmaxf(fmaxf(fmaxf(xn, yn), zn), c_lo);
}
inline long cull_cases(long n, std::vector<CullCase>& out) {
    reseed(2);
    std::vector<isc::SlabCase> slabs;
    const long outside = isc::slab_random(n, slabs);
    for (const isc::SlabCase& s : slabs) {
        CullCase c;
        c.s = s;
        margins_of(s.lo, s.hi, c.cm, c.ws);
        c.c_lo = nx() % 2 ? ptc::kWindowLo : -INFINITY;
        if (nx() % 4 == 0)      // t at the conservative test's own near value and one ulp either side
            c.s.t = ulps(cons_near(s.lo, s.hi, c.cm, c.ws, s.o, s.d, c.c_lo), (int)(nx() % 3) - 1);
        out.push_back(c);
    }
    return outside;
}

// ------------------------------------------------------------------ sweep: one table per launch
// Domain: n <= 32 boxes with lo <= hi inside the guard's scene half, rays inside the guard, t not NaN.
struct SweepRayCase {
    f3 o, d;
    float t, c_lo;
};
struct SweepTable {
    int n = 0;
    std::vector<Quad> quads;   // 2 per entry: {lo.x, hi.x, lo.y, hi.y}, {lo.z, hi.z, pair, inverse}
    float cm[3], ws[3];
    std::vector<SweepRayCase> rays;
};
// the near value of table entry k for a ray
inline float sweep_near(const SweepTable& T, int k, f3 o, f3 d, float c_lo) {
    const Quad a = T.quads[2 * k], b = T.quads[2 * k + 1];
    const float lo[3] = {a.x, a.z, b.x}, hi[3] = {a.y, a.w, b.y};
    return cons_near(lo, hi, T.cm, T.ws, o, d, c_lo);
}
inline long sweep_table(int which, long n_rays, SweepTable& T) {
    reseed(16 + (uint64_t)which);
    T.n = kSweepN[which];
    const float s = std::ldexp(1.0f, 3 * which - 4);      // a scale per table
    float rlo[3] = {INFINITY, INFINITY, INFINITY}, rhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < T.n; k++) {
        float lo[3], hi[3];
        for (int q = 0; q < 3; q++) {
            lo[q] = s * sym();
            hi[q] = lo[q] + (nx() % 8 == 0 ? 0.0f : s * uni());     // flat now and then
            rlo[q] = std::fmin(rlo[q], lo[q]);
            rhi[q] = std::fmax(rhi[q], hi[q]);
        }
        T.quads.push_back(Quad{lo[0], hi[0], lo[1], hi[1]});
        T.quads.push_back(Quad{lo[2], hi[2], (float)k, (float)k});
    }
    margins_of(rlo, rhi, T.cm, T.ws);
    long outside = 0;
    for (long i = 0; i < n_rays; i++) {
        SweepRayCase r;
        float ov[3], dv[3];
        const int aim = (int)(nx() % (uint64_t)T.n);
        const Quad a = T.quads[2 * aim], b = T.quads[2 * aim + 1];
        const float blo[3] = {a.x, a.z, b.x}, bhi[3] = {a.y, a.w, b.y};
        const uint64_t kind = nx() % 4;
        for (int q = 0; q < 3; q++) {
            const float reach = nx() % 4 == 0 ? 8.0f : 2.0f;
            ov[q] = isc::gclamp(reach * s * sym());
            const float tg = blo[q] + (bhi[q] - blo[q]) * uni();
            dv[q] = kind == 0 ? sym() : tg - ov[q];               // any direction, or at (kind 1: away from) a box
            if (kind == 1) dv[q] = -dv[q];
        }
        f3 dd = mk(dv[0], dv[1], dv[2]);
        if (!(pt::dot(dd, dd) > 0.0f)) dd = mk(1.0f, 1.0f, 1.0f);
        dd = pt::normalize(dd);
        r.o = mk(ov[0], ov[1], ov[2]);
        r.d = mk(isc::dclamp(dd.x), isc::dclamp(dd.y), isc::dclamp(dd.z));
        r.c_lo = nx() % 2 ? ptc::kWindowLo : -INFINITY;
        // t: +inf, any scale, or a box's own near value and one ulp either side
        const uint64_t tk = nx() % 8;
        if (tk == 0) r.t = INFINITY;
        else if (tk <= 4) {
            const int k = (int)(nx() % (uint64_t)T.n), u = (int)(nx() % 3) - 1;
            r.t = ulps(sweep_near(T, k, r.o, r.d, r.c_lo), u);
        }
        else r.t = std::fabs(mag(-6, 6)) * s;
        bool in = r.t == r.t;
        const float oo[3] = {r.o.x, r.o.y, r.o.z}, od[3] = {r.d.x, r.d.y, r.d.z};
        for (int q = 0; q < 3; q++) in = in && pt::in_guard(oo[q], 0x1p-40f, 0x1p60f) && pt::in_range_abs(od[q], 0x1p-20f, 2.0f);
        if (in) T.rays.push_back(r);
        else outside++;
    }
    return outside;
}

// ------------------------------------------------------------------ noise
// quantise.  Domain: any binary32 moments, n >= 2.
struct QuantCase {
    float s1, s2;
    int n;
};
inline float moment_special() {
    const float v[] = {0.0f, -0.0f, NAN, INFINITY, -INFINITY, -1.0f, -0x1p-149f, 0x1p-149f, 0x1.fffffep127f, 1.0f};
    return v[nx() % 10];
}
inline void quant_cases(long n, std::vector<QuantCase>& out) {
    reseed(3);
    const int ns[] = {2, 3, 64, 4096, (1 << 24) + 1};
    for (long k = 0; k < n; k++) {
        QuantCase c;
        c.n = ns[nx() % 5];
        const float nf = (float)c.n, mean = nx() % 4 == 0 ? std::fabs(mag(-20, 4)) : 2.0f * uni();
        const uint64_t kind = nx() % 8;
        if (kind == 0) {            // special moments
            c.s1 = nx() % 2 ? moment_special() : mean * nf;
            c.s2 = nx() % 2 ? moment_special() : mean * mean * nf;
        } else if (kind == 1) {     // a mean at and either side of -0.01
            c.s1 = ulps(-0.01f * nf, (int)(nx() % 7) - 3);
            c.s2 = uni() * nf;
        } else if (kind == 2) {     // no variance: s2 / n - m^2 rounds to zero or just beside it
            c.s1 = mean * nf;
            const float m = c.s1 / nf;
            c.s2 = ulps((m * m) * nf, (int)(nx() % 9) - 4);
        } else if (kind == 3) {     // a relative error at 64 and beside it: sem = 64 (m + 0.01), v = sem^2 (n - 1)
            c.s1 = mean * nf;
            const float m = c.s1 / nf, sem = 64.0f * (m + 0.01f), v = sem * sem * (float)(c.n - 1);
            c.s2 = ulps((v + m * m) * nf, (int)(nx() % 9) - 4);
        } else {                    // a render's moments: n luminances around the mean
            const float spread = uni() * uni();
            c.s1 = mean * nf;
            c.s2 = (mean * mean) * (1.0f + spread * spread * (nx() % 4 == 0 ? 4096.0f : 1.0f)) * nf;
        }
        out.push_back(c);
    }
}
// target_q and the comparison it exists for.  Domain: any binary32 target, any q.
struct TargetCase {
    float x;
    unsigned q;
};
inline void target_cases(long n, std::vector<TargetCase>& out) {
    reseed(4);
    const float xs[] = {0.0f, -0.0f, -1.0f, NAN, INFINITY, 64.0f, 0x1.fffffep5f, 0x1.000002p6f, 100.0f, 0.05f, 0x1p-16f, 0x1.fffffep-17f, 1.0f};
    for (long k = 0; k < n; k++) {
        TargetCase c;
        c.x = nx() % 4 == 0 ? xs[nx() % 13] : (nx() % 2 ? uni() : 64.0f * uni());
        const unsigned tq = ptn::target_q(c.x);
        c.q = nx() % 4 == 0 ? (unsigned)(nx() % (1u << 23)) : tq + (unsigned)(nx() % 3) - 1u;   // either side of target_q (wraps at 0)
        out.push_back(c);
    }
}
// tile_retires at its own threshold +-1.  Domain: sum_q <= pixels * 2^22, tq <= 2^22.
struct RetireCase {
    unsigned long long sum_q, pixels;
    unsigned tq;
};
inline void retire_cases(long n, std::vector<RetireCase>& out) {
    reseed(5);
    for (long k = 0; k < n; k++) {
        RetireCase c;
        c.pixels = nx() % 8 == 0 ? nx() % (1ull << 32) : 1 + nx() % 4096;
        c.tq = nx() % 8 == 0 ? (1u << 22) : (unsigned)(nx() % (1u << 22));
        const unsigned long long th = (unsigned long long)c.tq * c.pixels;
        c.sum_q = nx() % 4 == 0 ? nx() % (c.pixels * (1ull << 22) + 1) : th + (nx() % 3) - 1ull;
        if (c.sum_q > c.pixels * (1ull << 22)) c.sum_q = th;   // (th - 1 wrapped at th = 0)
        out.push_back(c);
    }
}
// 64 frame colours -> luminance -> add_sample in frame order.  Domain: any binary32.
struct FoldCase { float rgb[64][3]; };
inline void fold_cases(long n, std::vector<FoldCase>& out) {
    reseed(6);
    for (long k = 0; k < n; k++) {
        FoldCase c;
        const float level = nx() % 4 == 0 ? std::fabs(mag(-30, 30)) : 1.0f;
        for (auto& p : c.rgb)
            for (float& v : p) v = nx() % 64 == 0 ? 0.0f : level * (nx() % 16 == 0 ? 64.0f * uni() : uni());
        if (nx() % 32 == 0) {
            const float v = moment_special();
            const int i = (int)(nx() % 64), q = (int)(nx() % 3);
            c.rgb[i][q] = v;
        }
        out.push_back(c);
    }
}

// ------------------------------------------------------------------ wide: make_wray + wide_hits
// Domain: a ray inside the guard; a record whose box lies inside the scene half of the guard, exponents as
// pt_wide.cpp's axis_exp gives them (255 * 2^e spans the axis), cw = 2^-18 M rounded up; t not NaN.
struct WideHitsCase {
    f3 o, d;
    float cw[3], O[3];
    uint32_t w, a[4], b[2];
    float t;
    int s;
};
// the near value of child j, as wide_hits forms it
inline float wide_child_near(const WideHitsCase& c, int j) {
    const f3 rd = mk(1.0f / c.d.x, 1.0f / c.d.y, 1.0f / c.d.z);
    const ptw::WRay r = ptw::make_wray(c.o, rd, c.cw, rd.x < 0.0f, rd.y < 0.0f, rd.z < 0.0f);
    const int ex = (int)(int8_t)(c.w & 0xffu), ey = (int)(int8_t)((c.w >> 8) & 0xffu), ez = (int)(int8_t)((c.w >> 16) & 0xffu);
    const float Bx = ptw::ldexp2(r.rdx, ex), By = ptw::ldexp2(r.rdy, ey), Bz = ptw::ldexp2(r.rdz, ez);
    const float x = __builtin_fmaf(ptw::ubyte(r.sx ? c.a[1] : c.a[0], j), Bx, __builtin_fmaf(c.O[0], r.rdx, r.olx));
    const float y = __builtin_fmaf(ptw::ubyte(r.sy ? c.a[3] : c.a[2], j), By, __builtin_fmaf(c.O[1], r.rdy, r.oly));
    const float z = __builtin_fmaf(ptw::ubyte(r.sz ? c.b[1] : c.b[0], j), Bz, __builtin_fmaf(c.O[2], r.rdz, r.olz));
    return ptw::max3(x, y, z);
}
inline long wide_hits_cases(long n, std::vector<WideHitsCase>& out) {
    reseed(7);
    long outside = 0;
    for (long k = 0; k < n; k++) {
        WideHitsCase c;
        const float s = std::ldexp(1.0f, (int)(nx() % 61) - 20);
        float ext[3], ov[3], dv[3];
        int e[3];
        c.w = 0u;
        for (int q = 0; q < 3; q++) {
            c.O[q] = isc::gclamp(4.0f * s * sym());
            ext[q] = s * (0.25f + uni());
            e[q] = (int)std::ceil(std::log2((double)ext[q] / 255.0));      // axis_exp's start; +1 now and then
            if (nx() % 8 == 0) e[q]++;
            c.w |= ((uint32_t)e[q] & 0xffu) << (8 * q);
            const double M = std::fabs((double)c.O[q]) + 255.0 * std::ldexp(1.0, e[q]);
            float cw = (float)std::ldexp(M * (1.0 + 3.0 * uni()), -18);
            if ((double)cw < std::ldexp(M, -18)) cw = std::nextafterf(cw, INFINITY);
            c.cw[q] = cw;
        }
        c.w |= (uint32_t)(nx() & 0xffu) << 24;                              // the children's types: any byte
        uint32_t* words[6] = {&c.a[0], &c.a[1], &c.a[2], &c.a[3], &c.b[0], &c.b[1]};
        for (int q = 0; q < 3; q++) {
            uint32_t lo = 0u, hi = 0u;
            for (int j = 0; j < 4; j++) {
                uint32_t l = (uint32_t)(nx() % 256), h = (uint32_t)(nx() % 256);
                if (nx() % 8 == 0) l = nx() % 2 ? 0u : 255u;
                if (nx() % 8 == 0) h = nx() % 2 ? 0u : 255u;
                if (l > h) std::swap(l, h);
                lo |= l << (8 * j);
                hi |= h << (8 * j);
            }
            *words[2 * q] = lo;
            *words[2 * q + 1] = hi;
        }
        const int aim = (int)(nx() % 4);
        const uint64_t kind = nx() % 4;
        for (int q = 0; q < 3; q++) {
            const float reach = nx() % 4 == 0 ? 16.0f : 2.0f;
            ov[q] = isc::gclamp(c.O[q] + reach * s * sym());
            const float l = ptw::ubyte(*words[2 * q], aim), h = ptw::ubyte(*words[2 * q + 1], aim);
            const float tg = c.O[q] + std::ldexp(l + (h - l) * uni(), e[q]);
            dv[q] = kind == 0 ? sym() : tg - ov[q];
        }
        f3 dd = mk(dv[0], dv[1], dv[2]);
        if (!(pt::dot(dd, dd) > 0.0f) || !(pt::dot(dd, dd) < INFINITY)) dd = mk(1.0f, -1.0f, 1.0f);
        dd = pt::normalize(dd);
        c.o = mk(ov[0], ov[1], ov[2]);
        c.d = mk(isc::dclamp(dd.x), isc::dclamp(dd.y), isc::dclamp(dd.z));
        c.s = (int)(nx() % 4);
        const uint64_t tk = nx() % 8;
        if (tk == 0) c.t = INFINITY;
        else if (tk <= 4) {
            const int j = (int)(nx() % 4), u = (int)(nx() % 3) - 1;
            c.t = ulps(wide_child_near(c, j), u);
        }
        else c.t = std::fabs(mag(-4, 6)) * s;
        bool in = c.t == c.t;
        const float od[3] = {c.d.x, c.d.y, c.d.z};
        for (int q = 0; q < 3; q++)
            in = in && pt::in_guard(ov[q], 0x1p-40f, 0x1p60f) && pt::in_guard(c.O[q], 0x1p-40f, 0x1p60f) && pt::in_range_abs(od[q], 0x1p-20f, 2.0f);
        if (in) out.push_back(c);
        else outside++;
    }
    return outside;
}

// ------------------------------------------------------------------ wide: the walk state
// Domain: states a walk reaches.  Each sequence starts from the empty stack at the root and follows the positions
// wide_visit / wide_pop return, with random hits at every record; the state before each step is a case.
// Case i belongs to sequence i % kWideSeqs, so the 64 lanes of a wave hold 64 different walks.
constexpr int kWideSeqs = 4099;
struct WideNextCase {
    int cur, cbase, exit_, R;
    uint32_t pend, e[ptw::kStack];
    int op;       // 0: wide_visit, 1: wide_pop
    int flush;    // the step pushes onto a full stack (for the coverage counts only)
};
inline uint32_t random_pend(int s) {   // the hit children at slots >= s: types 1..3, 2 bits per slot
    uint32_t p = 0u;
    const uint64_t dense = nx() % 4;
    for (int j = s; j < 4; j++)
        if (nx() % 4 < 1 + dense) p |= (uint32_t)(1 + nx() % 3) << (2 * j);
    return p;
}
inline void wide_next_cases(long n, std::vector<WideNextCase>& out) {
    reseed(8);
    struct Seq { int cur = 0, R = -1; uint32_t e[ptw::kStack] = {}; };
    std::vector<Seq> seqs(kWideSeqs);
    for (long i = 0; i < n; i++) {
        Seq& q = seqs[(size_t)(i % kWideSeqs)];
        if (q.cur == -1) q = Seq();                         // the walk ended: another one from the root
        WideNextCase c;
        c.cur = q.cur;
        c.R = q.R;
        for (int k = 0; k < ptw::kStack; k++) c.e[k] = q.e[k];
        if (q.cur >= 0) {                                   // at a record: its hits, its children, its exit
            c.op = 0;
            c.pend = random_pend(q.cur & 7);
            c.cbase = (int)(nx() % (uint64_t)(ptw::kMaxRecords - 4));
            c.exit_ = -1;
            if (nx() % 8 != 0) {
                const uint64_t rec = nx() % (uint64_t)ptw::kMaxRecords, slot = 1 + nx() % 4;
                c.exit_ = (int)((rec << 3) | slot);
            }
            int kids = 0;
            for (int j = 0; j < 4; j++) kids += ((c.pend >> (2 * j)) & 3u) != 0u;
            c.flush = kids >= 2 && c.e[ptw::kStack - 1] != 0u;
            q.cur = ptw::wide_visit<ptw::kStack>(c.cur, c.pend, c.cbase, c.exit_, q.e, q.R);
        } else {                                            // stopped at a leaf: the next position from the stack
            c.op = 1;
            c.pend = 0u;
            c.cbase = 0;
            c.exit_ = 0;
            c.flush = 0;
            q.cur = ptw::wide_pop<ptw::kStack>(q.e, q.R);
        }
        out.push_back(c);
    }
}

// ------------------------------------------------------------------ math
// RNG states (any uint32) and pixel coordinates of seed.
struct RngCase {
    uint32_t s;
    int x, y, frame;
};
inline void rng_cases(long n, std::vector<RngCase>& out) {
    reseed(9);
    for (long k = 0; k < n; k++) {
        RngCase c;
        c.s = k < 4 ? (uint32_t)(0u - (uint32_t)k) : (uint32_t)nx();
        c.x = (int)(nx() % 8192);
        c.y = (int)(nx() % 8192);
        c.frame = nx() % 4 == 0 ? (1 << 24) + 1 : (int)(nx() % 100000);
        out.push_back(c);
    }
}
// Vectors whose dot(a, a) straddles 2^-100 and 2^100 (where normalize, length and sqrt_g switch between the fast
// and the IEEE forms), and operands of div_g at and beside 2^-60 and 2^60 (where it does).  Domain: finite binary32.
struct VecCase {
    f3 a, b;
    float s;
};
inline float edge_mag(int e) {
    const float sg = sgn();
    return sg * ulps(std::ldexp(1.0f, e), (int)(nx() % 5) - 2);
}
inline float any_mag() { return mag(-64, 64); }
inline void vec_cases(long n, std::vector<VecCase>& out) {
    reseed(10);
    for (long k = 0; k < n; k++) {
        VecCase c;
        const int e = nx() % 2 ? -50 : 50;
        const uint64_t kind = nx() % 4;
        if (kind == 0) {            // one component: dot = m * m beside 2^(2e)
            float v[3] = {0.0f, 0.0f, 0.0f};
            const int q = (int)(nx() % 3);
            v[q] = edge_mag(e);
            c.a = mk(v[0], v[1], v[2]);
        } else if (kind == 1) {     // a unit vector scaled by 2^e: dot within a few ulps of 2^(2e), either side
            uint32_t st = (uint32_t)nx();
            c.a = pt::random_unit_vector(st) * std::ldexp(1.0f, e);
        } else if (kind == 2) {     // half an octave either side
            c.a = isc::sym3(mk(0.0f, 0.0f, 0.0f), std::ldexp(1.0f, e));
        } else {                    // any scale
            const float x = any_mag(), y = any_mag(), z = any_mag();
            c.a = mk(x, y, z);
        }
        const int e2 = nx() % 2 ? -60 : 60;
        const float bx = nx() % 2 ? edge_mag(e2) : any_mag(), by = nx() % 2 ? edge_mag(e2) : any_mag(), bz = any_mag();
        c.b = mk(bx, by, bz);
        if (nx() % 2) c.a.y = nx() % 2 ? edge_mag(e2) : any_mag();      // div_g(b.y, a.y): a denominator at the edge
        c.s = nx() % 8 == 0 ? (float)(nx() % 2) : uni();
        out.push_back(c);
    }
}

// ------------------------------------------------------------------ guard: pti::ray_in_guard
// Domain: every binary32 in every component.  Most components lie inside their window, so that both verdicts are
// frequent; the rest sit at and one ulp either side of the windows' ends (2^-40 and 2^60 for the origin, 2^-20 and 2
// for the direction), or are zeros, NaNs, infinities and subnormals.
struct GuardCase {
    f3 o, d;
    int scene_fast;
};
inline float guard_component(bool origin) {
    const uint64_t kind = nx() % 16;
    if (kind >= 3) return origin ? gcoord() : isc::dcoord();
    if (kind == 0) {      // an end of the window, and one ulp either side
        const float sg = sgn();
        const float edge = nx() % 2 ? (origin ? 0x1p-40f : 0x1p-20f) : (origin ? 0x1p60f : 2.0f);
        return sg * ulps(edge, (int)(nx() % 3) - 1);
    }
    if (kind == 1) {      // an end of the other kind of component's window
        const float sg = sgn();
        const float edge = nx() % 2 ? (origin ? 0x1p-20f : 0x1p-40f) : (origin ? 2.0f : 0x1p60f);
        return sg * ulps(edge, (int)(nx() % 3) - 1);
    }
    const float v[] = {0.0f, -0.0f, NAN, -NAN, INFINITY, -INFINITY, 0x1p-149f, -0x1p-126f};
    return v[nx() % 8];
}
inline void guard_cases(long n, std::vector<GuardCase>& out) {
    reseed(11);
    for (long k = 0; k < n; k++) {
        GuardCase c;
        const float oz = guard_component(true), oy = guard_component(true), ox = guard_component(true);
        const float dz = guard_component(false), dy = guard_component(false), dx = guard_component(false);
        c.o = mk(ox, oy, oz);
        c.d = mk(dx, dy, dz);
        c.scene_fast = nx() % 8 != 0;
        out.push_back(c);
    }
}

// ------------------------------------------------------------------ sphere: pti::sphere_t
// Domain: any ray, a sphere with a finite centre and radius r >= 0, stored as the packer stores it ({centre, r * r}).
// Rays that miss, that graze (a discriminant of exactly 0 on small integers, and one ulp of the centre either side
// of it; tangent rays at any angle, whose discriminant is a few ulps from 0), that start inside the sphere or on it,
// that point away, and rays with zero, NaN or infinite components.
struct SphereCase {
    float c[3], r;
    f3 o, d;
};
inline void sphere_cases(long n, std::vector<SphereCase>& out) {
    reseed(12);
    for (long k = 0; k < n; k++) {
        SphereCase c;
        const float s = std::ldexp(1.0f, (int)(nx() % 33) - 16);
        const uint64_t kind = nx() % 8;
        if (kind == 0) {            // small integers along one axis: a = 1, disc = j^2 - (j^2 + m^2 - r^2) exactly
            const int axis = (int)(nx() % 3), side = (axis + 1 + (int)(nx() % 2)) % 3;
            const float j = (float)(1 + nx() % 64), m = (float)(nx() % 16);
            float cv[3] = {0.0f, 0.0f, 0.0f}, ov[3] = {0.0f, 0.0f, 0.0f}, dv[3] = {0.0f, 0.0f, 0.0f};
            cv[side] = ulps(m * s, (int)(nx() % 3) - 1);      // the centre m away from the ray's line, r = m: a graze
            ov[axis] = -j * s;
            dv[axis] = 1.0f;
            for (int q = 0; q < 3; q++) c.c[q] = cv[q];
            c.r = m * s;
            c.o = mk(ov[0], ov[1], ov[2]);
            c.d = mk(dv[0], dv[1], dv[2]);
        } else {
            const f3 ctr = isc::sym3(mk(0.0f, 0.0f, 0.0f), 4.0f * s);
            c.c[0] = ctr.x, c.c[1] = ctr.y, c.c[2] = ctr.z;
            c.r = s * (0.125f + uni());
            uint32_t st = (uint32_t)nx();
            const f3 u = pt::random_unit_vector(st);                 // the ray's direction
            f3 w = pt::cross(u, mk(0.0f, 0.0f, 1.0f));
            if (!(pt::dot(w, w) > 0.0f)) w = mk(1.0f, 0.0f, 0.0f);
            w = pt::normalize(w);                                     // a unit vector across it
            const float back = s * 8.0f * uni();
            if (kind == 1) {        // tangent: the line passes at distance r (and one ulp of r either side)
                const float rr = ulps(c.r, (int)(nx() % 3) - 1);
                c.o = (ctr + w * rr) - u * back;
                c.d = u;
            } else if (kind == 2) { // the origin inside the sphere, or on it
                const float f = nx() % 4 == 0 ? 1.0f : uni();
                c.o = ctr + w * (c.r * f);
                c.d = u;
            } else if (kind == 3) { // aimed at the sphere from behind it: both roots negative
                c.o = (ctr + w * (c.r * uni())) + u * (c.r + back);
                c.d = u;
            } else if (kind == 4) { // a wide miss
                c.o = (ctr + w * (c.r * (1.0f + 4.0f * uni()))) - u * back;
                c.d = u;
            } else {                // a hit, the direction not normalised
                const float len = nx() % 2 ? 1.0f : std::fabs(mag(-8, 8));
                c.o = (ctr + w * (c.r * uni())) - u * (c.r + back);
                c.d = u * len;
            }
            if (nx() % 32 == 0) {   // one component of the ray replaced
                const float v[] = {0.0f, -0.0f, NAN, INFINITY, -INFINITY, 0x1p-149f, 0x1p127f, -0x1p-126f};
                const float x = v[nx() % 8];
                float* comp[6] = {&c.o.x, &c.o.y, &c.o.z, &c.d.x, &c.d.y, &c.d.z};
                *comp[nx() % 6] = x;
            }
            if (nx() % 64 == 0) c.d = mk(0.0f, 0.0f, 0.0f);          // a = 0: 0/0 or x/0
        }
        out.push_back(c);
    }
}

// ------------------------------------------------------------------ leaf_choice: pti::leaf_choice
// Domain: every binary32 in h1, h2 and t.  Each is a distance of any scale, or sits at and one ulp either side of
// 1e-4, of t and of the other hit, or is -1 (a miss), NaN or +inf.
struct LeafChoiceCase {
    float h1, h2, t;
};
inline float choice_value(float near_a, float near_b) {
    switch (nx() % 8) {
        case 0: return ulps(0.0001f, (int)(nx() % 3) - 1);
        case 1: return ulps(near_a, (int)(nx() % 3) - 1);
        case 2: return ulps(near_b, (int)(nx() % 3) - 1);
        case 3: return -1.0f;
        case 4: { const float v[] = {NAN, INFINITY, 0.0f, -0.0f, -INFINITY, 0x1p-149f}; return v[nx() % 6]; }
        default: return std::fabs(mag(-16, 8));
    }
}
inline void leaf_choice_cases(long n, std::vector<LeafChoiceCase>& out) {
    reseed(13);
    for (long k = 0; k < n; k++) {
        LeafChoiceCase c;
        const uint64_t tk = nx() % 8;
        c.t = tk == 0 ? INFINITY : tk == 1 ? ulps(0.0001f, (int)(nx() % 3) - 1) : std::fabs(mag(-12, 8));
        if (nx() % 64 == 0) c.t = NAN;
        c.h1 = choice_value(c.t, 1.0f);
        c.h2 = choice_value(c.t, c.h1);
        if (nx() % 4 == 0) c.h1 = ulps(c.h2, (int)(nx() % 3) - 1);    // the first beside the second
        out.push_back(c);
    }
}

// ------------------------------------------------------------------ pinhole: pti::film_coord, pti::pinhole_dir
// Domain: an image of 1..65536 pixels a side, a pixel of it, a jitter in {0} U [2^-32, 1) as pt::random01 gives it
// (the numerator of film_coord is then 0 or in [2^-32, 2^17)), and a camera basis as pti::camera_basis derives it.
struct PinholeCase {
    int x, y, W, H;
    float ax, ay, rW, rH;      // rW, rH: RN(1/W), RN(1/H) by the host's IEEE division, as every caller derives them
    f3 fwd, right, up;
};
inline void pinhole_cases(long n, std::vector<PinholeCase>& out) {
    reseed(14);
    const int sizes[] = {1, 2, 3, 64, 640, 1000, 1920, 4096, 65535, 65536};
    for (long k = 0; k < n; k++) {
        PinholeCase c;
        c.W = nx() % 4 == 0 ? sizes[nx() % 10] : 1 + (int)(nx() % 65536);
        c.H = nx() % 4 == 0 ? sizes[nx() % 10] : 1 + (int)(nx() % 65536);
        c.x = nx() % 8 == 0 ? c.W - 1 : (int)(nx() % (uint64_t)c.W);
        c.y = nx() % 8 == 0 ? 0 : (int)(nx() % (uint64_t)c.H);
        uint32_t st = (uint32_t)nx();
        c.ax = nx() % 4 == 0 ? 0.0f : pt::random01(st);
        c.ay = nx() % 4 == 0 ? 0.0f : pt::random01(st);
        if (nx() % 16 == 0) c.ax = 0x1p-32f;
        c.rW = 1.0f / (float)c.W, c.rH = 1.0f / (float)c.H;
        const float dz = sym(), dy = sym(), dx = sym();
        float cam[12] = {0.0f, 0.0f, 0.0f, 0.0f, dx, dy, dz, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, b[12];
        pti::camera_basis(cam, c.W, c.H, b);
        c.fwd = mk(b[3], b[4], b[5]), c.right = mk(b[6], b[7], b[8]), c.up = mk(b[9], b[10], b[11]);
        out.push_back(c);
    }
}

// ------------------------------------------------------------------ sky_depth: pti::sky, pti::depth_term
// Domain: any direction (pt::normalize switches forms where dot(d, d) leaves [2^-100, 2^100]; zero and NaN
// directions as a ray outside every guard has them), and a hit point and origin of any finite scale.
struct SkyDepthCase {
    f3 d, hitp, o;
    int no_sky;
};
inline void sky_depth_cases(long n, std::vector<SkyDepthCase>& out) {
    reseed(15);
    for (long k = 0; k < n; k++) {
        SkyDepthCase c;
        const uint64_t kind = nx() % 8;
        if (kind == 0) {            // dot(d, d) beside 2^-100 or 2^100
            const int e = nx() % 2 ? -50 : 50;
            uint32_t st = (uint32_t)nx();
            c.d = pt::random_unit_vector(st) * std::ldexp(1.0f, e);
        } else if (kind == 1) {     // straight up, down, level
            const float z = nx() % 3 == 0 ? 0.0f : sgn();
            const float x = z == 0.0f ? 1.0f : 0.0f;
            c.d = mk(x, 0.0f, z);
        } else if (kind == 2) {
            const float v[] = {0.0f, -0.0f, NAN, INFINITY, -INFINITY, 0x1p-149f};
            const float z = v[nx() % 6], y = nx() % 2 ? 0.0f : sym(), x = nx() % 2 ? 0.0f : sym();
            c.d = mk(x, y, z);
        } else {
            uint32_t st = (uint32_t)nx();
            const float len = nx() % 2 ? 1.0f : std::fabs(mag(-20, 20));
            c.d = pt::random_unit_vector(st) * len;
        }
        const float s = std::ldexp(1.0f, (int)(nx() % 81) - 40);
        c.o = isc::sym3(mk(0.0f, 0.0f, 0.0f), s);
        const float far = nx() % 8 == 0 ? 0.0f : std::ldexp(1.0f, (int)(nx() % 41) - 20);
        c.hitp = isc::sym3(c.o, s * far);                               // far = 0: the hit at the origin, s = 0
        if (nx() % 64 == 0) c.hitp.x = nx() % 2 ? INFINITY : NAN;
        c.no_sky = nx() % 8 == 0;
        out.push_back(c);
    }
}

// ------------------------------------------------------------------ bounce: pti::shade_hit
// Domain: what a hit segment hands to the shade: a unit normal flipped against d, a direction of any length, a hit
// point, gathered light >= 0 and a carried colour in [0, 1], any RNG state, a material of the twin's fixed table
// (twf::TwinMats), all four display modes, bounce at, below and above max_bounce - 1.
constexpr int kTwinMats = 6;
struct BounceCase {
    f3 normal, hitp, o, d, inc, col;
    uint32_t state;
    int bounce, max_bounce, mode, mat;
};
inline void bounce_cases(long n, std::vector<BounceCase>& out) {
    reseed(32);
    for (long k = 0; k < n; k++) {
        BounceCase c;
        uint32_t st = (uint32_t)nx();
        c.normal = pt::random_unit_vector(st);
        const float len = nx() % 4 == 0 ? std::fabs(mag(-6, 6)) : 1.0f;
        c.d = pt::random_unit_vector(st) * len;
        if (nx() % 16 == 0) c.d = c.normal * -len;                      // head on: the reflection is -d
        if (nx() % 16 == 0) c.d = pt::cross(c.normal, c.d);             // grazing: dot(normal, d) about 0
        if (pt::dot(c.normal, c.d) > 0.0f) c.normal = c.normal * -1.0f;
        const float s = std::ldexp(1.0f, (int)(nx() % 25) - 12);
        c.o = isc::sym3(mk(0.0f, 0.0f, 0.0f), s);
        c.hitp = isc::sym3(c.o, s);
        const float iz = 4.0f * uni(), iy = 4.0f * uni(), ix = 4.0f * uni();
        c.inc = nx() % 4 == 0 ? mk(0.0f, 0.0f, 0.0f) : mk(ix, iy, iz);
        const float cz = uni(), cy = uni(), cx = uni();
        c.col = nx() % 4 == 0 ? mk(1.0f, 1.0f, 1.0f) : mk(cx, cy, cz);
        c.state = k < 4 ? (uint32_t)(0u - (uint32_t)k) : (uint32_t)nx();
        c.max_bounce = (int)(nx() % 9);
        c.bounce = nx() % 2 ? c.max_bounce : (int)(nx() % (uint64_t)(c.max_bounce + 1));
        c.mode = 1 + (int)(nx() % 4);
        c.mat = (int)(nx() % (uint64_t)kTwinMats);
        out.push_back(c);
    }
}

}  // namespace twc
