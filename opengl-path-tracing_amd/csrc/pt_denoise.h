// pt_denoise.h -- the variance-guided a-trous filter over first-hit guides (include/pt_api.h:
// pt_denoise, pt_denoise_host), shared by the device kernels
// (pt_denoise_kernels.hip) and the host restatement (pt_denoise.cpp), so the CPU suite checks
// the very per-tap code the GPU runs -- the idiom of pt_noise.h.
//
// Every operation is a separately rounded IEEE binary32 operation (the build's
// -ffp-contract=off and correctly rounded divide), and a pixel's taps are taken in one fixed
// order, so host and device agree bit for bit, and numpy float32 restates them exactly.  The
// weights are rational functions of the guide and colour distances: there is no transcendental
// whose rounding would have to be pinned.
#pragma once

#include "pt_noise.h"

#if defined(__HIPCC__)
#define PTD_HD __host__ __device__ __forceinline__
#else
#define PTD_HD inline
#endif

namespace ptd {

constexpr int kMaxIterations = 8;
constexpr float kVarEps = 1e-6f;      // added to the prefiltered variance under the luminance factor

struct Px { float r, g, b, v; };                      // a pixel's state: colour and variance of the mean luminance
struct Gd { float nx, ny, nz, z, ax, ay, az; };       // its guides: first-hit normal, distance, albedo
struct K { float kl, kn, ka, kz; };                   // 1 / sigma^2 per factor, 0 = the factor is off

// k of one sigma: a NaN or non-positive sigma switches the factor off
PTD_HD float inv_sq(float s) { return (s > 0.0f) ? 1.0f / (s * s) : 0.0f; }

PTD_HD bool finite(float x) { return __builtin_fabsf(x) <= 3.402823466e38f; }
PTD_HD bool usable(const Px& p) { return finite(p.r) && finite(p.g) && finite(p.b) && finite(p.v); }

// variance of the mean luminance from the moments (S1, S2) of n >= 2 frames (pt_noise.h's m and d); a NaN stays
PTD_HD float variance(float s1, float s2, int n) {
    const float nf = (float)n;
    const float m = s1 / nf;
    const float d = s2 / nf - m * m;
    return (d < 0.0f ? 0.0f : d) / (float)(n - 1);
}

// One pixel of one iteration.  `src` answers for the iteration's input:
//   inside(x, y)          the pixel is in the image and in the footprint
//   state(x, y)           the state of an inside pixel (the variance prefilter's unit offsets)
//   tap_state(dx, dy), tap_guide(dx, dy)   state and guides of the inside pixel (x + step*dx, y + step*dy)
// (x, y) itself is inside.  `lum_on`: the filter is guided (the moments hold n >= 2 frames).
template <class S>
PTD_HD Px filter_px(const S& src, int x, int y, int step, bool lum_on, const K& k) {
    const Px cp = src.tap_state(0, 0);
    const Gd gp = src.tap_guide(0, 0);
    const bool lum = lum_on && usable(cp);
    float gl = 0.0f, yp = 0.0f;
    if (lum) {      // the variance under the luminance factor: 3x3-prefiltered over the usable neighbours
        const float g3[3] = {0.25f, 0.5f, 0.25f};
        float pv = 0.0f, pw = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int dy = -1; dy <= 1; dy++)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int dx = -1; dx <= 1; dx++) {
                if (!src.inside(x + dx, y + dy)) continue;
                const Px q = src.state(x + dx, y + dy);
                if (!usable(q)) continue;
                const float w = g3[dy + 1] * g3[dx + 1];
                pv = pv + w * q.v;
                pw = pw + w;
            }
        const float vv = pw > 0.0f ? pv / pw : cp.v;
        gl = k.kl / (vv + kVarEps);
        yp = ptn::luminance(cp.r, cp.g, cp.b);
    }
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, sv = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dy = -2; dy <= 2; dy++)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int dx = -2; dx <= 2; dx++) {
            if (!src.inside(x + step * dx, y + step * dy)) continue;
            const Px q = src.tap_state(dx, dy);
            if (!usable(q)) continue;
            const Gd gq = src.tap_guide(dx, dy);
            const float nx = gp.nx - gq.nx, ny = gp.ny - gq.ny, nz = gp.nz - gq.nz;
            const float dn = (nx * nx + ny * ny) + nz * nz;
            const float ax = gp.ax - gq.ax, ay = gp.ay - gq.ay, az = gp.az - gq.az;
            const float da = (ax * ax + ay * ay) + az * az;
            const float zz = gp.z - gq.z;
            const float dz = zz * zz;
            float t = ((1.0f + dn * k.kn) * (1.0f + da * k.ka)) * (1.0f + dz * k.kz);
            if (lum) {
                const float dl = yp - ptn::luminance(q.r, q.g, q.b);
                t = t * (1.0f + (dl * dl) * gl);
            }
            t = t * t;
            t = t * t;
            const float w = (h[dy + 2] * h[dx + 2]) / t;
            if (!(w > 0.0f)) continue;      // also a NaN or an overflowed weight
            sw = sw + w;
            ar = ar + w * q.r;
            ag = ag + w * q.g;
            ab = ab + w * q.b;
            sv = sv + (w * w) * q.v;
        }
    if (!(sw > 0.0f)) return cp;            // no usable tap: the pixel keeps its input
    Px o;
    o.r = ar / sw;
    o.g = ag / sw;
    o.b = ab / sw;
    o.v = sv / (sw * sw);
    return o;
}

}  // namespace ptd
