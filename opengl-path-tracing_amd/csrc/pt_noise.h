// pt_noise.h -- the per-pixel noise estimate (include/pt_api.h: pt_noise, pt_noise_host;
// DESIGN.md §10), shared by the device kernels (pt_render.hip: k_accum_frames' moments,
// k_noise) and the host restatement (pt_noise.cpp: pt_noise_host), so the CPU suite checks the
// very functions the GPU runs -- the idiom of pt_group_plan.h.
//
// Every operation is a separately rounded IEEE binary32 operation (the build's
// -ffp-contract=off and correctly rounded divide / square root), so host and device agree bit
// for bit, and numpy float32 restates them exactly.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PTN_HD __host__ __device__ __forceinline__
#else
#define PTN_HD inline
#endif

namespace ptn {

constexpr float kRelMax = 64.0f;      // relative errors above this (and NaN) count as this
constexpr float kQScale = 65536.0f;   // q = rel in 1/65536 steps; q <= 2^22

// luminance of one frame's colour (Rec. 709 weights)
PTN_HD float luminance(float r, float g, float b) { return (r * 0.2126f + g * 0.7152f) + b * 0.0722f; }

// one frame's luminance folded into the pixel's moments (S1, S2), in frame order
PTN_HD void add_sample(float& s1, float& s2, float y) {
    s1 = s1 + y;
    s2 = s2 + y * y;
}

// (S1, S2) of n >= 2 frames -> the standard error of the mean luminance relative to the mean
// (+ 0.01 so black pixels do not dominate), in 1/65536 steps.  A relative error that is not
// in [0, 64] -- NaN or infinite moments, or a mean at or below -0.01, which no render
// produces -- counts as 64.
PTN_HD unsigned quantise(float s1, float s2, int n) {
    const float nf = (float)n;
    const float m = s1 / nf;
    const float d = s2 / nf - m * m;
    const float v = d < 0.0f ? 0.0f : d;      // rounding can take the variance below zero; NaN stays
#if defined(__HIP_DEVICE_COMPILE__)
    const float sem = __builtin_sqrtf(v / (float)(n - 1));   // correctly rounded (as pt_math.h's fsqrt)
#else
    const float sem = sqrtf(v / (float)(n - 1));
#endif
    float rel = sem / (m + 0.01f);
    if (!(rel >= 0.0f && rel <= kRelMax)) rel = kRelMax;
    return (unsigned)(rel * kQScale);
}

// a target relative error as the q it is compared with (pixels with q above it are counted)
PTN_HD unsigned target_q(float target) {
    float t = target;
    if (!(t >= 0.0f)) t = 0.0f;
    if (t > kRelMax) t = kRelMax;
    return (unsigned)(t * kQScale);
}

// The stop rule of adaptive sampling (pt_render_adaptive), per work-queue tile: the tile retires
// once the sum of its footprint pixels' q is at most target_q times their number -- the
// image-wide integer rule of pt_render_until on one tile.  sum_q <= 64 pixels * 2^22 and
// target_q <= 2^22: the product cannot overflow 64 bits for any pixel count an image has.
PTN_HD bool tile_retires(unsigned long long sum_q, unsigned long long pixels, unsigned tq) {
    return sum_q <= (unsigned long long)tq * pixels;
}

}  // namespace ptn
