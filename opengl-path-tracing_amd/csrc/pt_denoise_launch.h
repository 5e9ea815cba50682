// pt_denoise_launch.h -- what pt_render.hip calls of pt_denoise_kernels.hip.  The filter's kernels are a translation
// unit of their own, so the render kernels' code object does not change with them (DESIGN.md §10.5 on code placement).
#pragma once

#include "pt_denoise.h"

#include <hip/hip_runtime.h>

namespace ptd {

// How an iteration reads its taps: kAuto = the LDS tile up to kLdsMaxStep, direct loads beyond
// (tools/denoise_measure.py compares them through pt__denoise_debug).
enum Variant { kAuto = 0, kDirect = 1 };
constexpr int kLdsMaxStep = 16;

struct Image {
    int W, H;               // the image (one context holds all rows)
    int x_limit, y_limit;   // the dispatch footprint
};

// N.rgb, A.rgb and Z.x of three rendered planes into the two guide planes (N.rgb, Z), (A.rgb, 0)
void launch_pack(hipStream_t s, const float4* n, const float4* a, const float4* z, float4* g0, float4* g1, long long px);

// The state plane (rgb, v) of the image: v from the moments with a uniform count n, or with per-tile counts
// tile_frames[tile] + extra (tiles of (8 << tile_shift) x (8 >> tile_shift) pixels, tiles_x per row); moments null: v = 0
void launch_prep(hipStream_t s, const Image& im, const float4* accum, const float2* moments, int n,
                 const unsigned* tile_frames, int extra, int tile_shift, int tiles_x, float4* state);

// One iteration at `step`: in -> out.  alpha_from != null: the last iteration, out = (rgb, alpha_from.w)
void launch_iter(hipStream_t s, const Image& im, const float4* in, float4* out, const float4* g0, const float4* g1,
                 const float4* alpha_from, int step, bool lum_on, const K& k, int variant);

}  // namespace ptd
