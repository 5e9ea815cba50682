// pt_denoise.cpp -- the denoising filter on the host (include/pt_api.h: pt_denoise_host,
// pt_denoise_defaults).  Plain host code over pt_denoise.h, the per-tap code the device kernels
// run: the CPU suite (tests/test_denoise_host.py) checks it against a numpy restatement bit for
// bit, and the GPU suite checks pt_denoise against this.
#include "pt_denoise.h"

#include "../../include/pt_api.h"

#include <vector>

namespace {

struct HostSrc {
    const ptd::Px* st;
    const float* guides;                // 8 floats per pixel: N.rgb, Z, A.rgb, 0
    const unsigned char* fp;
    int W, H, x, y, step;
    bool inside(int qx, int qy) const {
        return qx >= 0 && qx < W && qy >= 0 && qy < H && (!fp || fp[(size_t)qy * W + qx]);
    }
    ptd::Px state(int qx, int qy) const { return st[(size_t)qy * W + qx]; }
    ptd::Px tap_state(int dx, int dy) const { return state(x + step * dx, y + step * dy); }
    ptd::Gd tap_guide(int dx, int dy) const {
        const float* g = guides + 8 * ((size_t)(y + step * dy) * W + (x + step * dx));
        return {g[0], g[1], g[2], g[3], g[4], g[5], g[6]};
    }
};

}  // namespace

extern "C" {

void pt_denoise_defaults(pt_denoise_params* p) {
    if (!p) return;
    p->iterations = 5;
    p->guide_frames = 4;
    p->sigma_lum = 8.0f;
    p->sigma_normal = 0.1f;
    p->sigma_albedo = 0.1f;
    p->sigma_depth = 0.05f;
}

int pt_denoise_host(const float* image, const float* variance, const float* guides, const unsigned char* in_footprint,
                    int W, int H, const pt_denoise_params* params, float* out) {
    if (!image || !guides || !out || W <= 0 || H <= 0) return PT_E_ARG;
    pt_denoise_params dp;
    pt_denoise_defaults(&dp);
    if (params) dp = *params;
    if (dp.iterations < 1 || dp.iterations > ptd::kMaxIterations || dp.guide_frames < 1) return PT_E_ARG;
    const ptd::K k = {ptd::inv_sq(dp.sigma_lum), ptd::inv_sq(dp.sigma_normal), ptd::inv_sq(dp.sigma_albedo),
                      ptd::inv_sq(dp.sigma_depth)};
    const size_t n = (size_t)W * (size_t)H;
    std::vector<ptd::Px> a(n), b(n);
    for (size_t i = 0; i < n; i++) a[i] = {image[4 * i], image[4 * i + 1], image[4 * i + 2], variance ? variance[i] : 0.0f};
    for (int it = 0; it < dp.iterations; it++) {
        HostSrc s = {a.data(), guides, in_footprint, W, H, 0, 0, 1 << it};
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                s.x = x, s.y = y;
                b[i] = s.inside(x, y) ? ptd::filter_px(s, x, y, s.step, variance != nullptr, k) : a[i];
            }
        a.swap(b);
    }
    for (size_t i = 0; i < n; i++) {
        out[4 * i] = a[i].r, out[4 * i + 1] = a[i].g, out[4 * i + 2] = a[i].b;
        out[4 * i + 3] = image[4 * i + 3];
    }
    return PT_OK;
}

}  // extern "C"
