// pt_camera.h -- camera models (include/pt_api.h: pt_camera, pt_trace_camera, pt_camera_rays_host): the
// ray of pixel (x, y) in frame f as a function of the pixel, the frame's random state and a launch-uniform camera,
// shared by the device kernels (pt_camera_kernels.hip) and the host twin (pt_camera.cpp) -- the idiom of pt_query.h
// and pt_trace.h, on which it is built.
//
// make_ray runs on state = pt::seed(x, y, frame), takes the camera's draws from it in a fixed order and leaves it for
// Trace, as the reference's main does for its jitter (computeShader.c:530-542):
//   1. unless PT_CAM_NO_AA: ax = random01, ay = random01 (else both 0, nothing drawn);
//   2. u = pti::film_coord(x + ax, W, RN(1/W)), v likewise with H;
//   3. the model's own draws: the thin lens takes u1, then u2; the others none.
// Every operation is a pt_math.h one (no libm by name: host and device libm differ); sin t = cosf_pinned(|t - pi/2|)
// with pi/2 = 0.5f * 3.1415926f, whose argument stays below 3 pi/2 for t in [0, 2 pi], inside cosf_pinned's domain.
// Nothing is special-cased: a fwd parallel to z makes NaN rays, as it does in the reference.
#pragma once

#include "pt_trace.h"

namespace ptcam {

using pt::f3;
using pt::mk;

constexpr float kPi = 3.1415926f;          // random_normal's constant (pt_math.h)
constexpr float kTwoPi = 2.0f * 3.1415926f;
constexpr float kHalfPi = 0.5f * 3.1415926f;

// What prepare() derives once per call: launch-uniform, a flat struct the kernels take by value (k_camera_rays keeps
// it in SGPRs; k_trace_camera reads it back from its argument segment where it makes a ray, pt_camera_kernels.hip).
struct Prepared {
    int model, W, H, flags;
    float fW, fH, rW, rH;      // (float)W, (float)H, RN(1/W), RN(1/H) by the host's IEEE division
    f3 pos, fwd, right;
    f3 upS;                    // pti::camera_basis's up: upU * H / W
    f3 upU;                    // normalize(cross(right, fwd))
    f3 F;                      // normalize(fwd.x, fwd.y, 0): the panorama's centre column
    float aperture, focus, ortho_width;
};

// PT_OK or PT_E_ARG: null, unknown model or flag, size out of range, and for the model that reads them a NaN,
// negative or (focus, ortho_width) zero parameter.  Fields a model does not read are ignored.
inline int validate(const pt_camera* c) {
    if (!c) return PT_E_ARG;
    if (c->model < PT_CAM_PINHOLE || c->model > PT_CAM_EQUIRECT || (c->flags & ~PT_CAM_NO_AA)) return PT_E_ARG;
    if (c->width < 1 || c->width > 65536 || c->height < 1 || c->height > 65536) return PT_E_ARG;
    if (c->model == PT_CAM_THIN_LENS && (!(c->aperture >= 0.0f) || !(c->focus > 0.0f))) return PT_E_ARG;
    if (c->model == PT_CAM_ORTHO && !(c->ortho_width > 0.0f)) return PT_E_ARG;
    return PT_OK;
}

inline Prepared prepare(const pt_camera& c) {
    float b[12];
    pti::camera_basis(c.cam, c.width, c.height, b);
    Prepared p;
    p.model = c.model, p.W = c.width, p.H = c.height, p.flags = c.flags;
    p.fW = (float)c.width, p.fH = (float)c.height, p.rW = 1.0f / p.fW, p.rH = 1.0f / p.fH;
    p.pos = mk(b[0], b[1], b[2]), p.fwd = mk(b[3], b[4], b[5]), p.right = mk(b[6], b[7], b[8]), p.upS = mk(b[9], b[10], b[11]);
    p.upU = pt::normalize(pt::cross(p.right, p.fwd));
    p.F = pt::normalize(mk(p.fwd.x, p.fwd.y, 0.0f));
    p.aperture = c.aperture, p.focus = c.focus, p.ortho_width = c.ortho_width;
    return p;
}

// sin t for t in [0, 2 pi]
PT_HD float sin_pinned(float t) { return pt::cosf_pinned(__builtin_fabsf(t - kHalfPi)); }

// The ray of pixel (x, y): o, d (normalised), t_max = +inf.  state: pt::seed(x, y, frame) in, Trace's state out.
// M: the model as a compile-time constant, or -1 for the camera's own (a launch-uniform switch).
template <int M = -1>
PT_HD void make_ray(const Prepared& c, int x, int y, uint32_t& state, f3& o, f3& d) {
    const int model = M < 0 ? c.model : M;
    float ax = 0.0f, ay = 0.0f;
    if (!(c.flags & PT_CAM_NO_AA)) {
        ax = pt::random01(state);
        ay = pt::random01(state);
    }
    const float u = pti::film_coord((float)x + ax, c.fW, c.rW);
    const float v = pti::film_coord((float)y + ay, c.fH, c.rH);
    if (model == PT_CAM_ORTHO) {
        o = (c.pos + c.right * (u * c.ortho_width)) + c.upS * (v * c.ortho_width);
        d = c.fwd;
    } else if (model == PT_CAM_EQUIRECT) {
        const float theta = kTwoPi * (u + 0.5f), alpha = kPi * (v + 0.5f);
        const float ct = pt::cosf_pinned(theta), st = sin_pinned(theta);
        const float ca = pt::cosf_pinned(alpha), sa = sin_pinned(alpha);
        const f3 h = c.F * (-ct) + c.right * (-st);
        o = c.pos;
        d = pt::normalize(h * sa + mk(0.0f, 0.0f, -ca));
    } else {
        const f3 D = pti::pinhole_dir(c.fwd, c.right, c.upS, u, v);
        if (model == PT_CAM_THIN_LENS) {
            const float u1 = pt::random01(state);
            const float u2 = pt::random01(state);
            const f3 P = c.pos + D * c.focus;             // D's fwd component is 1: the plane in focus
            const float r = c.aperture * pt::sqrt_g(u1), phi = kTwoPi * u2;
            o = (c.pos + c.right * (r * pt::cosf_pinned(phi))) + c.upU * (r * sin_pinned(phi));
            d = pt::normalize(P - o);
        } else {
            o = c.pos;
            d = pt::normalize(D);
        }
    }
}

// All frames of one pixel, folded into `rgba` in frame order: ptt::trace_frames with the ray made anew every frame.
// TWIN: ptt::trace_frames (pt_trace.h).
template <class Q, class S>
PT_HD Q trace_frames(const S& sc, const ptt::Frames& fr, const Prepared& c, int x, int y, Q rgba) {
    for (int k = 0; k < fr.n_frames; k++) {
        const int frame = fr.frame_first + k;
        uint32_t state = pt::seed(x, y, frame);
        f3 o, d, inc, col, rgb;
        make_ray(c, x, y, state, o, d);
        int bounce;
        ptt::start_path(inc, col, bounce);
        while (!ptt::segment<Q>(sc, fr, __builtin_huge_valf(), o, d, inc, col, state, bounce, rgb)) {}
        rgba = pti::accumulate(rgba, rgb, frame, k > 0 || fr.acc_first == 1);
    }
    return rgba;
}

}  // namespace ptcam
