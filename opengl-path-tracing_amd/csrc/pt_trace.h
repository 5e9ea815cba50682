// pt_trace.h -- traced rays (include/pt_api.h: pt_trace, pt_trace_device, pt_trace_host): the radiance
// along one caller-supplied ray, shared by the device kernel (pt_trace_kernels.hip) and the host twin (pt_trace.cpp),
// so the CPU suite checks the very per-ray code the GPU runs -- the idiom of pt_query.h, on which it is built.
//
// A frame of a ray is the reference's Trace (computeShader.c:434-501): incoming light 0, ray colour 1, and for every
// segment up to max_bounce one ptq::cast closest hit, then ptt::shade -- the surface bounce, the sky or a display-mode
// return.  The first segment's search starts at the ray's t_max, later ones at +inf.  Nothing is special-cased.
//
// Templated like ptq::cast on the quad type Q and a scene accessor S, which here has one more member:
//   Q    mat(int i, int k)                                  kMats, quad k of material i (3 quads per material)
#pragma once

#include "pt_query.h"

namespace ptt {

using pt::f3;
using pt::mk;

// Frame f of a ray starts from seed + f * 719393 (mod 2^32): with the pixel part y * 831266 + x * 923766 as the seed
// this is pt::seed(x, y, f) (:514-515).
PT_HD uint32_t frame_state(uint32_t seed, int frame) { return seed + (uint32_t)frame * 719393u; }
// The seed of ray i when the caller gives none: pixel (i, 0)'s.
PT_HD uint32_t default_seed(long long i) { return (uint32_t)i * 923766u; }
PT_HD uint32_t pixel_seed(int x, int y) { return (uint32_t)y * 831266u + (uint32_t)x * 923766u; }

// A finished segment (Trace :434-501) from the hit record ptq::cast returned for it: Hit::n is the flipped normal,
// Hit::p is o + d*t, Hit::mat the material.  Returns whether the path ended, with its colour in rgb; otherwise o, d,
// inc, col, state and bounce are the next segment's.  The pieces are pti::shade_hit and pti::sky (pt_isect.h).
template <class Q, class S>
PT_HD bool shade(const S& sc, const ptq::Hit& hit, f3& o, f3& d, f3& inc, f3& col, uint32_t& state, int& bounce,
                 int max_bounce, int mode, int flags, f3& rgb) {
    rgb = inc;
    if (hit.kind != PT_HIT_NONE && pt::length_gt_001(col))
        return pti::shade_hit<Q>(sc, hit.mat, hit.n, hit.p, mode, max_bounce, o, d, inc, col, state, bounce, rgb);
    rgb = inc + pti::sky(d, (flags & PT_FLAG_NO_SKY) != 0) * col;
    return true;
}

// What a launch holds for every ray: the context's settings and the frames asked for.
struct Frames {
    int flags, max_bounce, mode;
    int frame_first, n_frames, acc_first;
};

// The start of a path: the ray as given, nothing gathered yet.
PT_HD void start_path(f3& inc, f3& col, int& bounce) {
    inc = mk(0, 0, 0);
    col = mk(1, 1, 1);
    bounce = 0;
}

// One segment of a path: the closest hit from t_start, then the shade.  Returns whether the path ended (rgb).
template <class Q, class S>
PT_HD bool segment(const S& sc, const Frames& fr, float t_start, f3& o, f3& d, f3& inc, f3& col, uint32_t& state,
                   int& bounce, f3& rgb) {
    const ptq::Hit h = ptq::cast<Q>(sc, o, d, t_start, fr.flags, false);
    return shade<Q>(sc, h, o, d, inc, col, state, bounce, fr.max_bounce, fr.mode, fr.flags, rgb);
}

// All frames of one ray, folded into `rgba` in frame order (pti::accumulate; `rgba` is read only when the first frame
// accumulates).  n_segments, where given, gains the number of segments run (the measurement's unit of work).
template <class Q, class S>
PT_HD Q trace_frames(const S& sc, const Frames& fr, f3 o0, f3 d0, float t_max, uint32_t seed, Q rgba,
                     long long* n_segments = nullptr) {
    for (int k = 0; k < fr.n_frames; k++) {
        const int frame = fr.frame_first + k;
        uint32_t state = frame_state(seed, frame);
        f3 o = o0, d = d0, inc, col, rgb;
        int bounce;
        start_path(inc, col, bounce);
        float t_start = t_max;
        int segments = 1;
        while (!segment<Q>(sc, fr, t_start, o, d, inc, col, state, bounce, rgb)) t_start = __builtin_huge_valf(), segments++;
        if (n_segments) *n_segments += segments;
        rgba = pti::accumulate(rgba, rgb, frame, k > 0 || fr.acc_first == 1);
    }
    return rgba;
}

}  // namespace ptt
