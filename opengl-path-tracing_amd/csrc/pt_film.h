// pt_film.h -- the film (include/pt_api.h: pt_film_*, pt_film_expose_host): the running image, the
// luminance moments and the first-hit guides of one pt_camera, written in one pass over the paths.  The per-pixel code
// shared by the device kernel (pt_film_kernels.hip) and the host twin (pt_film.cpp) -- the idiom of pt_camera.h, on
// which it is built.
//
// A frame of a pixel is ptcam::make_ray, then Trace; the film splits Trace's first segment into ptq::cast and
// ptt::shade (what ptt::segment is), so that the hit is at hand for the guides:
//   image    pti::accumulate of the path's colour, as ptcam::trace_frames;
//   moments  Y = ptn::luminance of that colour, ptn::add_sample(S1, S2, Y), in frame order;
//   guides   in the frames f of [g_lo, g_hi] the seven values of guide_sample, each folded by fold() at frame f.
#pragma once

#include "pt_camera.h"
#include "pt_noise.h"

namespace ptfilm {

using pt::f3;
using pt::mk;

// What a first segment shows of the surface: the returns of ptt::shade in display modes 2, 3 and 4 for a path that
// has gathered nothing (inc = 0, col = 1) -- normal, albedo and the distance term -- and on a miss the sky for all
// three.  n, a and z are the rgb, rgb and .x of those three returns.
struct Guide {
    f3 n, a;
    float z;
};

// (inc = 0, col = 1: the gate holds; the sky's inc + env * col is written out for ptt::shade's -0 and NaN.)  o, d: as cast.
template <class Q, class S>
PT_HD Guide guide_sample(const S& sc, const ptq::Hit& hit, f3 o, f3 d, int flags) {
    Guide g;
    if (hit.kind != PT_HIT_NONE) {
        g.n = (hit.n + mk(1, 1, 1)) * 0.5f;
        g.z = pti::depth_term(hit.p, o);
        const Q m0 = sc.mat(hit.mat, 0);
        g.a = mk(m0.x, m0.y, m0.z);
    } else {
        const f3 rgb = mk(0, 0, 0) + pti::sky(d, (flags & PT_FLAG_NO_SKY) != 0) * mk(1, 1, 1);
        g.n = rgb, g.a = rgb, g.z = rgb.x;
    }
    return g;
}

// One component of the running mean at frame `frame` (pti::accumulate_1), from nothing at frame 1.
PT_HD float fold(float prev, float s, int frame) {
    return frame > 1 ? pti::accumulate_1(prev, s, (float)frame) : s;
}

// The two guide quads (N.rgb, Z), (A.rgb, 0) with the sample of frame `frame` folded in.
template <class Q>
PT_HD void fold_guides(Q& g0, Q& g1, const Guide& g, int frame) {
    g0 = pti::mkq<Q>(fold(g0.x, g.n.x, frame), fold(g0.y, g.n.y, frame), fold(g0.z, g.n.z, frame), fold(g0.w, g.z, frame));
    g1 = pti::mkq<Q>(fold(g1.x, g.a.x, frame), fold(g1.y, g.a.y, frame), fold(g1.z, g.a.z, frame), 0.0f);
}

// The guide frames of an exposure of frames [first, first + n) on a film that holds frames 1..held of guide_frames:
// the frames held + 1 .. min(guide_frames, last) when the range contains held + 1, else none (lo > hi).
struct GuideRange {
    int lo, hi;
};
inline GuideRange guide_range(int first, int n, int held, int guide_frames) {
    const int last = first + (n - 1);
    if (held >= guide_frames || first > held + 1 || last < held + 1) return {1, 0};
    return {held + 1, last < guide_frames ? last : guide_frames};
}
inline int held_after(const GuideRange& r, int held) { return r.lo <= r.hi ? r.hi : held; }

// All frames of one pixel.  rgba, s1 and s2 are read only where the first frame accumulates; g0, g1 in the guide
// frames after frame 1.
// TWIN: ptcam::trace_frames (pt_camera.h), with the first segment opened.
template <class Q, class S>
PT_HD void expose_pixel(const S& sc, const ptt::Frames& fr, const ptcam::Prepared& c, int x, int y, const GuideRange& gr,
                        Q& rgba, float& s1, float& s2, Q& g0, Q& g1) {
    for (int k = 0; k < fr.n_frames; k++) {
        const int frame = fr.frame_first + k;
        uint32_t state = pt::seed(x, y, frame);
        f3 o, d, inc, col, rgb;
        ptcam::make_ray(c, x, y, state, o, d);
        int bounce;
        ptt::start_path(inc, col, bounce);
        const ptq::Hit h = ptq::cast<Q>(sc, o, d, __builtin_huge_valf(), fr.flags, false);
        if (frame >= gr.lo && frame <= gr.hi) fold_guides(g0, g1, guide_sample<Q>(sc, h, o, d, fr.flags), frame);
        bool ended = ptt::shade<Q>(sc, h, o, d, inc, col, state, bounce, fr.max_bounce, fr.mode, fr.flags, rgb);
        while (!ended) ended = ptt::segment<Q>(sc, fr, __builtin_huge_valf(), o, d, inc, col, state, bounce, rgb);
        const bool acc = k > 0 || fr.acc_first == 1;
        rgba = pti::accumulate(rgba, rgb, frame, acc);
        if (!acc) s1 = 0.0f, s2 = 0.0f;
        ptn::add_sample(s1, s2, ptn::luminance(rgb.x, rgb.y, rgb.z));
    }
}

}  // namespace ptfilm
