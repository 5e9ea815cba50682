// pt_host_scene.h -- what the host twins (pt_query.cpp, pt_trace.cpp, pt_camera.cpp, pt_film.cpp) share:
// the scene accessor ptq::cast and ptt::shade are templated on, over a packed scene's buffers, and the argument checks
// of the *_host entry points.  Plain C++.  In an unnamed namespace on purpose: the templates instantiated on HostScene
// then have internal linkage in each twin, as they had with a struct of its own, and the library exports nothing new.
#pragma once

#include "pt_scene_pack.h"

#include <climits>

namespace pth {
namespace {

struct HostScene {
    const ptp::Quad* nodes;
    const ptp::Quad* tris;
    const ptp::Quad* spheres;
    const ptp::Quad* leaf;
    const ptp::Quad* mats;
    int nn, ns;
    bool fast;
    int n_nodes() const { return nn; }
    int n_spheres() const { return ns; }
    bool scene_fast() const { return fast; }
    void node(int i, ptp::Quad& lo, ptp::Quad& hi) const { lo = nodes[2 * (size_t)i], hi = nodes[2 * (size_t)i + 1]; }
    ptp::Quad tri(int slot, int k) const { return tris[4 * (size_t)slot + k]; }
    ptp::Quad sphere(int i, int k) const { return spheres[2 * (size_t)i + k]; }
    ptp::Quad leaf_tris(int pair) const { return leaf[pair]; }
    ptp::Quad mat(int i, int k) const { return mats[3 * (size_t)i + k]; }
};

inline HostScene host_scene(const ptp::PackedScene& p) {
    const auto quads = [&p](int b) { return reinterpret_cast<const ptp::Quad*>(p.buf[b].data()); };
    return {quads(ptp::kNodes), quads(ptp::kTris), quads(ptp::kSpheres), quads(ptp::kLeafTris), quads(ptp::kMats),
            p.facts.n_nodes, p.facts.n_spheres, p.facts.scene_fast != 0};
}

// A context's settings as a *_host entry point takes them.
inline bool settings_ok(int ctx_flags, int max_bounce, int display_mode) {
    return !(ctx_flags & ~PT_FLAG_ALL) && max_bounce >= 0 && display_mode >= 1 && display_mode <= 4;
}

// The frame range of a trace: what pte::check_frames (pt_entry.h) refuses with a message.
inline bool frames_ok(int frame_first, int n_frames, int accumulate_first) {
    return frame_first >= 1 && n_frames >= 1 && frame_first <= INT_MAX - n_frames &&
           (accumulate_first == 0 || accumulate_first == 1);
}

}  // namespace
}  // namespace pth
