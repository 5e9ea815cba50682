// pt_trace.cpp -- traced rays on the host (include/pt_api.h: pt_trace_host, pt_pixel_seeds).  Plain host code: the
// scene goes through ptp::pack_scene as an upload's does, and every ray runs ptt::trace_frames (pt_trace.h), the
// per-ray code the device kernel runs, on the packed buffers.  The CPU suite (tests/test_trace_host.py) checks it
// against the oracle's renders bit for bit, and the GPU suite checks pt_trace against this.
// The scene accessor over the packed buffers and the settings checks are pt_host_scene.h's, shared by the four twins.
#include "pt_trace.h"

#include "pt_host_scene.h"

#include <string>

extern "C" {

int pt_pixel_seeds(const int* xy, long long n, unsigned* seeds_out) {
    if (n < 0 || (n > 0 && (!xy || !seeds_out))) return PT_E_ARG;
    for (long long i = 0; i < n; i++) seeds_out[i] = ptt::pixel_seed(xy[2 * i], xy[2 * i + 1]);
    return PT_OK;
}

// Measurements only (tools/trace_measure.py), not part of the public ABI: pt_trace_host, and the number of segments
// it ran added to *segments.
int pt__trace_host_segments(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                            const float* spheres, int n_spheres, int ctx_flags, int max_bounce, int display_mode,
                            const pt_ray* rays, const unsigned* seeds, long long n, int frame_first, int n_frames,
                            int accumulate_first, float* rgba, long long* segments) {
    if (n < 0 || !pth::settings_ok(ctx_flags, max_bounce, display_mode)) return PT_E_ARG;
    if (!pth::frames_ok(frame_first, n_frames, accumulate_first)) return PT_E_ARG;
    if (n > 0 && (!rays || !rgba)) return PT_E_ARG;
    ptp::PackedScene packed;
    std::string err;
    const int rc = ptp::pack_scene(tris, n_tris, bvh, n_nodes, mats, n_mats, spheres, n_spheres, packed, err);
    if (rc) return rc;
    const pth::HostScene sc = pth::host_scene(packed);
    const ptt::Frames fr = {ctx_flags, max_bounce, display_mode, frame_first, n_frames, accumulate_first};
    for (long long i = 0; i < n; i++) {
        const pt_ray& r = rays[i];
        ptp::Quad prior = {0.0f, 0.0f, 0.0f, 0.0f};
        if (accumulate_first) prior = {rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]};
        const ptp::Quad q = ptt::trace_frames<ptp::Quad>(sc, fr, pt::mk(r.o[0], r.o[1], r.o[2]), pt::mk(r.d[0], r.d[1], r.d[2]),
                                                         r.t_max, seeds ? seeds[i] : ptt::default_seed(i), prior, segments);
        rgba[4 * i] = q.x, rgba[4 * i + 1] = q.y, rgba[4 * i + 2] = q.z, rgba[4 * i + 3] = q.w;
    }
    return PT_OK;
}

int pt_trace_host(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                  const float* spheres, int n_spheres, int ctx_flags, int max_bounce, int display_mode,
                  const pt_ray* rays, const unsigned* seeds, long long n, int frame_first, int n_frames,
                  int accumulate_first, float* rgba) {
    return pt__trace_host_segments(tris, n_tris, bvh, n_nodes, mats, n_mats, spheres, n_spheres, ctx_flags, max_bounce,
                                   display_mode, rays, seeds, n, frame_first, n_frames, accumulate_first, rgba, nullptr);
}

}  // extern "C"
