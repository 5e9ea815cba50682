// pt_film.cpp -- the film on the host (include/pt_api.h: pt_film_expose_host).  Plain host code: the scene goes through
// ptp::pack_scene as an upload's does, and every pixel runs ptfilm::expose_pixel (pt_film.h) -- ptcam::make_ray,
// ptq::cast, ptfilm::guide_sample, ptt::shade and ptt::segment, the per-pixel code the device kernel runs, on the
// packed buffers.  The CPU suite (tests/test_film_host.py) checks it against compositions of pt_trace_camera_host,
// and the GPU suite checks pt_film_expose against this.
// The scene accessor over the packed buffers and the settings checks are pt_host_scene.h's, shared by the four twins.
#include "pt_film.h"

#include "pt_host_scene.h"

#include <string>

extern "C" {

int pt_film_expose_host(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                        const float* spheres, int n_spheres, int ctx_flags, int max_bounce, int display_mode,
                        const pt_camera* camera, int guide_frames, int frame_first, int n_frames, int accumulate_first,
                        int frames_before, int guides_held, float* rgba, float* moments, float* guides,
                        int* guides_held_out) {
    if (!pth::settings_ok(ctx_flags, max_bounce, display_mode)) return PT_E_ARG;
    if (ptcam::validate(camera) != PT_OK) return PT_E_ARG;
    if (!pth::frames_ok(frame_first, n_frames, accumulate_first)) return PT_E_ARG;
    if (guide_frames < 1 || frames_before < 0 || guides_held < 0 || guides_held > guide_frames) return PT_E_ARG;
    if (!rgba || !moments || !guides) return PT_E_ARG;
    ptp::PackedScene packed;
    std::string err;
    const int rc = ptp::pack_scene(tris, n_tris, bvh, n_nodes, mats, n_mats, spheres, n_spheres, packed, err);
    if (rc) return rc;
    const pth::HostScene sc = pth::host_scene(packed);
    const ptt::Frames fr = {ctx_flags, max_bounce, display_mode, frame_first, n_frames, accumulate_first};
    const ptcam::Prepared cam = ptcam::prepare(*camera);
    const ptfilm::GuideRange gr = ptfilm::guide_range(frame_first, n_frames, guides_held, guide_frames);
    for (int y = 0; y < cam.H; y++)
        for (int x = 0; x < cam.W; x++) {
            const size_t i = (size_t)y * cam.W + x;
            float* q = rgba + 4 * i;
            float* m = moments + 2 * i;
            float* g = guides + 8 * i;
            // an exposure that restarts reads neither the image nor the moments
            ptp::Quad px = {0.0f, 0.0f, 0.0f, 0.0f};
            float s1 = 0.0f, s2 = 0.0f;
            if (accumulate_first) px = {q[0], q[1], q[2], q[3]}, s1 = m[0], s2 = m[1];
            ptp::Quad g0 = {g[0], g[1], g[2], g[3]}, g1 = {g[4], g[5], g[6], g[7]};
            ptfilm::expose_pixel<ptp::Quad>(sc, fr, cam, x, y, gr, px, s1, s2, g0, g1);
            q[0] = px.x, q[1] = px.y, q[2] = px.z, q[3] = px.w;
            m[0] = s1, m[1] = s2;
            if (gr.lo <= gr.hi) {
                g[0] = g0.x, g[1] = g0.y, g[2] = g0.z, g[3] = g0.w;
                g[4] = g1.x, g[5] = g1.y, g[6] = g1.z, g[7] = g1.w;
            }
        }
    if (guides_held_out) *guides_held_out = ptfilm::held_after(gr, guides_held);
    return PT_OK;
}

}  // extern "C"
