// pt_camera.cpp -- the camera models on the host (include/pt_api.h: pt_trace_camera_host, pt_camera_rays_host).  Plain
// host code: the scene goes through ptp::pack_scene as an upload's does, and every pixel runs ptcam::trace_frames
// (pt_camera.h) -- ptcam::make_ray, then ptt::segment -- the per-pixel code the device kernel runs, on the packed
// buffers.  The CPU suite (tests/test_camera_host.py) checks it against the oracle's default renders bit for bit, and
// the GPU suite checks pt_trace_camera against this.
// The scene accessor over the packed buffers and the settings checks are pt_host_scene.h's, shared by the four twins.
#include "pt_camera.h"

#include "pt_host_scene.h"

#include <string>

extern "C" {

int pt_camera_rays_host(const pt_camera* camera, const int* xy, long long n, int frame, pt_ray* rays_out,
                        unsigned* states_out) {
    if (ptcam::validate(camera) != PT_OK || n < 0 || frame < 1) return PT_E_ARG;
    if (n > 0 && (!xy || !rays_out)) return PT_E_ARG;
    // a pixel outside the image has no ray here: a panorama's angles would leave cosf_pinned's domain.  A pass of
    // its own over xy, before any ray is made, so that a refused call has written nothing.
    for (long long i = 0; i < n; i++)
        if (xy[2 * i] < 0 || xy[2 * i] >= camera->width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= camera->height) return PT_E_ARG;
    const ptcam::Prepared cam = ptcam::prepare(*camera);
    for (long long i = 0; i < n; i++) {
        const int x = xy[2 * i], y = xy[2 * i + 1];
        uint32_t state = pt::seed(x, y, frame);
        pt::f3 o, d;
        ptcam::make_ray(cam, x, y, state, o, d);
        pt_ray& r = rays_out[i];
        r.o[0] = o.x, r.o[1] = o.y, r.o[2] = o.z, r.t_max = __builtin_huge_valf();
        r.d[0] = d.x, r.d[1] = d.y, r.d[2] = d.z, r.pad = 0.0f;
        if (states_out) states_out[i] = state;
    }
    return PT_OK;
}

int pt_trace_camera_host(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                         const float* spheres, int n_spheres, int ctx_flags, int max_bounce, int display_mode,
                         const pt_camera* camera, int frame_first, int n_frames, int accumulate_first, float* rgba) {
    if (!pth::settings_ok(ctx_flags, max_bounce, display_mode)) return PT_E_ARG;
    if (ptcam::validate(camera) != PT_OK) return PT_E_ARG;
    if (!pth::frames_ok(frame_first, n_frames, accumulate_first)) return PT_E_ARG;
    if (!rgba) return PT_E_ARG;
    ptp::PackedScene packed;
    std::string err;
    const int rc = ptp::pack_scene(tris, n_tris, bvh, n_nodes, mats, n_mats, spheres, n_spheres, packed, err);
    if (rc) return rc;
    const pth::HostScene sc = pth::host_scene(packed);
    const ptt::Frames fr = {ctx_flags, max_bounce, display_mode, frame_first, n_frames, accumulate_first};
    const ptcam::Prepared cam = ptcam::prepare(*camera);
    for (int y = 0; y < cam.H; y++)
        for (int x = 0; x < cam.W; x++) {
            const size_t i = (size_t)y * cam.W + x;
            ptp::Quad prior = {0.0f, 0.0f, 0.0f, 0.0f};
            if (accumulate_first) prior = {rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]};
            const ptp::Quad q = ptcam::trace_frames<ptp::Quad>(sc, fr, cam, x, y, prior);
            rgba[4 * i] = q.x, rgba[4 * i + 1] = q.y, rgba[4 * i + 2] = q.z, rgba[4 * i + 3] = q.w;
        }
    return PT_OK;
}

}  // extern "C"
