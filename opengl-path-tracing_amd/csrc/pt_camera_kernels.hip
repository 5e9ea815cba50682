// pt_camera_kernels.hip -- the device half of the camera models (include/pt_api.h: pt_trace_camera,
// pt_trace_camera_device, pt_camera_rays_device) and its entry points.  A lane holds one pixel: it
// makes the pixel's ray for the frame with ptcam::make_ray (pt_camera.h) and runs ptt::segment (pt_trace.h) on it, the
// per-pixel code the host twin (pt_camera.cpp) runs too.  A translation unit of its own: the render kernels', the
// query's and the traced rays' code objects stay as they are.
//
// k_trace_camera<M>: k_trace<STAGED = false, REFILL = true>'s scheme (pt_trace_kernels.hip; the measured default of
// DESIGN.md §13.4) with another ray source.  A persistent grid of 256-thread workgroups, at most what is resident; a
// wave works through a static share of the pixels -- the 64-pixel blocks w, w + Wn, w + 2 Wn, ... for wave w of Wn; no
// atomics, no workspace, no LDS -- behind a wave-uniform cursor: once per iteration the lanes whose pixel has finished
// all its frames take the next pixels of the share (rank in the ballot), then every live lane runs one segment; a lane
// whose path ended folds the colour into its running mean (registers) and starts the next frame by making its ray
// again, where k_trace reloads two quads.  The kernel reads nothing but the scene and an accumulating call's prior,
// and writes one quad per pixel.  M: the model as a template constant, or -1 for the launch-uniform switch that ships
// (DESIGN.md §14.4).
// TWIN: k_trace<false, true> (pt_trace_kernels.hip), the refill loop; and k_film_expose (pt_film_kernels.hip), which
// restates this one (one shared loop moved the registers of all three kernels).
// Shared with the other ray-batch units: the scene accessor, rank_in, the argument-segment read and the
// persistent grid's size come from pt_batch_device.h, the error return, the checks and the staged buffer of the entry
// points from pt_entry.h.
#include "pt_batch_device.h"
#include "pt_camera_launch.h"
#include "pt_entry.h"
#include "pt_scene_pack.h"

#include <cstddef>
#include <type_traits>

namespace ptcam {
namespace {

using ptb::kThreads;
using ptb::kWaves;
using ptb::rank_in;
constexpr int kKernels = 5;                // the switch and the four models

struct CamArgs {
    const float4* nodes;
    const float4* tris;
    const float4* spheres;
    const float4* leaf_tris;
    const float4* mats;
    float4* rgba;
    long long n;                           // W * H
    int n_nodes, n_spheres, scene_fast;
    ptt::Frames fr;
    Prepared cam;
};

// The camera, read back from the argument segment where a ray is made (ptb::load_arg has the why).
__device__ __forceinline__ Prepared load_camera() { return ptb::load_arg<Prepared, offsetof(CamArgs, cam)>(); }

template <int M>
__global__ __launch_bounds__(kThreads) void k_trace_camera(CamArgs a) {
    const ptb::DevScene<CamArgs> sc = {a};
    const ptt::Frames fr = a.fr;
    // the wave's share: cursor position c is pixel (c / 64) * 64 * Wn + 64 * w + c % 64
    const long long w = (long long)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long Wn = (long long)gridDim.x * kWaves;
    const long long n_blocks = (a.n + 63) >> 6;
    const long long c_end = w < n_blocks ? 64 * ((n_blocks - w + Wn - 1) / Wn) : 0;
    long long c = 0;          // wave-uniform
    bool live = false;
    int x = 0, y = 0;         // the lane's pixel: index (unsigned)y * W + x
    f3 o = mk(0, 0, 0), d = o, inc = o, col = o;
    uint32_t state = 0u;
    int bounce = 0, kf = 0;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (;;) {
        const unsigned long long want = __ballot(!live);
        if (want != 0ull && c < c_end) {
            if (!live) {
                const long long cc = c + rank_in(want);
                const long long idx = (cc >> 6) * 64 * Wn + 64 * w + (cc & 63);
                if (cc < c_end && idx < a.n) {           // the share's last block may be the image's ragged tail
                    y = (int)((unsigned)idx / (unsigned)a.cam.W), x = (int)((unsigned)idx - (unsigned)y * (unsigned)a.cam.W);   // idx < W * H <= 2^32
                    kf = 0;
                    state = pt::seed(x, y, fr.frame_first);
                    make_ray<M>(load_camera(), x, y, state, o, d);
                    ptt::start_path(inc, col, bounce);
                    if (fr.acc_first == 1) acc = a.rgba[idx];
                    live = true;
                }
            }
            c += __popcll(want);
        }
        if (__ballot(live) == 0ull) {
            if (c >= c_end) break;
            continue;
        }
        if (live) {
            f3 rgb;
            const bool ended = ptt::segment<float4>(sc, fr, __builtin_huge_valf(), o, d, inc, col, state, bounce, rgb);
            if (ended) {
                acc = pti::accumulate(acc, rgb, fr.frame_first + kf, kf > 0 || fr.acc_first == 1);
                kf++;
                if (kf == fr.n_frames) {
                    a.rgba[(size_t)((unsigned)y * (unsigned)a.cam.W + (unsigned)x)] = acc;
                    live = false;
                } else {                                 // the next frame of the same pixel: its ray anew
                    state = pt::seed(x, y, fr.frame_first + kf);
                    make_ray<M>(load_camera(), x, y, state, o, d);
                    ptt::start_path(inc, col, bounce);
                }
            }
        }
    }
}

// ptb::load_arg's premise: the kernel's one parameter is CamArgs, at offset 0 of the argument segment.
static_assert(std::is_same<decltype(&k_trace_camera<-1>), void (*)(CamArgs)>::value, "CamArgs is the only kernel parameter");

// One thread per pixel: the ray of frame `frame` as two quads, and the state the camera left.
__global__ __launch_bounds__(kThreads) void k_camera_rays(Prepared cam, int frame, long long n, float4* rays, unsigned* states) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int y = (int)((unsigned)i / (unsigned)cam.W), x = (int)((unsigned)i - (unsigned)y * (unsigned)cam.W);   // i < 2^32
    uint32_t state = pt::seed(x, y, frame);
    f3 o, d;
    make_ray(cam, x, y, state, o, d);
    rays[2 * i] = make_float4(o.x, o.y, o.z, __builtin_huge_valf());
    rays[2 * i + 1] = make_float4(d.x, d.y, d.z, 0.0f);
    if (states) states[i] = state;
}

}  // namespace

hipError_t launch_trace_camera(hipStream_t s, const ptt::CtxView& v, const Launch& l) {
    const long long n = (long long)l.cam.W * l.cam.H;
    if (n <= 0) return hipSuccess;
    const ptt::Frames fr = {v.q.flags, v.max_bounce, v.mode, l.frame_first, l.n_frames, l.acc_first};
    const CamArgs a = {v.q.nodes, v.q.tris, v.q.spheres, v.q.leaf_tris, v.mats, l.rgba, n,
                       v.q.n_nodes, v.q.n_spheres, v.q.scene_fast, fr, l.cam};
    void (*fn)(CamArgs) = k_trace_camera<-1>;
    int which = 0;
    if (l.per_model) {
        which = 1 + l.cam.model;
        fn = l.cam.model == PT_CAM_PINHOLE ? k_trace_camera<PT_CAM_PINHOLE>
           : l.cam.model == PT_CAM_THIN_LENS ? k_trace_camera<PT_CAM_THIN_LENS>
           : l.cam.model == PT_CAM_ORTHO ? k_trace_camera<PT_CAM_ORTHO> : k_trace_camera<PT_CAM_EQUIRECT>;
    }
    static ptb::Resident resident[kKernels];
    const unsigned blocks = ptb::persistent_grid((const void*)fn, resident[which], v.q.device, n, l.grid_cap);
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_camera_rays(hipStream_t s, const Prepared& cam, int frame, float4* rays, unsigned* states) {
    const long long n = (long long)cam.W * cam.H;
    if (n <= 0) return hipSuccess;
    const long long blocks = (n + kThreads - 1) / kThreads;       // at most 2^24 for a 65536 x 65536 image
    hipLaunchKernelGGL(k_camera_rays, dim3((unsigned)blocks), dim3(kThreads), 0, s, cam, frame, n, rays, states);
    return hipGetLastError();
}

}  // namespace ptcam

// ===================================================================== entry points
namespace {

int g_grid_cap = 0, g_per_model = 0;       // pt__camera_debug (measurements and tests only)

// the checks both trace entry points share
int check_trace(pt_ctx* c, const pt_camera* cam, int frame_first, int n_frames, int accumulate_first, const void* rgba,
                const char* who, ptt::CtxView& v) {
    if (!c) return PT_E_ARG;
    int rc = pt__trace_view(c, &v);
    if (rc) return rc;
    if ((rc = pte::check_scene(c, v.q, who)) != PT_OK) return rc;
    if ((rc = pte::check_camera(c, cam)) != PT_OK) return rc;
    if ((rc = pte::check_frames(c, frame_first, n_frames, accumulate_first)) != PT_OK) return rc;
    if (!rgba) return pt__query_fail(c, PT_E_ARG, "null rgba");
    return PT_OK;
}

int enqueue(pt_ctx* c, const ptt::CtxView& v, const pt_camera* cam, int frame_first, int n_frames, int accumulate_first,
            void* d_rgba) {
    const ptcam::Launch l = {ptcam::prepare(*cam), (float4*)d_rgba, frame_first, n_frames, accumulate_first, g_grid_cap,
                             g_per_model == 1};
    PTCHK(c, ptcam::launch_trace_camera(v.q.stream, v, l));
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_trace_camera_device(pt_ctx* c, const pt_camera* cam, int frame_first, int n_frames, int accumulate_first,
                           void* d_rgba) {
    ptt::CtxView v;
    const int rc = check_trace(c, cam, frame_first, n_frames, accumulate_first, d_rgba, "pt_trace_camera_device", v);
    if (rc) return rc;
    if ((size_t)d_rgba & 15u) return pt__query_fail(c, PT_E_ARG, "device rgba must be 16-byte aligned");
    PTCHK(c, hipSetDevice(v.q.device));
    return enqueue(c, v, cam, frame_first, n_frames, accumulate_first, d_rgba);
}

int pt_trace_camera(pt_ctx* c, const pt_camera* cam, int frame_first, int n_frames, int accumulate_first, float* rgba) {
    ptt::CtxView v;
    int rc = check_trace(c, cam, frame_first, n_frames, accumulate_first, rgba, "pt_trace_camera", v);
    if (rc) return rc;
    PTCHK(c, hipSetDevice(v.q.device));
    const size_t rgba_bytes = (size_t)cam->width * (size_t)cam->height * 4 * sizeof(float);
    pte::Staged b(v.q.stream);
    void* d_rgba = b.alloc(rgba_bytes);
    // the caller's values are the prior of an accumulating first frame; otherwise rgba is never read
    if (accumulate_first) b.in(d_rgba, rgba, rgba_bytes);
    if (b.ok() && (rc = enqueue(c, v, cam, frame_first, n_frames, accumulate_first, d_rgba)) == PT_OK)
        b.out(rgba, d_rgba, rgba_bytes);
    return b.ok() ? rc : pte::hip_fail(c, "pt_trace_camera", b.e);
}

int pt_camera_rays_device(pt_ctx* c, const pt_camera* cam, int frame, void* d_rays, void* d_states) {
    if (!c) return PT_E_ARG;
    ptt::CtxView v;
    int rc = pt__trace_view(c, &v);
    if (rc) return rc;
    if ((rc = pte::check_camera(c, cam)) != PT_OK) return rc;
    if (frame < 1) return pt__query_fail(c, PT_E_ARG, "frame must be >= 1");
    if (!d_rays || ((size_t)d_rays & 15u) || ((size_t)d_states & 3u))
        return pt__query_fail(c, PT_E_ARG, "device rays must be non-null and 16-byte aligned, states 4-byte aligned");
    PTCHK(c, hipSetDevice(v.q.device));
    PTCHK(c, ptcam::launch_camera_rays(v.q.stream, ptcam::prepare(*cam), frame, (float4*)d_rays, (unsigned*)d_states));
    return PT_OK;
}

// Measurements and tests only (tools/camera_measure.py, tests/test_gpu_camera.py), not part of the public ABI: a
// ptcam::Debug setting for every later camera trace of the process.
int pt__camera_debug(int what, int value) {
    if (what == ptcam::kDebugGridCap && value >= 0) g_grid_cap = value;
    else if (what == ptcam::kDebugPerModel && value >= 0 && value <= 1) g_per_model = value;
    else return PT_E_ARG;
    return PT_OK;
}

}  // extern "C"
