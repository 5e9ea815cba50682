// pt_film_launch.h -- what pt_film_kernels.hip's entry points and launchers agree on.  The film's kernels and entry
// points (pt_film_*) are a translation unit of their own, like the camera models', so the render's, the query's, the
// trace's, the camera's and the denoiser's code objects do not change with them; they reach a context only through
// pt__trace_view and pt__scene_serial (pt_trace_launch.h).
#pragma once

#include "pt_camera_launch.h"
#include "pt_film.h"

namespace ptfilm {

// pt__film_debug(what, value) (tools/film_measure.py and the tests; not part of the public ABI)
enum Debug {
    kDebugGridCap = 0,         // value: at most this many workgroups; 0 = no cap
    kDebugMoments = 1          // value: 0 = the default, 1 = the moments in registers beside the running mean, stored
                               //        with the pixel, 2 = read-modify-write in global memory at each path end
                               //        (the measurement of DESIGN.md §15.4)
};

struct Launch {
    ptcam::Prepared cam;
    float4* rgba;              // in/out, cam.W * cam.H quads
    float2* moments;           // in/out, (S1, S2) per pixel
    float4* g0;                // in/out in the guide frames: (N.rgb, Z)
    float4* g1;                //                             (A.rgb, 0)
    int frame_first, n_frames, acc_first;
    GuideRange guides;         // the frames whose first hit is folded into g0, g1
    bool guides_only;          // paths end after the first segment; rgba and moments are not touched
    bool moments_in_regs;
    int grid_cap;              // 0 = none
};

// Enqueues the exposure of every pixel on `s`; hipSuccess or the launch error.  Allocates and copies nothing.
hipError_t launch_expose(hipStream_t s, const ptt::CtxView& v, const Launch& l);
// The noise summary of n pixels' moments after `frames` frames into the zeroed block `out`.
hipError_t launch_noise(hipStream_t s, int device, const float2* moments, long long n, int frames, unsigned target_q,
                        pt_noise_stats* out);
// pti::aces_px of n pixels.
hipError_t launch_aces(hipStream_t s, const float4* src, uchar4* dst, long long n);

}  // namespace ptfilm
