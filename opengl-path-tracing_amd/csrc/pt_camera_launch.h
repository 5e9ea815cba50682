// pt_camera_launch.h -- what pt_camera_kernels.hip's entry points and launchers agree on.  The camera models' kernels
// and entry points (pt_trace_camera, pt_trace_camera_device, pt_camera_rays_device) are a translation unit of their
// own, like the traced rays', so the render's, the query's and the trace's code objects do not change with them; they
// reach a context only through pt__trace_view (pt_trace_launch.h).
#pragma once

#include "pt_camera.h"
#include "pt_trace_launch.h"

namespace ptcam {

// pt__camera_debug(what, value) (tools/camera_measure.py and the tests; not part of the public ABI)
enum Debug {
    kDebugGridCap = 0,         // value: at most this many workgroups; 0 = no cap
    kDebugPerModel = 1         // value: 0 = the default (one kernel, the model a run-time switch), 1 = the kernel
                               //        instantiated per model (the measurement of DESIGN.md §14.4)
};

struct Launch {
    Prepared cam;
    float4* rgba;              // in/out, cam.W * cam.H quads
    int frame_first, n_frames, acc_first;
    int grid_cap;              // 0 = none
    bool per_model;
};

// Enqueues the trace of every pixel on `s`; hipSuccess or the launch error.  Allocates and copies nothing.
hipError_t launch_trace_camera(hipStream_t s, const ptt::CtxView& v, const Launch& l);
// Enqueues the rays (and, where states is not null, the states) of every pixel of frame `frame`.
hipError_t launch_camera_rays(hipStream_t s, const Prepared& cam, int frame, float4* rays, unsigned* states);

}  // namespace ptcam
