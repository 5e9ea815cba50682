// pt_trace_launch.h -- what pt_trace_kernels.hip and pt_render.hip know of each other.  The traced rays' kernel and
// entry points (pt_trace, pt_trace_device) are a translation unit of their own, like the ray query's, so the render
// kernels' code object does not change with them; pt_render.hip, which owns pt_ctx, hands out a read-only view.
#pragma once

#include "pt_query_launch.h"

namespace ptt {

// The query's view with what a path reads beside it.
struct CtxView {
    ptq::CtxView q;
    const float4* mats;        // ptp::kMats
    int max_bounce, mode;      // pt_config::max_bounce, the display mode as last set
};

// pt__trace_debug(what, value) (tools/trace_measure.py and the tests; not part of the public ABI)
enum Debug {
    kDebugStaging = 0,         // value: 0 = the default (unstaged), 1 = the top of the tree staged in LDS, 2 = unstaged
    kDebugRefill = 1,          // value: 0 = the default, 1 = refill between segments, 2 = the plain loop
    kDebugGridCap = 2          // value: at most this many workgroups; 0 = no cap
};

struct Launch {
    const float4* rays;        // 2 quads per ray
    const unsigned* seeds;     // or null: ptt::default_seed
    float4* rgba;              // in/out
    long long n;
    int frame_first, n_frames, acc_first;
    bool staged, refill;
    int grid_cap;              // 0 = none
};

// Enqueues the trace of l.n rays on `s`; hipSuccess or the launch error.  Allocates and copies nothing.
hipError_t launch_trace(hipStream_t s, const CtxView& v, const Launch& l);

}  // namespace ptt

extern "C" {
// pt_render.hip, not part of the public ABI: the view of a context, changing nothing in it.
int pt__trace_view(const pt_ctx* c, ptt::CtxView* out);
// ... and the count of scene replacements (pt_upload_scene bumps it on success): what a film's guides depend on.
int pt__scene_serial(const pt_ctx* c, unsigned long long* out);
}
