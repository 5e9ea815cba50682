// pt_query_launch.h -- what pt_query_kernels.hip and pt_render.hip know of each other.  The ray query's kernel and its
// entry points (pt_intersect, pt_intersect_device, pt_pick) are a translation unit of their own, so the render kernels'
// code object does not change with them; pt_render.hip, which owns pt_ctx, hands out a read-only view of a context.
#pragma once

#include "../../include/pt_api.h"

#include <hip/hip_runtime.h>

namespace ptq {

// How the walk reads the first ptp::kTopNodes node records: kAuto = staged in LDS unless the context's kernel variant
// keeps scenes in global memory (pt_set_kernel 3), kGlobal = never staged (tools/query_measure.py compares them
// through pt__query_debug).
enum Variant { kAuto = 0, kGlobal = 1 };

struct CtxView {
    const float4* nodes;       // ptp::kNodes
    const float4* tris;        // ptp::kTris
    const float4* spheres;     // ptp::kSpheres
    const float4* leaf_tris;   // ptp::kLeafTris
    int n_nodes, n_spheres, scene_fast;
    int flags;                 // the context's PT_FLAG_*
    int kernel_variant;        // pt_set_kernel
    int device, width, height;
    float cam[12];             // the derived basis {pos, fwd, right, up}
    bool scene_ok, cam_ok;
    hipStream_t stream;
};

struct Launch {
    const float4* rays;        // 2 quads per ray
    float4* hits;              // 3 quads per hit
    long long n;
    bool any_hit, staged;
};

// Enqueues the cast of l.n rays on `s`; hipSuccess or the launch error.
hipError_t launch_cast(hipStream_t s, const CtxView& v, const Launch& l);

}  // namespace ptq

extern "C" {
// pt_render.hip, not part of the public ABI: the view of a context, changing nothing in it; and its error string.
int pt__query_view(const pt_ctx* c, ptq::CtxView* out);
int pt__query_fail(pt_ctx* c, int code, const char* msg);
}
