// pt_query_kernels.hip -- the device half of the ray query (include/pt_api.h: pt_intersect, pt_intersect_device,
// pt_pick) and its entry points.  One ray per lane runs ptq::cast (pt_query.h), the per-ray code the
// host twin (pt_query.cpp) runs too.  A translation unit of its own: the render kernels' code object stays as it is.
//
// k_cast<ANY, STAGED>: a grid-stride loop over the rays.  STAGED: every workgroup first copies the first
// min(n_nodes, ptp::kTopNodes) node records of kNodes -- the breadth-first top of the tree, which the device numbering
// exists for -- into LDS (at most 24 KiB, as two planes like the render's global-memory walk); a walk reads those from
// LDS and the nodes beyond from global memory, one 16-byte load per quad.  The link choice is a select; the leaf's
// triangle tests run under the exec mask of the lanes whose box test passed at a leaf.
// Shared with the other ray-batch units: the scene accessor and the workgroup shape come from
// pt_batch_device.h, the error return, the checks and the staged buffers of the entry points from pt_entry.h.
#include "pt_batch_device.h"
#include "pt_entry.h"
#include "pt_query.h"
#include "pt_query_launch.h"
#include "pt_scene_pack.h"

#include <vector>

namespace ptq {
namespace {

using ptb::kThreads;
constexpr unsigned kMaxBlocks = 2048;  // 8 workgroups per CU of the 256; the loop strides over the rest

struct CastArgs {
    const float4* nodes;
    const float4* tris;
    const float4* spheres;
    const float4* leaf_tris;
    const float4* rays;
    float4* hits;
    long long n;
    int n_nodes, n_spheres, n_top, scene_fast, flags;
};

template <bool ANY, bool STAGED>
__global__ __launch_bounds__(kThreads) void k_cast(CastArgs a) {
    __shared__ float4 s_top[STAGED ? 2 * ptp::kTopNodes : 1];
    if (STAGED) {
        for (int i = (int)threadIdx.x; i < 2 * a.n_top; i += kThreads) {
            const int node = i >> 1, half = i & 1;       // consecutive lanes read consecutive quads
            s_top[half * a.n_top + node] = a.nodes[i];
        }
        __syncthreads();
    }
    const ptb::DevScene<CastArgs, STAGED> sc = {a, s_top};
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += stride) {
        const float4 r0 = a.rays[2 * i], r1 = a.rays[2 * i + 1];
        const Hit h = cast<float4>(sc, mk(r0.x, r0.y, r0.z), mk(r1.x, r1.y, r1.z), r0.w, a.flags, ANY);
        a.hits[3 * i] = make_float4(h.t, __int_as_float(h.kind), __int_as_float(h.prim), __int_as_float(h.mat));
        a.hits[3 * i + 1] = make_float4(h.n.x, h.n.y, h.n.z, 0.0f);
        a.hits[3 * i + 2] = make_float4(h.p.x, h.p.y, h.p.z, 0.0f);
    }
}

}  // namespace

hipError_t launch_cast(hipStream_t s, const CtxView& v, const Launch& l) {
    if (l.n <= 0) return hipSuccess;
    const int n_top = v.n_nodes < ptp::kTopNodes ? v.n_nodes : ptp::kTopNodes;
    const CastArgs a = {v.nodes, v.tris, v.spheres, v.leaf_tris, l.rays, l.hits, l.n,
                        v.n_nodes, v.n_spheres, n_top, v.scene_fast, v.flags};
    const long long want = (l.n + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(want < (long long)kMaxBlocks ? want : (long long)kMaxBlocks)), block(kThreads);
    const bool staged = l.staged && n_top > 0;
    if (l.any_hit) {
        if (staged) hipLaunchKernelGGL((k_cast<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_cast<true, false>), grid, block, 0, s, a);
    } else {
        if (staged) hipLaunchKernelGGL((k_cast<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_cast<false, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace ptq

// ===================================================================== entry points
namespace {

int g_query_variant = ptq::kAuto;     // pt__query_debug (measurements only)

// the checks every entry point shares; n = 0 is the caller's early PT_OK
int check_query(pt_ctx* c, const void* in, long long n, const void* out, int query_flags, const char* who,
                ptq::CtxView& v) {
    if (!c) return PT_E_ARG;
    int rc = pt__query_view(c, &v);
    if (rc) return rc;
    if ((rc = pte::check_scene(c, v, who)) != PT_OK) return rc;
    if (n < 0) return pt__query_fail(c, PT_E_ARG, "negative ray count");
    if (query_flags & ~PT_QUERY_ANY_HIT) return pt__query_fail(c, PT_E_ARG, "unknown query flags");
    if (n > 0 && (!in || !out)) return pt__query_fail(c, PT_E_ARG, "null array with a nonzero count");
    return PT_OK;
}

int enqueue(pt_ctx* c, const ptq::CtxView& v, const void* d_rays, long long n, void* d_hits, int query_flags) {
    const bool staged = g_query_variant != ptq::kGlobal && v.kernel_variant != 3;
    const ptq::Launch l = {(const float4*)d_rays, (float4*)d_hits, n, (query_flags & PT_QUERY_ANY_HIT) != 0, staged};
    PTCHK(c, ptq::launch_cast(v.stream, v, l));
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_intersect_device(pt_ctx* c, const void* d_rays, long long n, void* d_hits, int query_flags) {
    ptq::CtxView v;
    const int rc = check_query(c, d_rays, n, d_hits, query_flags, "pt_intersect_device", v);
    if (rc || n == 0) return rc;
    if (((size_t)d_rays | (size_t)d_hits) & 15u) return pt__query_fail(c, PT_E_ARG, "device arrays must be 16-byte aligned");
    PTCHK(c, hipSetDevice(v.device));
    return enqueue(c, v, d_rays, n, d_hits, query_flags);
}

int pt_intersect(pt_ctx* c, const pt_ray* rays, long long n, pt_hit* hits, int query_flags) {
    ptq::CtxView v;
    int rc = check_query(c, rays, n, hits, query_flags, "pt_intersect", v);
    if (rc || n == 0) return rc;
    PTCHK(c, hipSetDevice(v.device));
    pte::Staged b(v.stream);
    void* d_rays = b.alloc((size_t)n * sizeof(pt_ray));
    void* d_hits = b.alloc((size_t)n * sizeof(pt_hit));
    b.in(d_rays, rays, (size_t)n * sizeof(pt_ray));
    if (b.ok() && (rc = enqueue(c, v, d_rays, n, d_hits, query_flags)) == PT_OK)
        b.out(hits, d_hits, (size_t)n * sizeof(pt_hit));
    return b.ok() ? rc : pte::hip_fail(c, "pt_intersect", b.e);
}

int pt_pick(pt_ctx* c, const int* xy, long long n, pt_hit* hits) {
    ptq::CtxView v;
    const int rc = check_query(c, xy, n, hits, 0, "pt_pick", v);
    if (rc) return rc;
    if (!v.cam_ok) return pt__query_fail(c, PT_E_STATE, "pt_pick before pt_set_camera");
    if (n == 0) return PT_OK;
    std::vector<pt_ray> rays((size_t)n);
    for (long long i = 0; i < n; i++) ptq::pixel_ray(v.cam, v.width, v.height, xy[2 * i], xy[2 * i + 1], &rays[(size_t)i]);
    return pt_intersect(c, rays.data(), n, hits, 0);
}

// Measurements only (tools/query_measure.py), not part of the public ABI: ptq::Variant for every later query.
int pt__query_debug(int variant) {
    if (variant != ptq::kAuto && variant != ptq::kGlobal) return PT_E_ARG;
    g_query_variant = variant;
    return PT_OK;
}

}  // extern "C"
