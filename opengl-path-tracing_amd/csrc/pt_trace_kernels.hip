// pt_trace_kernels.hip -- the device half of traced rays (include/pt_api.h: pt_trace, pt_trace_device; DESIGN.md
// §13) and its entry points.  A lane holds one ray and runs ptt::segment (pt_trace.h) -- ptq::cast, then ptt::shade --
// the per-ray code the host twin (pt_trace.cpp) runs too.  A translation unit of its own: the render kernels' and the
// query's code objects stay as they are.
//
// k_trace<STAGED, REFILL>: a persistent grid of 256-thread workgroups, at most what is resident.  STAGED: every
// workgroup first copies the first min(n_nodes, ptp::kTopNodes) node records into LDS, exactly as k_cast does; the
// workgroups are persistent, so the copy is paid once per launch.  Measured slower than the unstaged walk on every
// scene, so only pt__trace_debug selects it.
//
// REFILL: a path has up to max_bounce + 1 segments and a ray n_frames paths, so a lane that ran one ray to its end
// would idle until its wave's longest ray ends.  Instead a wave works through a static share of the rays -- the
// 64-ray blocks w, w + Wn, w + 2 Wn, ... for wave w of Wn; no atomics, no workspace -- behind a wave-uniform cursor:
// once per iteration the lanes whose ray has finished all its frames take the next rays of the share (rank in the
// ballot), then every live lane runs one segment; a lane whose path ended folds the colour into its running mean
// (registers) and restarts the next frame from the ray, which it reloads.  Frames of a ray stay in order.
// !REFILL: a plain grid-stride loop, one ray per lane to the end (ptt::trace_frames).
// Shared with the other ray-batch units: the scene accessor, rank_in and the persistent grid's size
// come from pt_batch_device.h, the error return, the checks and the staged buffers of the entry points from pt_entry.h.
// The staging prologue and the refill loop are restated on purpose: §16.2.
#include "pt_batch_device.h"
#include "pt_entry.h"
#include "pt_trace.h"
#include "pt_trace_launch.h"
#include "pt_scene_pack.h"

namespace ptt {
namespace {

using ptb::kThreads;
using ptb::kWaves;
using ptb::rank_in;

struct TraceArgs {
    const float4* nodes;
    const float4* tris;
    const float4* spheres;
    const float4* leaf_tris;
    const float4* mats;
    const float4* rays;
    const unsigned* seeds;
    float4* rgba;
    long long n;
    int n_nodes, n_spheres, n_top, scene_fast;
    Frames fr;
};

__device__ __forceinline__ uint32_t seed_of(const TraceArgs& a, long long i) {
    return a.seeds ? a.seeds[i] : default_seed(i);
}

template <bool STAGED, bool REFILL>
__global__ __launch_bounds__(kThreads) void k_trace(TraceArgs a) {
    __shared__ float4 s_top[STAGED ? 2 * ptp::kTopNodes : 1];
    if (STAGED) {
        for (int i = (int)threadIdx.x; i < 2 * a.n_top; i += kThreads) {
            const int node = i >> 1, half = i & 1;       // consecutive lanes read consecutive quads
            s_top[half * a.n_top + node] = a.nodes[i];
        }
        __syncthreads();
    }
    const ptb::DevScene<TraceArgs, STAGED> sc = {a, s_top};
    const Frames fr = a.fr;
    if (!REFILL) {
        const long long stride = (long long)gridDim.x * kThreads;
        for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += stride) {
            const float4 r0 = a.rays[2 * i], r1 = a.rays[2 * i + 1];
            float4 prior = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (fr.acc_first == 1) prior = a.rgba[i];
            a.rgba[i] = trace_frames<float4>(sc, fr, mk(r0.x, r0.y, r0.z), mk(r1.x, r1.y, r1.z), r0.w, seed_of(a, i), prior);
        }
        return;
    }
    // TWIN: k_trace_camera (pt_camera_kernels.hip) restates this refill loop with the ray made by the lane, not loaded
    // (one shared loop moved the registers of all three kernels).
    // the wave's share: cursor position c is ray (c / 64) * 64 * Wn + 64 * w + c % 64
    const long long w = (long long)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long Wn = (long long)gridDim.x * kWaves;
    const long long n_blocks = (a.n + 63) >> 6;
    const long long c_end = w < n_blocks ? 64 * ((n_blocks - w + Wn - 1) / Wn) : 0;
    long long c = 0;          // wave-uniform
    bool live = false;
    long long i = 0;
    f3 o = mk(0, 0, 0), d = o, inc = o, col = o;
    uint32_t state = 0u;
    int bounce = 0, kf = 0;
    float t_start = 0.0f;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (;;) {
        const unsigned long long want = __ballot(!live);
        if (want != 0ull && c < c_end) {
            if (!live) {
                const long long cc = c + rank_in(want);
                const long long idx = (cc >> 6) * 64 * Wn + 64 * w + (cc & 63);
                if (cc < c_end && idx < a.n) {           // the share's last block may be the batch's ragged tail
                    i = idx;
                    const float4 r0 = a.rays[2 * i], r1 = a.rays[2 * i + 1];
                    o = mk(r0.x, r0.y, r0.z), d = mk(r1.x, r1.y, r1.z), t_start = r0.w;
                    kf = 0;
                    state = frame_state(seed_of(a, i), fr.frame_first);
                    start_path(inc, col, bounce);
                    if (fr.acc_first == 1) acc = a.rgba[i];
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
            const bool ended = segment<float4>(sc, fr, t_start, o, d, inc, col, state, bounce, rgb);
            t_start = __builtin_huge_valf();
            if (ended) {
                acc = pti::accumulate(acc, rgb, fr.frame_first + kf, kf > 0 || fr.acc_first == 1);
                kf++;
                if (kf == fr.n_frames) {
                    a.rgba[i] = acc;
                    live = false;
                } else {                                 // the next frame of the same ray
                    const float4 r0 = a.rays[2 * i], r1 = a.rays[2 * i + 1];
                    o = mk(r0.x, r0.y, r0.z), d = mk(r1.x, r1.y, r1.z), t_start = r0.w;
                    state = frame_state(seed_of(a, i), fr.frame_first + kf);
                    start_path(inc, col, bounce);
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_trace(hipStream_t s, const CtxView& v, const Launch& l) {
    if (l.n <= 0) return hipSuccess;
    const int n_top = v.q.n_nodes < ptp::kTopNodes ? v.q.n_nodes : ptp::kTopNodes;
    const Frames fr = {v.q.flags, v.max_bounce, v.mode, l.frame_first, l.n_frames, l.acc_first};
    const TraceArgs a = {v.q.nodes, v.q.tris, v.q.spheres, v.q.leaf_tris, v.mats, l.rays, l.seeds, l.rgba, l.n,
                         v.q.n_nodes, v.q.n_spheres, n_top, v.q.scene_fast, fr};
    const bool staged = l.staged && n_top > 0;
    void (*fn)(TraceArgs) = staged ? (l.refill ? k_trace<true, true> : k_trace<true, false>)
                                   : (l.refill ? k_trace<false, true> : k_trace<false, false>);
    static ptb::Resident resident[4];
    const unsigned blocks = ptb::persistent_grid((const void*)fn, resident[(staged ? 2 : 0) + (l.refill ? 1 : 0)],
                                                 v.q.device, l.n, l.grid_cap);
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace ptt

// ===================================================================== entry points
namespace {

int g_staging = 0, g_refill = 0, g_grid_cap = 0;     // pt__trace_debug (measurements and tests only)

// the checks both entry points share; n = 0 is the caller's early PT_OK
int check_trace(pt_ctx* c, const void* rays, long long n, int frame_first, int n_frames, int accumulate_first,
                const void* rgba, const char* who, ptt::CtxView& v) {
    if (!c) return PT_E_ARG;
    int rc = pt__trace_view(c, &v);
    if (rc) return rc;
    if ((rc = pte::check_scene(c, v.q, who)) != PT_OK) return rc;
    if (n < 0) return pt__query_fail(c, PT_E_ARG, "negative ray count");
    if ((rc = pte::check_frames(c, frame_first, n_frames, accumulate_first)) != PT_OK) return rc;
    if (n > 0 && (!rays || !rgba)) return pt__query_fail(c, PT_E_ARG, "null array with a nonzero count");
    return PT_OK;
}

int enqueue(pt_ctx* c, const ptt::CtxView& v, const void* d_rays, const void* d_seeds, long long n, int frame_first,
            int n_frames, int accumulate_first, void* d_rgba) {
    // the defaults are the measured ones: refill, and the walk unstaged -- the staged top costs a
    // wave of occupancy per SIMD and was slower on every scene, so it stays behind the debug hook only
    const bool staged = g_staging == 1;
    const bool refill = g_refill != 2;
    const ptt::Launch l = {(const float4*)d_rays, (const unsigned*)d_seeds, (float4*)d_rgba, n, frame_first, n_frames,
                           accumulate_first, staged, refill, g_grid_cap};
    PTCHK(c, ptt::launch_trace(v.q.stream, v, l));
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_trace_device(pt_ctx* c, const void* d_rays, const void* d_seeds, long long n, int frame_first, int n_frames,
                    int accumulate_first, void* d_rgba) {
    ptt::CtxView v;
    const int rc = check_trace(c, d_rays, n, frame_first, n_frames, accumulate_first, d_rgba, "pt_trace_device", v);
    if (rc || n == 0) return rc;
    if ((((size_t)d_rays | (size_t)d_rgba) & 15u) || ((size_t)d_seeds & 3u))
        return pt__query_fail(c, PT_E_ARG, "device rays and rgba must be 16-byte aligned, seeds 4-byte aligned");
    PTCHK(c, hipSetDevice(v.q.device));
    return enqueue(c, v, d_rays, d_seeds, n, frame_first, n_frames, accumulate_first, d_rgba);
}

int pt_trace(pt_ctx* c, const pt_ray* rays, const unsigned* seeds, long long n, int frame_first, int n_frames,
             int accumulate_first, float* rgba) {
    ptt::CtxView v;
    int rc = check_trace(c, rays, n, frame_first, n_frames, accumulate_first, rgba, "pt_trace", v);
    if (rc || n == 0) return rc;
    PTCHK(c, hipSetDevice(v.q.device));
    const size_t ray_bytes = (size_t)n * sizeof(pt_ray), seed_bytes = (size_t)n * sizeof(unsigned);
    const size_t rgba_bytes = (size_t)n * 4 * sizeof(float);
    pte::Staged b(v.q.stream);
    void* d_rays = b.alloc(ray_bytes);
    void* d_rgba = b.alloc(rgba_bytes);
    void* d_seeds = seeds ? b.alloc(seed_bytes) : nullptr;
    b.in(d_rays, rays, ray_bytes);
    if (seeds) b.in(d_seeds, seeds, seed_bytes);
    // the caller's values are the prior of an accumulating first frame; otherwise rgba is never read
    if (accumulate_first) b.in(d_rgba, rgba, rgba_bytes);
    if (b.ok() && (rc = enqueue(c, v, d_rays, d_seeds, n, frame_first, n_frames, accumulate_first, d_rgba)) == PT_OK)
        b.out(rgba, d_rgba, rgba_bytes);
    return b.ok() ? rc : pte::hip_fail(c, "pt_trace", b.e);
}

// Measurements and tests only (tools/trace_measure.py, tests/test_gpu_trace.py), not part of the public ABI: a
// ptt::Debug setting for every later trace of the process.
int pt__trace_debug(int what, int value) {
    if (what == ptt::kDebugStaging && value >= 0 && value <= 2) g_staging = value;
    else if (what == ptt::kDebugRefill && value >= 0 && value <= 2) g_refill = value;
    else if (what == ptt::kDebugGridCap && value >= 0) g_grid_cap = value;
    else return PT_E_ARG;
    return PT_OK;
}

}  // extern "C"
