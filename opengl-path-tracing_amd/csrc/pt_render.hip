// pt_render.hip -- the path-tracing hot path on MI355X (gfx950) behind the pt_api.h C ABI.
//
// Replaces LearnOpenGL/computeShader.c (main :505-554, Trace :434-501,
// calculateRayCollision :367-432, bvh_intersect :309-365, hit_triangle :274-307,
// hit_sphere :209-226, RNG :87-129) and the GL plumbing that drives it
// (ogl_path_trace.h:160-204, 367-530).  Results are bit-identical to the CPU oracle's
// restatement of those semantics; every float op is pinned via pt_math.h
// and -ffp-contract=off.
//
// Device layouts, built once per upload from the std140 records (pt_scene_pack.cpp):
//   node  32 B : {min.x, max.x, min.y, max.y}, {min.z, max.z, a, b}   (axis-paired so a
//                slab axis is one packed-f32 register pair)
//                internal: a = hit link (left child), b = miss
//                leaf:     a = ~(slot<<1 | single), b = next
//   tri   64 B : {n.xyz, d0}, {v0.xyz, cont}, {v1.xyz, matIdx}, {v2.xyz, 0}
//                n = normalize(cross(v1-v0, v2-v0)) and d0 = -dot(n, v0) are the exact values
//                hit_triangle recomputes per call; a leaf's triangles sit in slots 2k, 2k+1;
//                the plane test reads one quad, shading two (quads 0 and 2).  cont: the LDS
//                walk's continuation of the leaf (first slot only).
//   leaf code  : k << 2 | coplanar << 1 | single (k = leaf pair index, slots 2k and 2k+1)
//   mat   48 B : {color.rgb, smoothness}, {emission*strength, specProb}, {specular.rgb, 0}
//   sphere 32 B: {c.xyz, r*r}, {matIdx, 0, 0, 0}
#include "pt_cull.h"
#include "pt_denoise_launch.h"
#include "pt_isect.h"
#include "pt_launch_plan.h"
#include "pt_math.h"
#include "pt_noise.h"
#include "pt_pool.h"
#include "pt_query_launch.h"
#include "pt_render_kernels.h"
#include "pt_scene_pack.h"
#include "pt_wide.h"
#include "../../include/pt_api.h"
#include "../../include/pt_scene.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using pt::f3;
using pt::mk;
using ptl::kAccumPix;
using ptl::kAccumPixLong;
using ptl::kPadNodes;
using ptl::kPullBatch;

// The device half, as sections of this translation unit (one compile, one set of kernel symbols):
#include "pt_kparams.h"        // DevScene, KParams, Cnt, SceneView, the queue-head stride
#include "pt_render_phase.h"   // what both render kernels run: the launch-uniform facts, the shared pieces of SHADE and LEAF
#include "pt_render_sm.h"      // k_render_sm: scene access, the leaf tests, the three walks, the state machine
#include "pt_render_pool.h"    // k_render_pool: the swept line with the path state in a per-wave LDS pool
#include "pt_post_kernels.h"   // k_advance_frames, k_tile_order, k_accum_frames, k_aces, k_noise

// ===================================================================== host side
// Launch policy (LDS staging, workgroup, group, queue batch, the kernel key) lives in
// pt_launch_plan.{h,cpp}; this file fills KParams from its plan and does the stateful work.
using ptl::kAutoSlots;
using ptl::kMaxSlots;
using ptl::kShortLaunch;
// Scratch ring of overlapped launches: each launch takes the next entry (colour scratch, queue
// head, render / accumulate events) of a ring kRingMult times as long as the render streams, so
// a render waits for the accumulate pass of the launch kRingMult * slots back, not of the one
// that last used its stream (which the stream order already puts before it).
constexpr int kRingMult = 2, kRingMax = kRingMult * kMaxSlots;
constexpr size_t kQueueSet = kQueueStride;   // unsigned per queue head

constexpr int kPresentBufs = 4;   // pt_present_begin buffers

struct pt_ctx {
    pt_config cfg{};
    int rows_local = 0;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev_free;                               // recycled events
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending;     // launches not yet synced
    double total_ms = 0.0;
    int n_launches = 0;
    float4* accum = nullptr;
    uchar4* rgba8 = nullptr;
    float4* d_scene[ptp::kBufsAll] = {};   // the device scene (ptp::SceneBuf); null: the scene has no such buffer
    ptl::SceneFacts sf;             // what ptp::pack_scene learned (the launch planner's input)
    ptl::Tuning tun;                // pt_set_tuning values and the kernel variant
    unsigned long long* d_counters = nullptr;
    unsigned int* d_work = nullptr;
    int* d_frame = nullptr;                      // progressive graph frame counter
    // adaptive queue order ("longest first"): per-tile segment counts measured by the
    // previous renders order the next render's 8x8 tiles so cheap tiles form the tail
    unsigned* d_tile_cost = nullptr;
    unsigned* d_tile_perm = nullptr;
    int n_tiles = 0, tiles_x = 1;
    int tile_shift = 0, tile_key = 0;   // tile shape (KParams::tile_shift) and tuning key 20 (0 = automatic)
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int graph_frames = 0;
    unsigned persist_blocks = 2048;
    int order_skip = 0;             // short launches since the last tile-order sort
    bool order_sorted = false;      // a sort ran since the scene upload
    // k_tile_order launches since the scene upload (pt_debug_tile_order): enqueued directly, and
    // per replay of the captured graph
    unsigned long long n_sorts = 0, graph_sorts = 0;
    int n_cu = 0;
    float* d_rgb = nullptr;        // per-(frame, pixel) colours of the frame-split mode
    size_t rgb_bytes = 0;
    // overlapped short launches (enqueue_render): the render kernels of consecutive short
    // renders rotate over `tun.overlap_slots` streams with their own colour scratch and queue counter,
    // so frame f+1 renders while frame f's launch drains; k_accum_frames stays on `stream`
    // (created with the highest priority, so its small grid is dispatched as soon as render
    // blocks retire) in frame order
    hipStream_t rstream[kMaxSlots] = {};
    float* slot_rgb[kRingMax] = {};
    size_t slot_rgb_bytes[kRingMax] = {};
    hipEvent_t ev_rdone[kRingMax] = {}, ev_adone[kRingMax] = {};
    // main-stream fence an overlapped render waits for: recorded after every tile-order sort
    // and graph replay (the writers of tile_perm, which the render reads)
    hipEvent_t ev_fence = nullptr;
    bool adone_rec[kRingMax] = {}, fence_rec = false;
    int slot = 0;
    int ring = 0;                   // next scratch-ring entry of an overlapped launch
    // a captured graph bakes in the scratch pointer it was captured with: that buffer stays
    // alive (owned here once ensure_rgb has moved on to a larger one) until drop_graph
    float* graph_rgb = nullptr;
    std::vector<float*> graph_owned;
    bool scene_ok = false, cam_ok = false, counting = false;
    float cam[12] = {0};
    float last_ms = 0.0f;
    unsigned long long last_counts[16] = {0};
    unsigned long long n_line_launches[2] = {0, 0};   // render launches enqueued on a generic / a COMMON line (pt_debug_launches)
    bool count_pending = false;
    bool last_swept = false;        // the last render launch enqueued ran the leaf sweep (pt_debug_sweep)
    bool last_pooled = false;       // ... ran k_render_pool (pt_debug_pool)
    // asynchronous presentation (pt_present_begin / _end): per buffer a pinned host image and
    // its copy event; the device view is rgba8 (one, as the copies and the passes that write
    // it are ordered on the context stream)
    unsigned char* present_host[kPresentBufs] = {};
    hipEvent_t ev_copied[kPresentBufs] = {};
    bool present_pending[kPresentBufs] = {};
    // The accumulate pass writes the ACES view into rgba8 beside the running mean when the
    // caller presented after the previous render (aces_fuse, from `presented`); stage_ok: rgba8
    // holds the view of the current image (set by such a pass, cleared by anything that may
    // change the image or rgba8 afterwards).
    bool presented = false, aces_fuse = false, stage_ok = false;
    // noise estimate (pt_set_moments): the luminance moments beside accum, the frames folded
    // into them since the image last restarted (host count), and the summary's device block
    // and pinned host copy (k_noise)
    float2* moments = nullptr;
    int mom_frames = 0;
    pt_noise_stats* d_noise = nullptr;
    pt_noise_stats* h_noise = nullptr;
    // adaptive sampling (pt_render_adaptive): the moments hold per-tile frame counts since the last adaptive run
    // (mom_frames is then the largest) until the image restarts; the per-tile frame map, the two lists of active
    // tiles a batch reads and writes, and the call's summary block with its pinned host copy -- all sized by the tile
    // grid and dropped with it (set_tiles)
    bool mom_mixed = false;
    unsigned* d_tile_frames = nullptr;
    unsigned* d_active[2] = {nullptr, nullptr};
    AdaptSum* d_adapt = nullptr;
    AdaptSum* h_adapt = nullptr;
    int adapt_done = 0;             // frames_done of the adaptive call the per-tile counts are from
    // denoised view (pt_denoise): the two guide planes (N.rgb, Z) and (A.rgb, 0) with the guide_frames
    // they hold, the filter's ping-pong state planes, its result and the result's ACES view.  The three rendered
    // guide images pass through dn_state[0], dn_state[1] and dn_out on their way into the guide planes.
    float4* dn_guide[2] = {nullptr, nullptr};
    float4* dn_state[2] = {nullptr, nullptr};
    float4* dn_out = nullptr;
    uchar4* dn_rgba8 = nullptr;
    bool guides_ok = false, dn_done = false;
    int guides_frames = 0;
    int dn_variant = 0;             // ptd::Variant (pt__denoise_debug; measurements only)
    bool dn_timing = false;         // ... and events around the guide render, the prep and every iteration
    hipEvent_t dn_ev[ptd::kMaxIterations + 3] = {};
    int dn_ev_n = 0;
    std::string err;
};

// Queue-order entry of linear tile t (row-major 8x8 tiles): (ty << 16) | tx, so the kernel
// decodes a tile without an integer division.
static unsigned pack_tile(const pt_ctx* c, unsigned t) {
    return ((t / (unsigned)c->tiles_x) << 16) | (t % (unsigned)c->tiles_x);
}


static void drop_graph(pt_ctx* c);   // a captured graph bakes in scene/camera/config
static int ensure_tiles(pt_ctx* c);  // the tile shape this context's next launch uses


static int fail(pt_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
#define HIPCHK(ctx, call)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(ctx, PT_E_HIP, std::string(#call ": ") + hipGetErrorString(e_));     \
    } while (0)

// Tile shape of the work queue: 64 pixels as (8 << s) columns x (8 >> s) local rows (tuning
// key 20; automatic: ensure_tiles).  Recomputes the tile count and resets the queue order.
static int set_tiles(pt_ctx* c, int s) {
    c->tile_shift = s;
    const int tw = 8 << s, th = 8 >> s;
    c->tiles_x = (c->cfg.width + tw - 1) / tw;
    c->n_tiles = c->tiles_x * ((c->rows_local + th - 1) / th);
    (void)hipFree(c->d_tile_perm);
    (void)hipFree(c->d_tile_cost);
    c->d_tile_perm = c->d_tile_cost = nullptr;
    (void)hipFree(c->d_tile_frames);      // the adaptive buffers are per tile: allocated again on first use
    (void)hipFree(c->d_active[0]);
    (void)hipFree(c->d_active[1]);
    c->d_tile_frames = c->d_active[0] = c->d_active[1] = nullptr;
    std::vector<unsigned> ident(std::max(c->n_tiles, 1));
    for (size_t i = 0; i < ident.size(); i++) ident[i] = pack_tile(c, (unsigned)i);
    HIPCHK(c, hipMalloc(&c->d_tile_perm, ident.size() * sizeof(unsigned)));
    HIPCHK(c, hipMalloc(&c->d_tile_cost, ident.size() * sizeof(unsigned)));
    HIPCHK(c, hipMemcpy(c->d_tile_perm, ident.data(), ident.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->d_tile_cost, 0, ident.size() * sizeof(unsigned)));
    c->order_sorted = false;
    c->order_skip = 0;
    return PT_OK;
}

static void free_scene(pt_ctx* c) {
    for (float4*& d : c->d_scene) {
        (void)hipFree(d);
        d = nullptr;
    }
    c->sf.wide_ok = false;
    c->sf.n_wide = 0;
    c->sf.sweep_ok = false;
    c->scene_ok = false;
}

extern "C" {

int pt_create(const pt_config* cfg, pt_ctx** out) {
    if (!cfg || !out) return PT_E_ARG;
    *out = nullptr;
    pt_ctx* c = new pt_ctx();
    c->cfg = *cfg;
    if (c->cfg.rays_per_pixel <= 0) c->cfg.rays_per_pixel = 1;
    if (c->cfg.world <= 0) c->cfg.world = 1;
    *out = c;
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->width > 65536 || cfg->height > 65536)
        return fail(c, PT_E_ARG, "width/height out of range");
    if (cfg->display_mode < 1 || cfg->display_mode > 4) return fail(c, PT_E_ARG, "display_mode must be 1..4");
    if (cfg->max_bounce < 0) return fail(c, PT_E_ARG, "max_bounce must be >= 0");
    if (cfg->flags & ~PT_FLAG_ALL) return fail(c, PT_E_ARG, "unknown PT_FLAG bits");
    if (c->cfg.rank < 0 || c->cfg.rank >= c->cfg.world) return fail(c, PT_E_ARG, "rank out of range");
    int ndev = 0;
    HIPCHK(c, hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(c, PT_E_HIP, "no such HIP device");
    HIPCHK(c, hipSetDevice(cfg->device));
    int rank = c->cfg.rank, world = c->cfg.world;
    c->rows_local = cfg->height > rank ? (cfg->height - rank + world - 1) / world : 0;
    if ((long long)c->rows_local * cfg->width >= (1LL << 31)) return fail(c, PT_E_ARG, "framebuffer exceeds 2^31 pixels");
    size_t px = (size_t)c->rows_local * cfg->width;
    {
        int lo = 0, hi = 0;   // hi = the greatest priority (numerically least)
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(c, hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi));
    }
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_fence, hipEventDisableTiming));
    HIPCHK(c, hipMalloc(&c->accum, std::max<size_t>(px, 1) * sizeof(float4)));
    HIPCHK(c, hipMemset(c->accum, 0, std::max<size_t>(px, 1) * sizeof(float4)));
    HIPCHK(c, hipMalloc(&c->rgba8, std::max<size_t>(px, 1) * sizeof(uchar4)));
    HIPCHK(c, hipMalloc(&c->d_counters, 16 * sizeof(unsigned long long)));
    // work-queue heads (kQueueStride apart): one for the main stream and
    // one per overlap slot
    HIPCHK(c, hipMalloc(&c->d_work, kQueueSet * sizeof(unsigned) * (1 + kRingMax)));
    int n_cu = 0;
    HIPCHK(c, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device));
    c->persist_blocks = (unsigned)std::max(1, n_cu) * 8u;   // 8 x 256 threads = 32 waves per CU
    c->n_cu = std::max(1, n_cu);
    {
        size_t total_mem = 0;
        HIPCHK(c, hipDeviceTotalMem(&total_mem, cfg->device));
        c->tun.scratch_budget = std::min<size_t>(32ull << 30, total_mem / 4);
    }
    {
        int rc = set_tiles(c, 0);   // 8 x 8 until a scene picks the automatic shape (ensure_tiles)
        if (rc) return rc;
    }
    // default camera (ogl_path_trace.h:53-54)
    const float defcam[12] = {0, -6, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0};
    pt_set_camera(c, defcam);
    return PT_OK;
}

void pt_destroy(pt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    drop_graph(c);
    free_scene(c);
    (void)hipFree(c->accum); (void)hipFree(c->rgba8); (void)hipFree(c->d_counters); (void)hipFree(c->d_work);
    (void)hipFree(c->d_frame);
    (void)hipFree(c->moments);
    (void)hipFree(c->d_noise);
    if (c->h_noise) (void)hipHostFree(c->h_noise);
    (void)hipFree(c->d_tile_perm);
    (void)hipFree(c->d_tile_cost);
    (void)hipFree(c->d_tile_frames);
    (void)hipFree(c->d_active[0]);
    (void)hipFree(c->d_active[1]);
    (void)hipFree(c->d_adapt);
    if (c->h_adapt) (void)hipHostFree(c->h_adapt);
    (void)hipFree(c->dn_guide[0]); (void)hipFree(c->dn_guide[1]);
    (void)hipFree(c->dn_state[0]); (void)hipFree(c->dn_state[1]);
    (void)hipFree(c->dn_out); (void)hipFree(c->dn_rgba8);
    for (hipEvent_t e : c->dn_ev)
        if (e) (void)hipEventDestroy(e);
    (void)hipFree(c->d_rgb);
    for (int i = 0; i < kMaxSlots; i++) {
        if (c->rstream[i]) (void)hipStreamSynchronize(c->rstream[i]);
        if (c->rstream[i]) (void)hipStreamDestroy(c->rstream[i]);
    }
    for (int i = 0; i < kRingMax; i++) {
        (void)hipFree(c->slot_rgb[i]);
        if (c->ev_rdone[i]) (void)hipEventDestroy(c->ev_rdone[i]);
        if (c->ev_adone[i]) (void)hipEventDestroy(c->ev_adone[i]);
    }
    if (c->ev_fence) (void)hipEventDestroy(c->ev_fence);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (int b = 0; b < kPresentBufs; b++) {
        if (c->present_host[b]) (void)hipHostFree(c->present_host[b]);
        if (c->ev_copied[b]) (void)hipEventDestroy(c->ev_copied[b]);
    }
    for (auto& pr : c->ev_pending) { c->ev_free.push_back(pr.first); c->ev_free.push_back(pr.second); }
    for (hipEvent_t e : c->ev_free) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* pt_last_error(const pt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int pt_upload_scene(pt_ctx* c, const float* tris, int n_tris, const float* bvh, int n_nodes,
                    const float* mats, int n_mats, const float* spheres, int n_spheres) {
    if (!c) return PT_E_ARG;
    int rc = ptp::check_scene_args(tris, n_tris, bvh, n_nodes, mats, n_mats, spheres, n_spheres, c->err);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // validation and every device layout (pt_scene_pack.cpp); a rejected scene leaves the current one in place
    ptp::PackedScene packed;
    rc = ptp::pack_scene(tris, n_tris, bvh, n_nodes, mats, n_mats, spheres, n_spheres, packed, c->err);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // a render in flight may still read the old scene
    drop_graph(c);
    free_scene(c);
    for (int b = 0; b < ptp::kBufsAll; b++) {
        const size_t bytes = packed.buf[b].size() * sizeof(float);
        if (!bytes) continue;
        HIPCHK(c, hipMalloc(&c->d_scene[b], bytes));
        HIPCHK(c, hipMemcpy(c->d_scene[b], packed.buf[b].data(), bytes, hipMemcpyHostToDevice));
    }
    c->sf = packed.facts;
    c->order_sorted = false;      // the next sort pools the new scene's first short launches
    c->order_skip = 0;
    c->n_sorts = 0;
    c->scene_ok = true;
    c->guides_ok = false;         // the guides are of the old scene
    return PT_OK;
}

int pt_set_camera(pt_ctx* c, const float cam[12]) {
    if (!c || !cam) return PT_E_ARG;
    // camera basis (computeShader.c:519-522), evaluated once per dispatch on the host with
    // the same pinned binary32 ops the shader performs per invocation.
    f3 pos = mk(cam[0], cam[1], cam[2]);
    f3 fwd = pt::normalize(mk(cam[4], cam[5], cam[6]));
    f3 right = pt::normalize(pt::cross(fwd, mk(0, 0, 1)));
    f3 up = (pt::normalize(pt::cross(right, fwd)) * (float)c->cfg.height) / (float)c->cfg.width;
    float v[12] = {pos.x, pos.y, pos.z, fwd.x, fwd.y, fwd.z, right.x, right.y, right.z, up.x, up.y, up.z};
    std::memcpy(c->cam, v, sizeof(v));
    c->cam_ok = true;
    c->guides_ok = false;         // ... or of the old camera
    drop_graph(c);
    return PT_OK;
}

int pt_set_display_mode(pt_ctx* c, int mode) {
    if (!c) return PT_E_ARG;
    if (mode < 1 || mode > 4) return fail(c, PT_E_ARG, "display_mode must be 1..4");
    if (mode != c->cfg.display_mode) drop_graph(c);   // a captured graph bakes in the mode
    c->cfg.display_mode = mode;
    return PT_OK;
}

int pt_set_counting(pt_ctx* c, int enable) {
    if (!c) return PT_E_ARG;
    // graph replays never count (pt_progressive_setup refuses counting): a graph captured
    // before counting was switched on would silently produce no counts, so it is dropped
    if ((enable != 0) != c->counting) drop_graph(c);
    c->counting = enable != 0;
    return PT_OK;
}

int pt_set_kernel(pt_ctx* c, int variant) {
    if (!c) return PT_E_ARG;
    if (variant != 0 && variant != 3)
        return fail(c, PT_E_ARG, "unknown kernel variant (0 state machine, 3 state machine with the scene kept in "
                                 "global memory)");
    c->tun.variant = variant;
    drop_graph(c);
    return PT_OK;
}

// The plain integer keys of pt_set_tuning: a value `ok` accepts goes to its Tuning member,
// any other fails with `msg`.  A key may have several rows, checked in order.
struct TuningKey {
    int key;
    int ptl::Tuning::*member;       // null: a check only
    bool (*ok)(int);
    const char* msg;
    bool drops_graph;               // a captured graph bakes the value in
};
static bool in_0_1(int v) { return v == 0 || v == 1; }
static bool in_0_64(int v) { return v >= 0 && v <= 64; }
static const char kThresholdMsg[] = "threshold must be in 1..64 (0 = automatic)";
static const TuningKey kTuningKeys[] = {
    {0, &ptl::Tuning::leaf_thresh, in_0_64, kThresholdMsg, true},
    {1, &ptl::Tuning::shade_thresh, in_0_64, kThresholdMsg, true},
    {3, nullptr, in_0_64, kThresholdMsg, true},
    {3, &ptl::Tuning::minw, [](int v) { return v == 0 || (v >= 5 && v <= 8); }, "waves per SIMD must be 5..8 (0 = auto)", true},
    {4, &ptl::Tuning::pull_batch, [](int v) { return v >= 0 && v <= 1024; }, "pull batch must be 1..1024 (0 = auto)", true},
    {5, &ptl::Tuning::group_force, [](int v) { return v >= 0; }, "frames per work item must be >= 1 (0 = automatic)", true},
    {6, &ptl::Tuning::trav_floor, in_0_64, kThresholdMsg, true},
    {7, &ptl::Tuning::compact_max, [](int v) { return v >= 0 && v <= 63; }, "compaction limit must be in 0..63", true},
    {15, &ptl::Tuning::cons_off, in_0_1, "culling walk: 0 = automatic, 1 = off", true},
    {16, &ptl::Tuning::wide_off, in_0_1, "wide global walk: 0 = automatic, 1 = off", true},
    {17, &ptl::Tuning::wide_threads, [](int v) { return v == 0 || v == 256 || v == 512 || v == 768 || v == 1024; },
     "wide walk workgroup: 256, 512, 768 or 1024 threads (0 = automatic)", true},
    {18, &ptl::Tuning::overlap_bpc, [](int v) { return v >= 0 && v <= 8; },
     "overlapped render blocks per CU must be 1..8 (0 = automatic)", false},
    {19, &ptl::Tuning::cert_off, in_0_1, "leaf re-test certificate: 0 = automatic, 1 = off", true},
    {21, &ptl::Tuning::common_off, in_0_1, "specialised default-path kernel: 0 = automatic, 1 = off", true},
    {22, &ptl::Tuning::win_off, in_0_1, "window clause of the culling walk: 0 = automatic, 1 = off", true},
    {23, &ptl::Tuning::sweep_off, in_0_1, "leaf sweep: 0 = automatic, 1 = off", true},
    {24, &ptl::Tuning::pool_off, in_0_1, "path pool: 0 = automatic, 1 = off", true},
};

int pt_set_tuning(pt_ctx* c, int key, int value) {
    if (!c) return PT_E_ARG;
    const TuningKey* hit = nullptr;
    for (const TuningKey& k : kTuningKeys) {
        if (k.key != key) continue;
        if (!k.ok(value)) return fail(c, PT_E_ARG, k.msg);
        hit = &k;
    }
    if (hit) {
        c->tun.*hit->member = value;
        if (hit->drops_graph) drop_graph(c);
        return PT_OK;
    }
    if (key == 8) {
        if (value < 0) return fail(c, PT_E_ARG, "scratch budget (MiB) must be >= 0 (0 = automatic)");
        if (value == 0) {
            size_t total_mem = 0;
            HIPCHK(c, hipDeviceTotalMem(&total_mem, c->cfg.device));
            c->tun.scratch_budget = std::min<size_t>(32ull << 30, total_mem / 4);
        } else {
            c->tun.scratch_budget = (size_t)value << 20;
        }
        drop_graph(c);
        return PT_OK;
    }
    if (key == 9) {
        if (value < 0 || value > kMaxSlots)
            return fail(c, PT_E_ARG, "overlap slots must be 1..4 (1 = off, 0 = automatic)");
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->tun.overlap_slots = value ? value : kAutoSlots;
        c->slot = 0;
        c->ring = 0;
        return PT_OK;
    }
    if (key == 20) {
        if (value < 0 || value > 4) return fail(c, PT_E_ARG, "tile shape: 1..4 = 8x8, 16x4, 32x2, 64x1 (0 = automatic)");
        c->tile_key = value;
        HIPCHK(c, hipSetDevice(c->cfg.device));
        return ensure_tiles(c);
    }
    // (as ever, the threshold range is checked before the key)
    if (!in_0_64(value)) return fail(c, PT_E_ARG, kThresholdMsg);
    if (key != 2) return fail(c, PT_E_ARG, "unknown tuning key");
    // a learned order stays when the setting does not change (re-applying the default must
    // not send the next long render back through the cold probe launch)
    if ((value != 0) == c->tun.adaptive) return PT_OK;
    c->tun.adaptive = value != 0;
    c->order_sorted = false;
    c->order_skip = 0;
    if (!c->tun.adaptive && c->n_tiles > 0) {       // back to raster order
        std::vector<unsigned> ident(c->n_tiles);
        for (int i = 0; i < c->n_tiles; i++) ident[i] = pack_tile(c, (unsigned)i);
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(c->d_tile_perm, ident.data(), ident.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    }
    drop_graph(c);
    return PT_OK;
}

// The work queue's tile shape (set_tiles): tuning key 20, else 8 x 8.  16 x 4 tiles for scenes
// staged in LDS measured equal: with the builds in alternating order (ABBA, profiles/ab/
// r06n_*) 16 x 4 and 8 x 8 are within 0.1% on C2 and C5; the +0.4..0.6% of the first A/Bs
// (r06k_*, r06l_*, r06m_*) was tools/ab_inproc.py's first-position bias.  A shape change drains
// the context's streams and drops a captured graph (which holds the tile arrays).
static int ensure_tiles(pt_ctx* c) {
    const int want = c->tile_key ? c->tile_key - 1 : 0;
    if (want == c->tile_shift) return PT_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < kMaxSlots; i++)
        if (c->rstream[i]) HIPCHK(c, hipStreamSynchronize(c->rstream[i]));
    drop_graph(c);
    return set_tiles(c, want);
}

constexpr int kOrderEvery = 64;               // short launches per tile-order sort (enqueue_render)
constexpr int kOrderFirst = 8;                // ... and before the first sort after an upload
constexpr int kProbeFrames = 2, kProbeMin = 64;  // cold long renders: a sorted order after 2 frames

// The launch planner's view of the context (pt_launch_plan.h).
static ptl::Image plan_image(const pt_ctx* c) {
    return {c->cfg.width, c->rows_local, c->n_tiles, c->cfg.rays_per_pixel, c->cfg.flags, c->n_cu, c->persist_blocks,
            c->tile_shift};
}
static ptl::State plan_state(const pt_ctx* c) { return {c->counting, c->moments != nullptr, c->aces_fuse}; }
static ptl::LaunchPlan plan(const pt_ctx* c, int n_frames, bool graph) {
    return ptl::plan_launch(c->sf, c->tun, plan_image(c), plan_state(c), n_frames, graph);
}
static int launch_frames(const pt_ctx* c, int n_frames) {
    return ptl::launch_frames(c->sf, c->tun, plan_image(c), plan_state(c), n_frames);
}

// Grows the frame-split scratch to n_frames frame planes.  Earlier launches on the stream may
// still read the old buffer, so the stream is drained first; a buffer a captured graph was
// built with is handed to the graph (freed by drop_graph) instead of being freed under it.
static int ensure_rgb(pt_ctx* c, size_t need) {
    if (need <= c->rgb_bytes) return PT_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->d_rgb && c->graph_exec && c->d_rgb == c->graph_rgb) c->graph_owned.push_back(c->d_rgb);
    else (void)hipFree(c->d_rgb);
    c->d_rgb = nullptr;
    c->rgb_bytes = 0;
    HIPCHK(c, hipMalloc(&c->d_rgb, need));
    c->rgb_bytes = need;
    return PT_OK;
}

// Render stream `sl` and scratch-ring entry `e` of an overlapped launch (enqueue_render),
// created on first use.  The entry's buffer may still be read by the accumulate pass of the
// last launch that used it, on any render stream, so a reallocation first drains the main
// stream (every accumulate pass) and the render streams.
static int ensure_slot(pt_ctx* c, int sl, int e, size_t need) {
    if (!c->rstream[sl]) HIPCHK(c, hipStreamCreateWithFlags(&c->rstream[sl], hipStreamNonBlocking));
    if (!c->ev_rdone[e]) {
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_rdone[e], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_adone[e], hipEventDisableTiming));
        // the entry's queue heads start at zero; afterwards each accumulate pass re-zeroes them
        HIPCHK(c, hipMemset(c->d_work + kQueueSet * (1 + e), 0, kQueueSet * sizeof(unsigned)));
    }
    if (need <= c->slot_rgb_bytes[e]) return PT_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < kMaxSlots; i++)
        if (c->rstream[i]) HIPCHK(c, hipStreamSynchronize(c->rstream[i]));
    (void)hipFree(c->slot_rgb[e]);
    c->slot_rgb[e] = nullptr;
    c->slot_rgb_bytes[e] = 0;
    HIPCHK(c, hipMalloc(&c->slot_rgb[e], need));
    c->slot_rgb_bytes[e] = need;
    return PT_OK;
}

// The main-stream scratch a launch of n_frames needs (none in register mode), in place before it.
static int ensure_scratch(pt_ctx* c, int n_frames, bool graph) {
    return ensure_rgb(c, ptl::scratch_bytes(plan(c, n_frames, graph), plan_image(c), n_frames));
}

// k_render_sm by its template arguments: key and kernel from the same pt_render_kernels.h line.
struct RenderKernel { ptl::KernelKey key; void (*fn)(KParams); };
#define PT_X(C, L, MW, M, S, P, NT, W) {{C, L, MW, M, S, P, NT, W}, k_render_sm<C, L, MW, M, S, P, NT, W>},
static const RenderKernel kRenderKernels[] = {PT_RENDER_KERNELS(PT_X)};
#undef PT_X
// ... and the lines also built with COMMON (the launch-uniform facts as constants), by the same key
#define PT_X(C, L, MW, M, S, P, NT, W) {{C, L, MW, M, S, P, NT, W}, k_render_sm<C, L, MW, M, S, P, NT, W, true>},
static const RenderKernel kRenderKernelsCommon[] = {PT_RENDER_KERNELS_COMMON(PT_X)};
#undef PT_X
// ... and those once more with the leaf sweep as a constant too (the plan's `sweep`)
#define PT_X(C, L, MW, M, S, P, NT, W) {{C, L, MW, M, S, P, NT, W}, k_render_sm<C, L, MW, M, S, P, NT, W, true, true>},
static const RenderKernel kRenderKernelsCommonSweep[] = {PT_RENDER_KERNELS_COMMON(PT_X)};
#undef PT_X
static const RenderKernel* find_kernel(const ptl::KernelKey& key, bool common = false, bool sweep = false) {
    if (common) {
        for (const RenderKernel& k : sweep ? kRenderKernelsCommonSweep : kRenderKernelsCommon)
            if (k.key == key) return &k;
        return nullptr;
    }
    for (const RenderKernel& k : kRenderKernels)
        if (k.key == key) return &k;
    return nullptr;
}
// The facts of a COMMON line the planner cannot see (ptl::common_launch has the rest): the shaded display mode, a
// tile order and the cost counts that keep it current (a context's first launches have no learned order yet and run
// the generic line), a footprint that does not clip, an item division the kernel has by magic or not at all.
static bool common_params_ok(const pt_ctx* c, const KParams& p, int n_frames) {
    const int n_groups = (n_frames + p.group - 1) / p.group;
    return (p.mode < 2 || p.mode > 4) && p.tile_perm && p.tile_cost && c->order_sorted && p.tile_shift == 0 &&
           p.x_limit >= p.W && p.y_limit >= p.H && (p.grp_magic != 0 || n_groups == 1);
}
typedef void (*KParamsKernel)(KParams);
static KParamsKernel accum_kernel(const ptl::LaunchPlan& pl) {   // the accumulate pass of a split launch
    if (pl.accum_long) return pl.accum_moments ? k_accum_frames<kAccumPixLong, kAccumFramesLong, true>
                                               : k_accum_frames<kAccumPixLong, kAccumFramesLong>;
    return pl.accum_moments ? k_accum_frames<kAccumPix, 1, true> : k_accum_frames<kAccumPix, 1>;
}

// The image half of the kernel parameters (every kernel that takes KParams reads these).
static void fill_image(KParams& p, const pt_ctx* c) {
    p.W = c->cfg.width, p.H = c->cfg.height;
    p.row0 = c->cfg.rank, p.row_stride = c->cfg.world, p.rows_local = c->rows_local;
    p.x_limit = (c->cfg.flags & PT_FLAG_REF_DISPATCH) ? (p.W / 10) * 10 : p.W;
    p.y_limit = (c->cfg.flags & PT_FLAG_REF_DISPATCH) ? (p.H / 10) * 10 : p.H;
}

// The kernel parameters of a launch, from the context and its plan (scratch, queue head and
// the accumulate pass's outputs are the caller's).
static KParams fill_params(const pt_ctx* c, const ptl::LaunchPlan& pl, int frame_first, int n_frames, int acc_first,
                           const int* frame_dev, int frame_offset) {
    KParams p;
    std::memset(&p, 0, sizeof(p));
    // the wide walk reads the node / triangle arrays numbered by its index, and its records
    float4* const* d = c->d_scene;
    p.sc = {d[pl.wide ? ptp::kWideNodes : ptp::kNodes], d[ptp::kWalk], d[ptp::kWalkSink],
            d[pl.wide ? ptp::kWideTris : ptp::kTris], d[ptp::kMats], d[ptp::kSpheres],
            pl.wide ? d[ptp::kWideRec] : nullptr, pl.wide ? d[ptp::kWideLeafBox] : nullptr,
            c->sf.n_nodes, c->sf.n_spheres};
    if (pl.wide) std::memcpy(p.wide_cw, c->sf.wide_cw, sizeof(p.wide_cw));
    fill_image(p, c);
    p.rW = 1.0f / (float)p.W, p.fW = (float)p.W, p.fH = (float)p.H, p.rH = 1.0f / (float)p.H;
    p.accum = c->accum;
    std::memcpy(p.cam, c->cam, sizeof(p.cam));
    p.frame_first = frame_first, p.n_frames = n_frames, p.acc_first = acc_first;
    p.frame_dev = frame_dev, p.frame_offset = frame_offset;
    p.max_bounce = c->cfg.max_bounce, p.mode = c->cfg.display_mode, p.flags = c->cfg.flags, p.rpp = c->cfg.rays_per_pixel;
    p.counters = c->d_counters, p.work_counter = c->d_work;
    // scene facts
    p.n_slots = c->sf.n_slots, p.walk_np = c->sf.walk_np, p.n_mats = c->sf.n_mats, p.scene_fast = c->sf.scene_fast;
    std::memcpy(p.cons_m, c->sf.cons_m, sizeof(p.cons_m));
    std::memcpy(p.win_slack, c->sf.win_slack, sizeof(p.win_slack));
    p.win_lo = ptl::window_cull_on(c->sf, c->tun, c->cfg.flags, c->counting) ? ptc::kWindowLo : -__builtin_huge_valf();
    std::memcpy(p.root_box, c->sf.root_box, sizeof(p.root_box));
    p.root_child = c->sf.root_child;
    // the plan
    p.n_top = pl.n_top, p.wide_top = pl.wide_top, p.shade_lds = pl.shade_lds;
    p.cons_walk = pl.cons_walk, p.leaf_cert = pl.leaf_cert;
    p.sweep = pl.sweep, p.sweep_tab = d[ptp::kSweep], p.n_sweep = c->sf.sweep_ok ? c->sf.n_leaves : 0;
    {   // a camera outside the root box: its rays take the root's test before the sweep (pt_cull.h, sweep_root_hit)
        const float* rb = c->sf.root_box;
        p.sweep_root = !(c->cam[0] >= rb[0] && c->cam[0] <= rb[1] && c->cam[1] >= rb[2] && c->cam[1] <= rb[3] &&
                         c->cam[2] >= rb[4] && c->cam[2] <= rb[5]);
    }
    p.leaf_thresh = pl.leaf_thresh, p.shade_thresh = pl.shade_thresh, p.trav_floor = pl.trav_floor;
    p.compact_max = c->tun.compact_max;
    p.group = pl.group, p.pull_batch = pl.pull_batch, p.grp_magic = pl.grp_magic;
    p.tile_perm = c->d_tile_perm, p.tile_shift = c->tile_shift;
    p.queue_tiles = (unsigned)c->n_tiles;
    p.tile_cost = (c->tun.adaptive && !c->counting) ? c->d_tile_cost : nullptr;
    return p;
}

// Enqueues one render launch (work-queue reset + kernel) on the context stream.  With
// `frame_dev` the frame range is read on the device (progressive graph replay).
static int enqueue_render(pt_ctx* c, int frame_first, int n_frames, int acc_first, const int* frame_dev,
                          int frame_offset, bool force_sort = false) {
    c->stage_ok = false;    // this launch changes the image: rgba8 holds its view only if written below
    const ptl::LaunchPlan pl = plan(c, n_frames, frame_dev != nullptr);
    KParams p = fill_params(c, pl, frame_first, n_frames, acc_first, frame_dev, frame_offset);
    // Overlapped short launches (the plan's `overlap`): the render kernel runs on overlap slot
    // `sl` (own stream, colour scratch and queue counter); the accumulate pass stays on the
    // main stream, in frame order (the running mean, :548-551).  Dependencies: the slot's
    // scratch is reused only after the accumulate pass that read it (ev_adone), and a render
    // never overlaps a tile-order sort (ev_fence; the sort runs on the main stream, which has
    // waited for every earlier render).
    const size_t scratch = ptl::scratch_bytes(pl, plan_image(c), n_frames);
    const int sl = c->slot;
    const int ring = kRingMult * c->tun.overlap_slots;
    const int re = c->ring % ring;       // this launch's scratch-ring entry
    hipStream_t rs = c->stream;
    unsigned* work = c->d_work;
    if (pl.overlap) {
        int rc = ensure_slot(c, sl, re, scratch);
        if (rc) return rc;
        rs = c->rstream[sl];
        work = c->d_work + kQueueSet * (1 + re);
        p.rgb = c->slot_rgb[re];
        p.work_counter = work;
        c->slot = (sl + 1) % c->tun.overlap_slots;
        c->ring = (re + 1) % ring;
    } else if (pl.split) {
        int rc = ensure_rgb(c, scratch);
        if (rc) return rc;
        p.rgb = c->d_rgb;
    }
    if (c->rows_local == 0) return PT_OK;
    const bool common = pl.common && common_params_ok(c, p, n_frames);
    // a sweeping launch has its table: the plan's `sweep` needs sweep_ok, and a scene with sweep_ok was packed with one
    if (pl.sweep && (!p.sweep_tab || p.n_sweep < 1 || p.n_sweep > ptl::kSweepMaxLeaves || 2 * p.n_sweep != p.n_slots))
        return fail(c, PT_E_STATE, "internal: a sweeping launch without a sweep table");
    const RenderKernel* kernel = find_kernel(pl.key, common, pl.sweep);
    c->last_swept = pl.sweep;
    // the path pool: the plan's `pool` on the specialised swept line, and the bounce count its packing holds
    const bool pool = pl.pool && common && pl.sweep &&
                      ptpool::pack_ok(p.W, p.rows_local, n_frames, p.max_bounce, p.n_slots, p.sc.n_spheres);
    c->last_pooled = pool;
    if (!kernel) {
        const ptl::KernelKey& k = pl.key;
        char key[96];
        std::snprintf(key, sizeof key, "<%d,%d,%d,%d,%d,%d,%d,%d>", k.count, k.lds, k.minw, k.multi, k.split, k.padn, k.nt, k.wide);
        return fail(c, PT_E_STATE, std::string("no k_render_sm instantiation for the launch key ") + key);
    }
    if (pl.overlap) {
        if (c->adone_rec[re]) HIPCHK(c, hipStreamWaitEvent(rs, c->ev_adone[re], 0));
        if (c->fence_rec) HIPCHK(c, hipStreamWaitEvent(rs, c->ev_fence, 0));
    }
    // an overlap slot's heads were zeroed by the accumulate pass of its last render (or at
    // the slot's creation)
    if (pl.overlap) p.reset_work = work;
    else HIPCHK(c, hipMemsetAsync(work, 0, kQueueSet * sizeof(unsigned), rs));
    if (pool)
        hipLaunchKernelGGL((k_render_pool<ptl::kPoolThreads, ptl::kPoolPaths, ptl::kPoolWaves>), dim3(pl.pool_blocks),
                           dim3((unsigned)pl.pool_nt), pl.pool_lds_bytes, rs, p);
    else
        hipLaunchKernelGGL(kernel->fn, dim3(pl.blocks), dim3((unsigned)kernel->key.nt), pl.dyn_lds_bytes, rs, p);
    c->n_line_launches[common]++;
    if (pl.split) {
        if (pl.overlap) {
            HIPCHK(c, hipEventRecord(c->ev_rdone[re], rs));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_rdone[re], 0));
        }
        p.aces_out = pl.aces_out ? c->rgba8 : nullptr;
        c->stage_ok = pl.aces_out;
        p.moments = c->moments;
        hipLaunchKernelGGL(accum_kernel(pl), dim3(pl.accum_blocks), dim3(256), 0, c->stream, p);
        if (pl.overlap) {
            HIPCHK(c, hipEventRecord(c->ev_adone[re], c->stream));
            c->adone_rec[re] = true;
        }
    }
    // The queue order is recomputed from the accumulated tile costs after every long launch,
    // but only after every kOrderEvery-th short one (the first time after kOrderFirst): a
    // sort after each one-frame 1080p launch cost more than the order gained (adaptive off:
    // +0.5%), while a sorted order, even one 64 frames old, keeps most of the gain
    // (same-process A/B of one-frame launches, against sorting every launch: every 4th
    // +6%, 8th +8.4%, 16th +9.8%, 64th +10.7%).  Captured graphs (frame_dev) sort every replay.
    if (p.tile_cost && c->n_tiles > 1 &&
        (frame_dev || force_sort || n_frames > kShortLaunch ||
         ++c->order_skip >= (c->order_sorted ? kOrderEvery : kOrderFirst))) {
        c->order_skip = 0;
        c->order_sorted = true;
        c->n_sorts++;
        hipLaunchKernelGGL(k_tile_order, dim3(1), dim3(1024), 0, c->stream, c->d_tile_cost, c->d_tile_perm,
                           c->n_tiles, c->tiles_x);
        if (!frame_dev) {   // later overlapped renders start after the new order
            HIPCHK(c, hipEventRecord(c->ev_fence, c->stream));
            c->fence_rec = true;
        }
    }
    HIPCHK(c, hipGetLastError());
    return PT_OK;
}

// A pair of timing events from the recycled pool, queued for pt_sync.
static int take_events(pt_ctx* c, hipEvent_t ev[2]) {
    for (int i = 0; i < 2; i++) {
        if (c->ev_free.empty()) {
            HIPCHK(c, hipEventCreate(&ev[i]));
        } else {
            ev[i] = c->ev_free.back();
            c->ev_free.pop_back();
        }
    }
    c->ev_pending.emplace_back(ev[0], ev[1]);
    return PT_OK;
}

// Enqueues a render of n_frames as launches of at most launch_frames() frames (one launch
// when the scratch budget and the 32-bit queue ids allow).  Launch j > 0 continues the
// running mean (accumulate = 1), so the image is that of n_frames single dispatches.
static int enqueue_frames(pt_ctx* c, int frame_first, int n_frames, int acc_first, const int* frame_dev,
                          int frame_offset) {
    // A long render on a context whose tile order was never sorted (the first render after an
    // upload) would run in raster order.  Its first kProbeFrames frames go first as a short
    // launch whose tile costs are sorted at once, so the remaining frames already run most-
    // expensive-tile-first; the continuation accumulates, so the image is unchanged.
    if (!frame_dev && c->tun.adaptive && !c->counting && !c->order_sorted && n_frames >= kProbeMin) {
        // the scratch for the launch this render would have been: the next identical render
        // then finds it in place instead of freeing and mapping ~25 GB (1.5 s measured on one
        // box) in front of its kernel
        int rc = ensure_scratch(c, launch_frames(c, n_frames), false);
        if (rc) return rc;
        rc = enqueue_render(c, frame_first, kProbeFrames, acc_first, nullptr, 0, true);
        if (rc) return rc;
        frame_first += kProbeFrames;
        n_frames -= kProbeFrames;
        acc_first = 1;
    }
    const int step = launch_frames(c, n_frames);
    for (int done = 0; done < n_frames; done += step) {
        const int n = std::min(step, n_frames - done);
        int rc = enqueue_render(c, frame_first + done, n, done ? 1 : acc_first, frame_dev, frame_offset + done);
        if (rc) return rc;
    }
    return PT_OK;
}

int pt_render_async(pt_ctx* c, int frame_first, int n_frames, int acc_first) {
    if (!c) return PT_E_ARG;
    if (!c->scene_ok) return fail(c, PT_E_STATE, "pt_render before pt_upload_scene");
    if (n_frames <= 0) return fail(c, PT_E_ARG, "n_frames must be > 0");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    {
        int rc0 = ensure_tiles(c);
        if (rc0) return rc0;
    }
    if (c->counting) HIPCHK(c, hipMemsetAsync(c->d_counters, 0, 16 * sizeof(unsigned long long), c->stream));
    hipEvent_t ev[2];
    int rc = take_events(c, ev);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    // a caller that presented after its previous render gets the ACES view from this render's
    // accumulate pass (pt_present_begin then only copies it)
    c->aces_fuse = c->presented;
    c->presented = false;
    rc = enqueue_frames(c, frame_first, n_frames, acc_first, nullptr, 0);
    if (rc) return rc;
    if (c->moments) {   // the frames in the moments: they restart where the image does
        if (!acc_first) c->mom_frames = 0, c->mom_mixed = false;
        c->mom_frames += n_frames;
    }
    HIPCHK(c, hipEventRecord(ev[1], c->stream));
    c->count_pending = c->counting;
    return PT_OK;
}

static void drop_graph(pt_ctx* c) {
    if (c->graph_exec) (void)hipGraphExecDestroy(c->graph_exec);
    if (c->graph) (void)hipGraphDestroy(c->graph);
    c->graph_exec = nullptr;
    c->graph = nullptr;
    c->graph_rgb = nullptr;
    if (!c->graph_owned.empty()) {      // scratch only the dropped graph still referenced
        (void)hipSetDevice(c->cfg.device);
        (void)hipStreamSynchronize(c->stream);
        for (float* b : c->graph_owned) (void)hipFree(b);
        c->graph_owned.clear();
    }
}

int pt_progressive_setup(pt_ctx* c, int frames_per_launch, int launches_per_replay) {
    if (!c) return PT_E_ARG;
    c->stage_ok = false;
    if (!c->scene_ok) return fail(c, PT_E_STATE, "pt_progressive_setup before pt_upload_scene");
    if (frames_per_launch <= 0 || launches_per_replay <= 0) return fail(c, PT_E_ARG, "counts must be > 0");
    if (c->counting) return fail(c, PT_E_STATE, "counting is not supported in graph replay");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    drop_graph(c);
    {
        int rc0 = ensure_tiles(c);
        if (rc0) return rc0;
    }
    if (!c->d_frame) HIPCHK(c, hipMalloc(&c->d_frame, 64));
    {   // no allocation inside the capture: the scratch of the largest sub-launch first
        int rc0 = ensure_scratch(c, launch_frames(c, frames_per_launch), true);
        if (rc0) return rc0;
    }
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    const unsigned long long sorts_before = c->n_sorts;   // captured sorts run (and count) per replay
    int rc = PT_OK;
    for (int i = 0; i < launches_per_replay && rc == PT_OK; i++)
        rc = enqueue_frames(c, 0, frames_per_launch, 0, c->d_frame, i * frames_per_launch);
    if (rc == PT_OK) {
        hipLaunchKernelGGL(k_advance_frames, dim3(1), dim3(64), 0, c->stream, c->d_frame,
                           frames_per_launch * launches_per_replay);
    }
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(c->stream, &g);
    c->graph_sorts = c->n_sorts - sorts_before;
    c->n_sorts = sorts_before;
    if (rc != PT_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return fail(c, PT_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    c->graph = g;
    HIPCHK(c, hipGraphInstantiate(&c->graph_exec, g, nullptr, nullptr, 0));
    c->graph_rgb = c->d_rgb;
    c->graph_frames = frames_per_launch * launches_per_replay;
    return pt_progressive_reset(c, 1);
}

int pt_progressive_reset(pt_ctx* c, int next_frame) {
    if (!c) return PT_E_ARG;
    if (!c->d_frame) return fail(c, PT_E_STATE, "pt_progressive_setup first");
    if (next_frame < 1) return fail(c, PT_E_ARG, "frames start at 1");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpyAsync(c->d_frame, &next_frame, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // frame 1 restarts the image and the moments on the device (resolve_frames); any other
    // frame continues both
    if (next_frame == 1) c->mom_frames = 0, c->mom_mixed = false;
    return PT_OK;
}

int pt_progressive_run(pt_ctx* c, int replays) {
    if (!c) return PT_E_ARG;
    c->stage_ok = false;
    if (!c->graph_exec) return fail(c, PT_E_STATE, "pt_progressive_setup first");
    if (replays <= 0) return fail(c, PT_E_ARG, "replays must be > 0");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    hipEvent_t ev[2];
    {
        int rc = take_events(c, ev);
        if (rc) return rc;
    }
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    for (int r = 0; r < replays; r++) {
        HIPCHK(c, hipGraphLaunch(c->graph_exec, c->stream));
        c->n_sorts += c->graph_sorts;
    }
    if (c->moments) c->mom_frames += replays * c->graph_frames;
    HIPCHK(c, hipEventRecord(c->ev_fence, c->stream));   // the replays sort the tile order
    c->fence_rec = true;
    HIPCHK(c, hipEventRecord(ev[1], c->stream));
    return PT_OK;
}

int pt_sync(pt_ctx* c) {
    if (!c) return PT_E_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto& pr : c->ev_pending) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, pr.first, pr.second));
        c->last_ms = ms;
        c->total_ms += ms;
        c->n_launches++;
        c->ev_free.push_back(pr.first);
        c->ev_free.push_back(pr.second);
    }
    c->ev_pending.clear();
    if (c->count_pending) {
        HIPCHK(c, hipMemcpy(c->last_counts, c->d_counters, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        c->count_pending = false;
    }
    return PT_OK;
}

int pt_render(pt_ctx* c, int frame_first, int n_frames, int acc_first) {
    int rc = pt_render_async(c, frame_first, n_frames, acc_first);
    if (rc) return rc;
    return pt_sync(c);
}

int pt_rows(const pt_ctx* c, int* rows_local, int* row0, int* row_stride) {
    if (!c) return PT_E_ARG;
    if (rows_local) *rows_local = c->rows_local;
    if (row0) *row0 = c->cfg.rank;
    if (row_stride) *row_stride = c->cfg.world;
    return PT_OK;
}

int pt_get_config(const pt_ctx* c, pt_config* out) {
    if (!c || !out) return PT_E_ARG;
    *out = c->cfg;
    return PT_OK;
}

// Scene replication for pt_group_upload_scene (pt_group.hip, not part of the public ABI):
// gives `dst` a device scene of exactly `src`'s layout -- the same host-side facts and
// buffers of the same sizes, contents undefined -- and returns both contexts' buffer pointers
// and sizes, so the caller can fill dst's from src's (an RCCL broadcast across devices or a
// device copy).  Both contexts must have the same width (tile facts are per image).
int pt__scene_replicate_layout(pt_ctx* dst, const pt_ctx* src, void* dptr[ptp::kBufsAll], const void* sptr[ptp::kBufsAll],
                               size_t bytes[ptp::kBufsAll]) {
    if (!dst || !src || !dptr || !sptr || !bytes) return PT_E_ARG;
    if (!src->scene_ok) return fail(dst, PT_E_STATE, "source context has no scene");
    HIPCHK(dst, hipSetDevice(dst->cfg.device));
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    drop_graph(dst);
    free_scene(dst);
    for (int i = 0; i < ptp::kBufsAll; i++) {
        bytes[i] = ptp::buf_quads(src->sf, i) * sizeof(float4);
        sptr[i] = src->d_scene[i];
        if (bytes[i]) HIPCHK(dst, hipMalloc(&dst->d_scene[i], bytes[i]));
        dptr[i] = dst->d_scene[i];
    }
    dst->sf = src->sf;
    dst->order_sorted = false;
    dst->order_skip = 0;
    dst->n_sorts = 0;
    dst->guides_ok = false;
    // scene_ok stays false until the caller has filled the buffers (pt__scene_set_ready): a
    // failed broadcast or copy must not leave a context rendering from uninitialised memory
    dst->scene_ok = false;
    return PT_OK;
}

// ACES epilogue of n RGBA32F pixels on a caller's stream (pt_group's gathered frame; the
// same k_aces as pt_read_rgba8_aces and pt_present_*).  Internal, not part of the public ABI.
int pt__aces_launch(const void* src, void* dst, long long n, void* stream) {
    if (!src || !dst || n < 0) return PT_E_ARG;
    if (n == 0) return PT_OK;
    hipLaunchKernelGGL(k_aces, dim3((unsigned)((n + 256 * kAcesPix - 1) / (256 * kAcesPix))), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)src, (uchar4*)dst, n);
    return hipGetLastError() == hipSuccess ? PT_OK : PT_E_HIP;
}

int pt__scene_set_ready(pt_ctx* c, int ready) {
    if (!c) return PT_E_ARG;
    c->scene_ok = ready != 0 && c->d_scene[ptp::kMats] != nullptr;
    return PT_OK;
}

// The ray query's view of a context (pt_query_kernels.hip; internal, not part of the public ABI): the scene buffers
// and facts a cast reads, the context's flags, camera basis, size and stream.  Changes nothing in the context -- a
// query stays invisible to rendering.
int pt__query_view(const pt_ctx* c, ptq::CtxView* out) {
    if (!c || !out) return PT_E_ARG;
    const float4* const* d = c->d_scene;
    out->nodes = d[ptp::kNodes], out->tris = d[ptp::kTris], out->spheres = d[ptp::kSpheres];
    out->leaf_tris = d[ptp::kLeafTris];
    out->n_nodes = c->sf.n_nodes, out->n_spheres = c->sf.n_spheres, out->scene_fast = c->sf.scene_fast;
    out->flags = c->cfg.flags, out->kernel_variant = c->tun.variant;
    out->device = c->cfg.device, out->width = c->cfg.width, out->height = c->cfg.height;
    std::memcpy(out->cam, c->cam, sizeof(out->cam));
    out->scene_ok = c->scene_ok && d[ptp::kLeafTris] != nullptr, out->cam_ok = c->cam_ok;
    out->stream = c->stream;
    return PT_OK;
}
int pt__query_fail(pt_ctx* c, int code, const char* msg) { return fail(c, code, msg ? msg : ""); }

int pt_read_rgba32f(pt_ctx* c, float* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    size_t need = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    if (bytes < need) return fail(c, PT_E_ARG, "destination too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->accum, need, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_write_rgba32f(pt_ctx* c, const float* src, size_t bytes) {
    if (!c || !src) return PT_E_ARG;
    c->stage_ok = false;
    size_t need = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    if (bytes < need) return fail(c, PT_E_ARG, "source too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->accum, src, need, hipMemcpyHostToDevice));
    return PT_OK;
}

// The noise estimate.  Turning the moments on or off changes which accumulate
// kernel every later launch runs and whether register-mode launches exist (split_mode), so
// the context's streams are drained and a captured graph, which bakes the pointer in, is dropped.
int pt_set_moments(pt_ctx* c, int enable) {
    if (!c) return PT_E_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t px = std::max<size_t>((size_t)c->rows_local * c->cfg.width, 1);
    c->mom_frames = 0;
    c->mom_mixed = false;
    if ((enable != 0) == (c->moments != nullptr)) {
        // already so; on again: zeroed behind the passes that may still write them
        if (c->moments) HIPCHK(c, hipMemsetAsync(c->moments, 0, px * sizeof(float2), c->stream));
        return PT_OK;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < kMaxSlots; i++)
        if (c->rstream[i]) HIPCHK(c, hipStreamSynchronize(c->rstream[i]));
    drop_graph(c);
    if (!enable) {
        (void)hipFree(c->moments);
        c->moments = nullptr;
        return PT_OK;
    }
    if (!c->d_noise) HIPCHK(c, hipMalloc(&c->d_noise, sizeof(pt_noise_stats)));
    if (!c->h_noise) HIPCHK(c, hipHostMalloc((void**)&c->h_noise, sizeof(pt_noise_stats), hipHostMallocDefault));
    float2* m = nullptr;
    HIPCHK(c, hipMalloc(&m, px * sizeof(float2)));
    hipError_t e = hipMemset(m, 0, px * sizeof(float2));
    if (e != hipSuccess) {
        (void)hipFree(m);
        return fail(c, PT_E_HIP, std::string("hipMemset(moments): ") + hipGetErrorString(e));
    }
    c->moments = m;
    return PT_OK;
}

int pt_read_moments(pt_ctx* c, float* dst, size_t bytes, int* frames) {
    if (!c || !dst) return PT_E_ARG;
    if (!c->moments) return fail(c, PT_E_STATE, "moments are off (pt_set_moments)");
    const size_t need = (size_t)c->rows_local * c->cfg.width * sizeof(float2);
    if (bytes < need) return fail(c, PT_E_ARG, "destination too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->moments, need, hipMemcpyDeviceToHost));
    if (frames) *frames = c->mom_frames;
    return PT_OK;
}

// The summary on the context stream, behind the accumulate passes it depends on: the 32-byte
// block zeroed, k_noise, the block copied to pinned host memory; then one wait.
int pt_noise(pt_ctx* c, float target, pt_noise_stats* out) {
    if (!c || !out) return PT_E_ARG;
    if (!c->moments) return fail(c, PT_E_STATE, "moments are off (pt_set_moments)");
    if (c->mom_frames < 2) return fail(c, PT_E_STATE, "the noise estimate needs at least 2 frames");
    if (c->mom_mixed) return fail(c, PT_E_STATE, "per-tile frame counts after pt_render_adaptive: no single n until the image restarts");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemsetAsync(c->d_noise, 0, sizeof(pt_noise_stats), c->stream));
    const long long px = (long long)c->rows_local * c->cfg.width;
    if (px > 0) {
        KParams p;
        std::memset(&p, 0, sizeof(p));
        fill_image(p, c);
        p.moments = c->moments;
        const unsigned blocks = (unsigned)std::min<long long>((px + 255) / 256, (long long)kNoiseBlocksPerCu * c->n_cu);
        hipLaunchKernelGGL(k_noise, dim3(blocks), dim3(256), 0, c->stream, p, c->mom_frames, ptn::target_q(target),
                           c->d_noise);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(c->h_noise, c->d_noise, sizeof(pt_noise_stats), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = *c->h_noise;
    out->frames = c->mom_frames;
    return PT_OK;
}

int pt_render_until(pt_ctx* c, int frame_first, int acc_first, int batch, int max_frames, float target,
                    int* frames_done, pt_noise_stats* last) {
    if (!c || !frames_done) return PT_E_ARG;
    *frames_done = 0;
    if (batch < 2 || max_frames < batch || !(target > 0.0f))
        return fail(c, PT_E_ARG, "pt_render_until: batch >= 2, max_frames >= batch, target > 0");
    if (!c->scene_ok) return fail(c, PT_E_STATE, "pt_render_until before pt_upload_scene");
    if (acc_first && c->moments && c->mom_mixed)
        return fail(c, PT_E_STATE, "per-tile frame counts after pt_render_adaptive: pt_render_until must restart the image");
    if (!c->moments) {
        int rc = pt_set_moments(c, 1);
        if (rc) return rc;
    }
    const unsigned long long tq = ptn::target_q(target);
    pt_noise_stats s = {0, 0, 0, 0, 0};
    int done = 0;
    while (done < max_frames) {
        const int n = std::min(batch, max_frames - done);
        int rc = pt_render(c, frame_first + done, n, done ? 1 : acc_first);
        if (rc) return rc;
        done += n;
        *frames_done = done;
        rc = pt_noise(c, target, &s);
        if (rc) return rc;
        if (s.sum_q <= tq * s.pixels) break;      // mean relative error at or below the target
    }
    if (last) *last = s;
    return PT_OK;
}

// Adaptive sampling.  The buffers of the tile grid, on first use after set_tiles.
static int ensure_adaptive(pt_ctx* c) {
    const size_t bytes = (size_t)std::max(c->n_tiles, 1) * sizeof(unsigned);
    if (!c->d_adapt) HIPCHK(c, hipMalloc(&c->d_adapt, sizeof(AdaptSum)));
    if (!c->h_adapt) HIPCHK(c, hipHostMalloc((void**)&c->h_adapt, sizeof(AdaptSum), hipHostMallocDefault));
    if (!c->d_tile_frames) {
        HIPCHK(c, hipMalloc(&c->d_tile_frames, bytes));
        HIPCHK(c, hipMemsetAsync(c->d_tile_frames, 0, bytes, c->stream));
    }
    for (unsigned*& l : c->d_active)
        if (!l) HIPCHK(c, hipMalloc(&l, bytes));
    return PT_OK;
}

// One launch of an adaptive batch on the context stream: the render kernel over the `n_list` tiles of `list` (the
// generic line of the key the planner gives for that many tiles, no tile costs), then k_accum_retire over the same
// list.  n_after != 0: the batch's last launch, which decides.
static int enqueue_adaptive(pt_ctx* c, int frame_first, int n_frames, int acc_first, const unsigned* list, unsigned n_list,
                            unsigned* next, int n_after, unsigned frames_after, unsigned target_q) {
    ptl::Image im = plan_image(c);
    im.n_tiles = (int)n_list;
    ptl::State st = plan_state(c);
    st.adaptive = true;
    const ptl::LaunchPlan pl = ptl::plan_launch(c->sf, c->tun, im, st, n_frames, false);
    if (!pl.split || pl.overlap || pl.common) return fail(c, PT_E_STATE, "internal: an adaptive launch must be a plain split launch");
    KParams p = fill_params(c, pl, frame_first, n_frames, acc_first, nullptr, 0);
    int rc = ensure_rgb(c, ptl::scratch_bytes(pl, plan_image(c), n_frames));   // full-image planes (aidx)
    if (rc) return rc;
    p.rgb = c->d_rgb;
    p.tile_perm = list;
    p.queue_tiles = n_list;
    p.tile_cost = nullptr;
    p.moments = c->moments;
    if (pl.sweep && (!p.sweep_tab || p.n_sweep < 1 || p.n_sweep > ptl::kSweepMaxLeaves || 2 * p.n_sweep != p.n_slots))
        return fail(c, PT_E_STATE, "internal: a sweeping launch without a sweep table");
    const RenderKernel* kernel = find_kernel(pl.key, false, false);
    if (!kernel) return fail(c, PT_E_STATE, "no k_render_sm instantiation for the adaptive launch's key");
    c->last_swept = pl.sweep;
    c->last_pooled = false;
    HIPCHK(c, hipMemsetAsync(c->d_work, 0, kQueueSet * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(kernel->fn, dim3(pl.blocks), dim3((unsigned)kernel->key.nt), pl.dyn_lds_bytes, c->stream, p);
    c->n_line_launches[0]++;
    const unsigned per_wave = adapt_tiles_per_wave(n_list), per_block = 4u * per_wave;
    AdaptArgs a = {n_list, per_wave, c->n_tiles, n_after, frames_after, target_q, c->d_tile_frames, next, c->d_adapt};
    hipLaunchKernelGGL(k_accum_retire, dim3((n_list + per_block - 1) / per_block), dim3(256), 0, c->stream, p, a);
    HIPCHK(c, hipGetLastError());
    return PT_OK;
}

int pt_render_adaptive(pt_ctx* c, int frame_first, int acc_first, int batch, int max_frames, float target,
                       int* frames_done, pt_adaptive_stats* last) {
    if (!c || !frames_done) return PT_E_ARG;
    *frames_done = 0;
    if (batch < 2 || max_frames < batch || !(target > 0.0f))
        return fail(c, PT_E_ARG, "pt_render_adaptive: batch >= 2, max_frames >= batch, target > 0");
    if (!c->scene_ok) return fail(c, PT_E_STATE, "pt_render_adaptive before pt_upload_scene");
    if (acc_first && c->moments && c->mom_mixed)
        return fail(c, PT_E_STATE, "per-tile frame counts after pt_render_adaptive: the next adaptive call must restart the image");
    if (!c->moments) {
        int rc = pt_set_moments(c, 1);
        if (rc) return rc;
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = ensure_tiles(c);
    if (rc) return rc;
    rc = ensure_adaptive(c);
    if (rc) return rc;
    const int n0 = acc_first ? c->mom_frames : 0;
    const unsigned tq = ptn::target_q(target);
    const size_t tile_bytes = (size_t)std::max(c->n_tiles, 1) * sizeof(unsigned);
    if (c->counting) HIPCHK(c, hipMemsetAsync(c->d_counters, 0, 16 * sizeof(unsigned long long), c->stream));
    c->stage_ok = false;
    c->aces_fuse = false;       // no ACES view from these passes: pt_present_begin runs its own
    c->presented = false;
    // the first list: every tile, in the learned order (behind the sorts on this stream; overlapped renders of
    // earlier calls have been waited for by the accumulate passes on it)
    HIPCHK(c, hipMemcpyAsync(c->d_active[0], c->d_tile_perm, tile_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_tile_frames, 0, tile_bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_adapt, 0, sizeof(AdaptSum), c->stream));
    std::memset(c->h_adapt, 0, sizeof(AdaptSum));
    unsigned n_list = c->rows_local > 0 ? (unsigned)c->n_tiles : 0u;
    int done = 0, cur = 0;
    while (done < max_frames && n_list > 0) {
        const int n = std::min(batch, max_frames - done);
        // the batch's share of the summary block: the tiles that stay active, and the next list's length
        HIPCHK(c, hipMemsetAsync(&c->d_adapt->act_pixels, 0, sizeof(AdaptSum) - offsetof(AdaptSum, act_pixels), c->stream));
        // a batch too large for the scratch budget or the 32-bit queue ids runs as several launches; the last decides
        const int step = launch_frames(c, n);
        for (int off = 0; off < n; off += step) {
            const int m = std::min(step, n - off);
            const bool decides = off + m >= n;
            rc = enqueue_adaptive(c, frame_first + done + off, m, (done + off) ? 1 : acc_first, c->d_active[cur], n_list,
                                  c->d_active[cur ^ 1], decides ? n0 + done + n : 0, (unsigned)(done + n), tq);
            if (rc) return rc;
        }
        HIPCHK(c, hipMemcpyAsync(c->h_adapt, c->d_adapt, sizeof(AdaptSum), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        done += n;
        c->mom_frames = n0 + done;      // the largest count; per tile from here on
        c->mom_mixed = true;
        c->adapt_done = done;
        if (c->h_adapt->n_next > n_list) return fail(c, PT_E_STATE, "internal: the active list grew");
        n_list = c->h_adapt->n_next;
        cur ^= 1;
    }
    if (done == 0) {    // a context without rows: nothing rendered, the (empty) state restarts like the image
        if (!acc_first) c->mom_frames = 0, c->mom_mixed = false;
    }
    c->count_pending = c->counting;
    *frames_done = done;
    if (last) {
        const AdaptSum& s = *c->h_adapt;
        last->noise.pixels = s.ret_pixels + s.act_pixels;
        last->noise.sum_q = s.ret_sum_q + s.act_sum_q;
        last->noise.above = s.ret_above + s.act_above;
        last->noise.max_q = std::max(s.ret_max_q, s.act_max_q);
        last->noise.frames = n0 + done;
        last->tiles = s.ret_tiles + s.n_next;
        last->tiles_active = s.n_next;
        last->pixel_frames = s.pixel_frames;
    }
    return pt_sync(c);
}

int pt_read_tile_frames(pt_ctx* c, unsigned* dst, int max_tiles, int* n_tiles, int* tiles_x) {
    if (!c) return PT_E_ARG;
    if (dst && max_tiles < c->n_tiles) return fail(c, PT_E_ARG, "tile frame buffer too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_tiles) *n_tiles = c->n_tiles;
    if (tiles_x) *tiles_x = c->tiles_x;
    if (dst && c->n_tiles > 0) {
        if (c->d_tile_frames)
            HIPCHK(c, hipMemcpy(dst, c->d_tile_frames, (size_t)c->n_tiles * sizeof(unsigned), hipMemcpyDeviceToHost));
        else
            std::memset(dst, 0, (size_t)c->n_tiles * sizeof(unsigned));
    }
    return PT_OK;
}

// ---------------------------------------------------------------- denoised view
// One launch of a guide render on the context stream: the render kernel in display mode `mode` over the whole tile
// grid, then the plain accumulate pass into `plane` instead of the image.  Planned like an adaptive launch -- a
// frame-split launch on the generic line of its key, on the context's own stream, never counting -- and invisible to
// the context: no tile costs, no moments, no ACES view, no timing events, and none of the launch bookkeeping
// (pt_debug_launches, pt_debug_sweep, pt_debug_pool, the sort cadence) moves.
static int enqueue_guide(pt_ctx* c, const ptl::State& st, int mode, int frame_first, int n_frames, int acc_first, float4* plane) {
    const ptl::Image im = plan_image(c);
    const ptl::LaunchPlan pl = ptl::plan_launch(c->sf, c->tun, im, st, n_frames, false);
    if (!pl.split || pl.overlap || pl.common) return fail(c, PT_E_STATE, "internal: a guide launch must be a plain split launch");
    KParams p = fill_params(c, pl, frame_first, n_frames, acc_first, nullptr, 0);
    int rc = ensure_rgb(c, ptl::scratch_bytes(pl, im, n_frames));
    if (rc) return rc;
    p.rgb = c->d_rgb;
    p.accum = plane;
    p.mode = mode;
    p.tile_cost = nullptr;
    p.moments = nullptr;
    // (fill_params decides the window clause with the context's counting flag; a guide launch never counts)
    p.win_lo = ptl::window_cull_on(c->sf, c->tun, c->cfg.flags, false) ? ptc::kWindowLo : -__builtin_huge_valf();
    if (pl.sweep && (!p.sweep_tab || p.n_sweep < 1 || p.n_sweep > ptl::kSweepMaxLeaves || 2 * p.n_sweep != p.n_slots))
        return fail(c, PT_E_STATE, "internal: a sweeping launch without a sweep table");
    const RenderKernel* kernel = find_kernel(pl.key, false, false);
    if (!kernel) return fail(c, PT_E_STATE, "no k_render_sm instantiation for the guide launch's key");
    HIPCHK(c, hipMemsetAsync(c->d_work, 0, kQueueSet * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(kernel->fn, dim3(pl.blocks), dim3((unsigned)kernel->key.nt), pl.dyn_lds_bytes, c->stream, p);
    const KParamsKernel acc = pl.accum_long ? k_accum_frames<kAccumPixLong, kAccumFramesLong> : k_accum_frames<kAccumPix, 1>;
    hipLaunchKernelGGL(acc, dim3(pl.accum_blocks), dim3(256), 0, c->stream, p);
    HIPCHK(c, hipGetLastError());
    return PT_OK;
}

// The guide planes of `frames` frames: display modes 2, 3 and 4 rendered as pt_render(1, frames, 0) would, each into a
// zeroed plane (pixels outside the dispatch footprint stay zero), then packed.
static int render_guides(pt_ctx* c, int frames) {
    const size_t bytes = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    float4* raw[3] = {c->dn_state[0], c->dn_state[1], c->dn_out};
    ptl::State st = {false, true, false};   // not counting; split as with the moments on (the pass below keeps none)
    st.adaptive = true;
    for (int m = 0; m < 3; m++) {
        HIPCHK(c, hipMemsetAsync(raw[m], 0, bytes, c->stream));
        int done = 0;
        while (done < frames) {
            const int n = ptl::launch_frames(c->sf, c->tun, plan_image(c), st, frames - done);
            int rc = enqueue_guide(c, st, 2 + m, 1 + done, n, done ? 1 : 0, raw[m]);
            if (rc) return rc;
            done += n;
        }
    }
    ptd::launch_pack(c->stream, raw[0], raw[1], raw[2], c->dn_guide[0], c->dn_guide[1],
                     (long long)c->rows_local * c->cfg.width);
    HIPCHK(c, hipGetLastError());
    return PT_OK;
}

int pt_denoise_async(pt_ctx* c, const pt_denoise_params* params, pt_denoise_info* info) {
    if (!c) return PT_E_ARG;
    pt_denoise_params dp;
    pt_denoise_defaults(&dp);
    if (params) dp = *params;
    if (dp.iterations < 1 || dp.iterations > ptd::kMaxIterations) return fail(c, PT_E_ARG, "pt_denoise: iterations must be 1..8");
    if (dp.guide_frames < 1) return fail(c, PT_E_ARG, "pt_denoise: guide_frames must be >= 1");
    if (!c->scene_ok) return fail(c, PT_E_STATE, "pt_denoise before pt_upload_scene");
    if (c->cfg.world > 1)
        return fail(c, PT_E_STATE, "pt_denoise on a row-split context: its interleaved rows have no neighbours (groups are out of scope)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t px = (size_t)c->rows_local * c->cfg.width;     // world == 1: every row
    if (!c->dn_out) {
        float4** planes[5] = {&c->dn_guide[0], &c->dn_guide[1], &c->dn_state[0], &c->dn_state[1], &c->dn_out};
        for (float4** pl : planes)
            if (!*pl) HIPCHK(c, hipMalloc(pl, px * sizeof(float4)));
    }
    if (c->dn_timing)
        for (hipEvent_t& e : c->dn_ev)
            if (!e) HIPCHK(c, hipEventCreate(&e));
    int ev = 0;
    const auto mark = [&]() { if (c->dn_timing) (void)hipEventRecord(c->dn_ev[ev++], c->stream); };
    mark();
    const bool render = !c->guides_ok || c->guides_frames != dp.guide_frames;
    if (render) {
        c->guides_ok = false;
        c->dn_done = false;     // (the rendered planes pass through the result's plane)
        int rc = render_guides(c, dp.guide_frames);
        if (rc) return rc;
        c->guides_ok = true;
        c->guides_frames = dp.guide_frames;
    }
    mark();
    const bool guided = c->moments != nullptr && c->mom_frames >= 2;
    ptd::Image im;
    {
        KParams p;
        fill_image(p, c);
        im = {p.W, p.H, p.x_limit, p.y_limit};
    }
    const bool per_tile = guided && c->mom_mixed && c->d_tile_frames;
    ptd::launch_prep(c->stream, im, c->accum, guided ? c->moments : nullptr, c->mom_frames,
                     per_tile ? c->d_tile_frames : nullptr, c->mom_frames - c->adapt_done, c->tile_shift, c->tiles_x,
                     c->dn_state[0]);
    mark();
    const ptd::K k = {ptd::inv_sq(dp.sigma_lum), ptd::inv_sq(dp.sigma_normal), ptd::inv_sq(dp.sigma_albedo),
                      ptd::inv_sq(dp.sigma_depth)};
    for (int i = 0; i < dp.iterations; i++) {
        const bool last = i + 1 == dp.iterations;
        ptd::launch_iter(c->stream, im, c->dn_state[i & 1], last ? c->dn_out : c->dn_state[(i + 1) & 1], c->dn_guide[0],
                         c->dn_guide[1], last ? c->accum : nullptr, 1 << i, guided, k, c->dn_variant);
        mark();
    }
    c->dn_ev_n = ev;
    HIPCHK(c, hipGetLastError());
    c->dn_done = true;
    if (info) *info = {guided ? 1 : 0, render ? 1 : 0, dp.iterations, c->moments ? c->mom_frames : 0};
    return PT_OK;
}

int pt_denoise(pt_ctx* c, const pt_denoise_params* params, pt_denoise_info* info) {
    int rc = pt_denoise_async(c, params, info);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_read_denoised_rgba32f(pt_ctx* c, float* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    if (!c->dn_done) return fail(c, PT_E_STATE, "no denoised image (pt_denoise first)");
    const size_t need = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    if (bytes < need) return fail(c, PT_E_ARG, "destination too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->dn_out, need, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_read_denoised_rgba8_aces(pt_ctx* c, unsigned char* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    if (!c->dn_done) return fail(c, PT_E_STATE, "no denoised image (pt_denoise first)");
    const long long n = (long long)c->rows_local * c->cfg.width;
    if (bytes < (size_t)n * 4) return fail(c, PT_E_ARG, "destination too small");
    if (n == 0) return PT_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!c->dn_rgba8) HIPCHK(c, hipMalloc(&c->dn_rgba8, (size_t)n * sizeof(uchar4)));
    // a view of its own: the image's (rgba8, stage_ok) is pt_present_*'s
    hipLaunchKernelGGL(k_aces, dim3((unsigned)((n + 256 * kAcesPix - 1) / (256 * kAcesPix))), dim3(256), 0, c->stream,
                       c->dn_out, c->dn_rgba8, n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->dn_rgba8, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_read_guides(pt_ctx* c, float* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    if (!c->guides_ok) return fail(c, PT_E_STATE, "no guides (pt_denoise first)");
    const size_t n = (size_t)c->rows_local * c->cfg.width;
    if (bytes < n * 8 * sizeof(float)) return fail(c, PT_E_ARG, "destination too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<float> g(n * 4);
    for (int h = 0; h < 2; h++) {
        if (n) HIPCHK(c, hipMemcpy(g.data(), c->dn_guide[h], n * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) std::memcpy(dst + 8 * i + 4 * h, g.data() + 4 * i, 4 * sizeof(float));
    }
    return PT_OK;
}

// Measurements only (tools/denoise_measure.py; not part of the public ABI): how the iterations read their taps
// (ptd::Variant), and events around the guide render, the prep and each iteration of the denoises that follow.
int pt__denoise_debug(pt_ctx* c, int variant, int timing) {
    if (!c || variant < 0 || variant > 1) return PT_E_ARG;
    c->dn_variant = variant;
    c->dn_timing = timing != 0;
    c->dn_ev_n = 0;
    return PT_OK;
}
// ms of the last timed denoise: out[0] guide render, [1] prep, [2 ..] the iterations; returns the count (waits).
int pt__denoise_times(pt_ctx* c, float* out, int max_out) {
    if (!c || !out) return PT_E_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int n = 0;
    for (int i = 0; i + 1 < c->dn_ev_n && n < max_out; i++, n++) HIPCHK(c, hipEventElapsedTime(&out[n], c->dn_ev[i], c->dn_ev[i + 1]));
    return n;
}

int pt_read_rgba8_aces(pt_ctx* c, unsigned char* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    long long n = (long long)c->rows_local * c->cfg.width;
    if (bytes < (size_t)n * 4) return fail(c, PT_E_ARG, "destination too small");
    if (n == 0) return PT_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // the view the last render's accumulate pass wrote when the caller also read (or presented)
    // after the render before it (pt_present_begin), else the ACES pass here
    if (!c->stage_ok) {
        hipLaunchKernelGGL(k_aces, dim3((unsigned)((n + 256 * kAcesPix - 1) / (256 * kAcesPix))), dim3(256), 0,
                           c->stream, c->accum, c->rgba8, n);
        HIPCHK(c, hipGetLastError());
    }
    c->stage_ok = true;     // rgba8 is the view of the current image
    c->presented = true;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->rgba8, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

// Asynchronous presentation for a viewer that shows every frame (ogl_path_trace.h:189-192
// draws each frame's texture on the GPU that rendered it; a headless caller reads it back).
// begin: the ACES epilogue of the current image on the context stream (after every render
// issued so far and its running mean), then a copy into pinned host memory on a separate
// stream, so renders issued after it run while the image crosses PCIe.  end: waits for that
// copy and hands out the pinned pixels.
int pt_present_begin(pt_ctx* c, int buf) {
    if (!c) return PT_E_ARG;
    if (buf < 0 || buf >= kPresentBufs) return fail(c, PT_E_ARG, "present buffer must be 0..3");
    const long long n = (long long)c->rows_local * c->cfg.width;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!c->present_host[buf]) {
        HIPCHK(c, hipHostMalloc((void**)&c->present_host[buf], std::max<long long>(n, 1) * sizeof(uchar4),
                                hipHostMallocDefault));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_copied[buf], hipEventDisableTiming));
    }
    // a buffer begun again before its end: its previous copy must land first
    if (c->present_pending[buf]) HIPCHK(c, hipEventSynchronize(c->ev_copied[buf]));
    c->present_pending[buf] = false;
    // the view of the current image: written by the last render's accumulate pass when the
    // caller presented after the render before it (stage_ok), else the ACES pass here
    if (n > 0 && !c->stage_ok) {
        hipLaunchKernelGGL(k_aces, dim3((unsigned)((n + 256 * kAcesPix - 1) / (256 * kAcesPix))), dim3(256), 0,
                           c->stream, c->accum, c->rgba8, n);
        HIPCHK(c, hipGetLastError());
    }
    c->stage_ok = true;     // rgba8 is the view of the current image
    c->presented = true;
    // the copy on the context stream itself: a copy stream waiting on an event started each
    // copy about 150 us after the view was ready (one-frame loop with lag 2: 0.578 -> 0.537
    // ms per frame); the next render's accumulate pass, which rewrites the view, follows it
    if (n > 0)
        HIPCHK(c, hipMemcpyAsync(c->present_host[buf], c->rgba8, (size_t)n * sizeof(uchar4), hipMemcpyDeviceToHost,
                                 c->stream));
    HIPCHK(c, hipEventRecord(c->ev_copied[buf], c->stream));
    c->present_pending[buf] = true;
    return PT_OK;
}

int pt_present_end(pt_ctx* c, int buf, const unsigned char** pixels) {
    if (!c || !pixels) return PT_E_ARG;
    if (buf < 0 || buf >= kPresentBufs) return fail(c, PT_E_ARG, "present buffer must be 0..3");
    if (!c->present_pending[buf]) return fail(c, PT_E_STATE, "pt_present_end without pt_present_begin");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipEventSynchronize(c->ev_copied[buf]));
    c->present_pending[buf] = false;
    *pixels = c->present_host[buf];
    return PT_OK;
}

int pt_accum_device(pt_ctx* c, void** ptr, size_t* bytes) {
    if (!c) return PT_E_ARG;
    c->stage_ok = false;   // the caller may write the image through this pointer
    if (ptr) *ptr = c->accum;
    if (bytes) *bytes = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    return PT_OK;
}

int pt_copy_rows_device(pt_ctx* c, void* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    size_t need = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    if (bytes < need) return fail(c, PT_E_ARG, "destination too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpyAsync(dst, c->accum, need, hipMemcpyDeviceToDevice, c->stream));
    return pt_sync(c);
}

int pt_timing(pt_ctx* c, double* total_ms, int* n, int reset) {
    if (!c) return PT_E_ARG;
    if (total_ms) *total_ms = c->total_ms;
    if (n) *n = c->n_launches;
    if (reset) { c->total_ms = 0.0; c->n_launches = 0; }
    return PT_OK;
}

int pt_stream(pt_ctx* c, void** s) {
    if (!c || !s) return PT_E_ARG;
    c->stage_ok = false;   // ... or queue work on this stream that does
    *s = (void*)c->stream;
    return PT_OK;
}

#ifdef PT_WAVE_TRACE
extern "C" int pt_debug_wave_trace(unsigned long long* out, int max_waves, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    const int n = max_waves < kWaveTraceMax ? max_waves : kWaveTraceMax;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_trace), sizeof(unsigned long long) * 4 * n) != hipSuccess) return -1;
    if (reset) {
        std::vector<unsigned long long> z(4 * (size_t)kWaveTraceMax, 0ull);
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_wave_trace), z.data(), z.size() * 8) != hipSuccess) return -1;
    }
    return n;
}
#endif

#ifdef PT_PHASE_CLOCK
extern "C" int pt_debug_phase_clock(unsigned long long out[8], int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_clk), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_clk), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif


int pt_stats_ex(pt_ctx* c, unsigned long long out[16]) {
    if (!c || !out) return PT_E_ARG;
    std::memcpy(out, c->last_counts, sizeof(c->last_counts));
    out[13] = c->sf.lds_bytes;
    out[14] = c->sf.walk_nested ? c->sf.lds_bytes_sk : 0;
    out[15] = ptl::cons_walk_on(c->sf, c->tun, c->counting);               // the scene's LDS walk culls (slab_oct_cons)
    return PT_OK;
}

int pt_debug_window_cull(pt_ctx* c, int* active, float* slack) {
    if (!c) return PT_E_ARG;
    if (active) *active = ptl::window_cull_on(c->sf, c->tun, c->cfg.flags, c->counting) ? 1 : 0;
    if (slack) *slack = std::max(c->sf.win_slack[0], std::max(c->sf.win_slack[1], c->sf.win_slack[2]));
    return PT_OK;
}

int pt_debug_sweep(pt_ctx* c, int* swept, int* qualifies, int* n_leaves) {
    if (!c) return PT_E_ARG;
    if (swept) *swept = c->last_swept ? 1 : 0;
    if (qualifies) *qualifies = c->sf.sweep_ok ? 1 : 0;
    if (n_leaves) *n_leaves = c->sf.n_leaves;
    return PT_OK;
}

int pt_debug_pool(pt_ctx* c, int* pooled) {
    if (!c) return PT_E_ARG;
    if (pooled) *pooled = c->last_pooled ? 1 : 0;
    return PT_OK;
}

int pt_debug_launches(pt_ctx* c, unsigned long long out[2]) {
    if (!c || !out) return PT_E_ARG;
    out[0] = c->n_line_launches[0];
    out[1] = c->n_line_launches[1];
    return PT_OK;
}

int pt_debug_tile_order(pt_ctx* c, unsigned long long* sorts, unsigned* perm_out, int max_tiles, int* n_tiles,
                        int* tiles_x) {
    if (!c) return PT_E_ARG;
    if (perm_out && max_tiles < c->n_tiles) return fail(c, PT_E_ARG, "tile order buffer too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // the sorts run on the context stream, which waits for every render before them
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sorts) *sorts = c->n_sorts;
    if (n_tiles) *n_tiles = c->n_tiles;
    if (tiles_x) *tiles_x = c->tiles_x;
    if (perm_out && c->n_tiles > 0)
        HIPCHK(c, hipMemcpy(perm_out, c->d_tile_perm, (size_t)c->n_tiles * sizeof(unsigned), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_stats(pt_ctx* c, double* ms, unsigned long long out[5]) {
    if (!c) return PT_E_ARG;
    if (ms) *ms = c->last_ms;
    if (out) std::memcpy(out, c->last_counts, 5 * sizeof(unsigned long long));
    return PT_OK;
}

}  // extern "C"

