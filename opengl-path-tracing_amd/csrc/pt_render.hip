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
#include "pt_trace_launch.h"
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
// pt_launch_plan.{h,cpp}; this file fills KParams from its plan and does the stateful work: the context's life,
// scene, camera and settings, the tile grid, the render launch, the progressive graph.  The rest is its end's sections.
#include "pt_ctx.h"            // struct pt_ctx, fail / HIPCHK, the helpers more than one section calls

// Queue-order entry of linear tile t (row-major 8x8 tiles): (ty << 16) | tx, so the kernel
// decodes a tile without an integer division.
static unsigned pack_tile(const pt_ctx* c, unsigned t) {
    return ((t / (unsigned)c->tiles_x) << 16) | (t % (unsigned)c->tiles_x);
}

static void drop_graph(pt_ctx* c);   // a captured graph bakes in scene/camera/config

// The buffers sized by the tile grid (the adaptive ones are per tile too: allocated again on first use).
static void free_tiles(pt_ctx* c) {
    for (unsigned** b : {&c->d_tile_perm, &c->d_tile_cost, &c->d_tile_frames, &c->d_active[0], &c->d_active[1]}) {
        (void)hipFree(*b);
        *b = nullptr;
    }
}

// Tile shape of the work queue: 64 pixels as (8 << s) columns x (8 >> s) local rows (tuning
// key 20; automatic: ensure_tiles).  Recomputes the tile count and resets the queue order.
static int set_tiles(pt_ctx* c, int s) {
    c->tile_shift = s;
    const int tw = 8 << s, th = 8 >> s;
    c->tiles_x = (c->cfg.width + tw - 1) / tw;
    c->n_tiles = c->tiles_x * ((c->rows_local + th - 1) / th);
    free_tiles(c);
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

// The work queue's tile shape (set_tiles): tuning key 20, else 8 x 8.  16 x 4 tiles for scenes
// staged in LDS measured equal: with the builds in alternating order (ABBA, profiles/ab/
// r06n_*) 16 x 4 and 8 x 8 are within 0.1% on C2 and C5; the +0.4..0.6% of the first A/Bs
// (r06k_*, r06l_*, r06m_*) was tools/ab_inproc.py's first-position bias.  A shape change drains
// the context's streams and drops a captured graph (which holds the tile arrays).
static int ensure_tiles(pt_ctx* c) {
    const int want = c->tile_key ? c->tile_key - 1 : 0;
    if (want == c->tile_shift) return PT_OK;
    HIPCHK(c, drain_streams(c));
    drop_graph(c);
    return set_tiles(c, want);
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
    c->order_sorted = false;      // the next sort pools the new scene's first short launches
    c->order_skip = 0;
    c->n_sorts = 0;
    c->guides_ok = false;         // the guides are of the old scene
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
    int rc = pt_set_tuning(c, 8, 0);   // the automatic scratch budget
    if (rc) return rc;
    rc = set_tiles(c, 0);   // 8 x 8 until a scene picks the automatic shape (ensure_tiles)
    if (rc) return rc;
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
    free_tiles(c);
    void* const bufs[] = {c->accum, c->d_work, c->d_frame, c->d_rgb, c->moments, c->d_noise, c->d_adapt, c->dn_guide[0],
                          c->dn_guide[1], c->dn_state[0], c->dn_state[1], c->dn_out, c->dn_rgba8, c->rgba8, c->d_counters};
    for (void* b : bufs) (void)hipFree(b);
    if (c->h_noise) (void)hipHostFree(c->h_noise);
    if (c->h_adapt) (void)hipHostFree(c->h_adapt);
    for (hipEvent_t e : c->dn_ev)
        if (e) (void)hipEventDestroy(e);
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
    c->scene_ok = true;
    c->scene_serial++;
    return PT_OK;
}

int pt_set_camera(pt_ctx* c, const float cam[12]) {
    if (!c || !cam) return PT_E_ARG;
    pti::camera_basis(cam, c->cfg.width, c->cfg.height, c->cam);
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
    HIPCHK(c, drain_streams(c));
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

// The kernel parameters of a launch, from the context, the state it was planned with and its plan (scratch, queue
// head and the accumulate pass's outputs are the caller's).
static KParams fill_params(const pt_ctx* c, const ptl::LaunchPlan& pl, const ptl::State& st, int frame_first, int n_frames,
                           int acc_first, const int* frame_dev, int frame_offset) {
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
    p.win_lo = ptl::window_cull_on(c->sf, c->tun, c->cfg.flags, st.counting) ? ptc::kWindowLo : -__builtin_huge_valf();
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
    p.tile_cost = (c->tun.adaptive && !st.counting) ? c->d_tile_cost : nullptr;
    return p;
}

// One render launch on stream `rs`, the sequence every caller shares: the kernel of the plan's key (k_render_pool
// for `pool`) with the plan's grid, block and LDS bytes, behind the reset of its queue head p.work_counter (an overlap
// slot's was zeroed by its last accumulate pass).  `visible`: it shows in pt_debug_sweep, _pool and _launches.
static int launch_render(pt_ctx* c, const ptl::LaunchPlan& pl, KParams& p, hipStream_t rs, bool common, bool pool, bool visible) {
    // a sweeping launch has its table: the plan's `sweep` needs sweep_ok, and a scene with sweep_ok was packed with one
    if (pl.sweep && (!p.sweep_tab || p.n_sweep < 1 || p.n_sweep > ptl::kSweepMaxLeaves || 2 * p.n_sweep != p.n_slots))
        return fail(c, PT_E_STATE, "internal: a sweeping launch without a sweep table");
    const RenderKernel* kernel = find_kernel(pl.key, common, pl.sweep);
    if (visible) c->last_swept = pl.sweep, c->last_pooled = pool;
    if (!kernel) {
        const ptl::KernelKey& k = pl.key;
        char key[96];
        std::snprintf(key, sizeof key, "<%d,%d,%d,%d,%d,%d,%d,%d>", k.count, k.lds, k.minw, k.multi, k.split, k.padn, k.nt, k.wide);
        return fail(c, PT_E_STATE, std::string("no k_render_sm instantiation for the launch key ") + key);
    }
    if (pl.overlap) p.reset_work = p.work_counter;
    else HIPCHK(c, hipMemsetAsync(p.work_counter, 0, kQueueSet * sizeof(unsigned), rs));
    if (pool)
        hipLaunchKernelGGL((k_render_pool<ptl::kPoolThreads, ptl::kPoolPaths, ptl::kPoolWaves>), dim3(pl.pool_blocks),
                           dim3((unsigned)pl.pool_nt), pl.pool_lds_bytes, rs, p);
    else
        hipLaunchKernelGGL(kernel->fn, dim3(pl.blocks), dim3((unsigned)kernel->key.nt), pl.dyn_lds_bytes, rs, p);
    if (visible) c->n_line_launches[common]++;
    return PT_OK;
}

// The plan and parameters of a launch that must be a plain split one on the context stream (an adaptive batch over
// `im`'s tiles, a guide plane): planned with `st`, its full-image frame planes (aidx) in place as p.rgb.
static int plan_plain_split(pt_ctx* c, const ptl::Image& im, const ptl::State& st, int frame_first, int n_frames,
                            int acc_first, ptl::LaunchPlan& pl, KParams& p) {
    pl = ptl::plan_launch(c->sf, c->tun, im, st, n_frames, false);
    if (!pl.split || pl.overlap || pl.common) return fail(c, PT_E_STATE, "internal: not a plain split launch");
    p = fill_params(c, pl, st, frame_first, n_frames, acc_first, nullptr, 0);
    int rc = ensure_rgb(c, ptl::scratch_bytes(pl, plan_image(c), n_frames));
    p.rgb = c->d_rgb;
    return rc;
}

// Enqueues one render launch (work-queue reset + kernel) on the context stream.  With
// `frame_dev` the frame range is read on the device (progressive graph replay).
static int enqueue_render(pt_ctx* c, int frame_first, int n_frames, int acc_first, const int* frame_dev,
                          int frame_offset, bool force_sort = false) {
    c->stage_ok = false;    // this launch changes the image: rgba8 holds its view only if written below
    const ptl::LaunchPlan pl = plan(c, n_frames, frame_dev != nullptr);
    KParams p = fill_params(c, pl, plan_state(c), frame_first, n_frames, acc_first, frame_dev, frame_offset);
    // Overlapped short launches (the plan's `overlap`): the render kernel runs on overlap slot
    // `sl` (own stream, colour scratch and queue counter); the accumulate pass stays on the
    // main stream, in frame order (the running mean, k_accum_frames).  Dependencies: the slot's
    // scratch is reused only after the accumulate pass that read it (ev_adone), and a render
    // never overlaps a tile-order sort (ev_fence; the sort runs on the main stream, which has
    // waited for every earlier render).
    const size_t scratch = ptl::scratch_bytes(pl, plan_image(c), n_frames);
    const int sl = c->slot;
    const int ring = kRingMult * c->tun.overlap_slots;
    const int re = c->ring % ring;       // this launch's scratch-ring entry
    hipStream_t rs = c->stream;
    if (pl.overlap) {
        int rc = ensure_slot(c, sl, re, scratch);
        if (rc) return rc;
        rs = c->rstream[sl];
        p.rgb = c->slot_rgb[re];
        p.work_counter = c->d_work + kQueueSet * (1 + re);
        c->slot = (sl + 1) % c->tun.overlap_slots;
        c->ring = (re + 1) % ring;
    } else if (pl.split) {
        int rc = ensure_rgb(c, scratch);
        if (rc) return rc;
        p.rgb = c->d_rgb;
    }
    if (c->rows_local == 0) return PT_OK;
    const bool common = pl.common && common_params_ok(c, p, n_frames);
    // the path pool: the plan's `pool` on the specialised swept line, and the bounce count its packing holds
    const bool pool = pl.pool && common && pl.sweep &&
                      ptpool::pack_ok(p.W, p.rows_local, n_frames, p.max_bounce, p.n_slots, p.sc.n_spheres);
    if (pl.overlap) {
        if (c->adone_rec[re]) HIPCHK(c, hipStreamWaitEvent(rs, c->ev_adone[re], 0));
        if (c->fence_rec) HIPCHK(c, hipStreamWaitEvent(rs, c->ev_fence, 0));
    }
    const int rc = launch_render(c, pl, p, rs, common, pool, true);
    if (rc) return rc;
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
    int rc = ensure_tiles(c);
    if (rc) return rc;
    HIPCHK(c, reset_counters(c));
    hipEvent_t ev[2];
    rc = take_events(c, ev);
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
    int rc = ensure_tiles(c);
    if (rc) return rc;
    if (!c->d_frame) HIPCHK(c, hipMalloc(&c->d_frame, 64));
    // no allocation inside the capture: the scratch of the largest sub-launch first
    rc = ensure_scratch(c, launch_frames(c, frames_per_launch), true);
    if (rc) return rc;
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    const unsigned long long sorts_before = c->n_sorts;   // captured sorts run (and count) per replay
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
    const int rc = take_events(c, ev);
    if (rc) return rc;
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
    const int rc = pt_render_async(c, frame_first, n_frames, acc_first);
    return rc ? rc : pt_sync(c);
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
    launch_aces((hipStream_t)stream, (const float4*)src, (uchar4*)dst, n);
    return hipGetLastError() == hipSuccess ? PT_OK : PT_E_HIP;
}

int pt__scene_set_ready(pt_ctx* c, int ready) {
    if (!c) return PT_E_ARG;
    c->scene_ok = ready != 0 && c->d_scene[ptp::kMats] != nullptr;
    if (c->scene_ok) c->scene_serial++;       // a group's upload: the buffers were filled behind pt_upload_scene's back
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

// The traced rays' view (pt_trace_kernels.hip; internal, not part of the public ABI): the query's, with the materials
// and the two settings a path reads beside it.  Changes nothing in the context either.
int pt__trace_view(const pt_ctx* c, ptt::CtxView* out) {
    if (!c || !out) return PT_E_ARG;
    const int rc = pt__query_view(c, &out->q);
    if (rc) return rc;
    out->mats = c->d_scene[ptp::kMats];
    out->max_bounce = c->cfg.max_bounce, out->mode = c->cfg.display_mode;
    return PT_OK;
}

// The scene serial (pt_film_kernels.hip; internal, not part of the public ABI): a count that moves whenever the device
// scene is replaced, so that a film knows its guides are of another scene.  Changes nothing in the context.
int pt__scene_serial(const pt_ctx* c, unsigned long long* out) {
    if (!c || !out) return PT_E_ARG;
    *out = c->scene_serial;
    return PT_OK;
}

}  // extern "C"

// The rest of the host half, as sections of this translation unit (each opens its own extern "C"):
#include "pt_ctx_noise.h"      // the moments, pt_noise, pt_render_until, adaptive sampling
#include "pt_ctx_denoise.h"    // the guide launch, pt_denoise*, the denoised reads
#include "pt_ctx_io.h"         // reading and writing the image, the 8-bit view, pt_present_*, timing
#include "pt_ctx_debug.h"      // pt_debug_*, pt_stats, pt_stats_ex
