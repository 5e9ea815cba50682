// pt_ctx.h -- a section of the pt_render.hip translation unit, not a general-purpose header: pt_render.hip includes
// it once, after the device sections.  The context every host section works on: the ring and slot constants,
// struct pt_ctx with its fields grouped by the section that owns them, fail / HIPCHK, and the few helpers more than
// one host section calls.
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
    // ---- configuration, scene and camera (pt_render.hip)
    pt_config cfg{};
    int rows_local = 0;
    int n_cu = 0;
    float4* d_scene[ptp::kBufsAll] = {};   // the device scene (ptp::SceneBuf); null: the scene has no such buffer
    ptl::SceneFacts sf;             // what ptp::pack_scene learned (the launch planner's input)
    ptl::Tuning tun;                // pt_set_tuning values and the kernel variant
    bool scene_ok = false, cam_ok = false, counting = false;
    unsigned long long scene_serial = 0;   // moves whenever the device scene is replaced (pt__scene_serial: a film's guides)
    float cam[12] = {0};
    std::string err;
    // ---- the image and its launches (pt_render.hip)
    hipStream_t stream = nullptr;
    float4* accum = nullptr;
    unsigned int* d_work = nullptr;
    unsigned persist_blocks = 2048;
    float* d_rgb = nullptr;        // per-(frame, pixel) colours of the frame-split mode
    size_t rgb_bytes = 0;
    // adaptive queue order ("longest first"): per-tile segment counts measured by the
    // previous renders order the next render's 8x8 tiles so cheap tiles form the tail
    unsigned* d_tile_cost = nullptr;
    unsigned* d_tile_perm = nullptr;
    int n_tiles = 0, tiles_x = 1;
    int tile_shift = 0, tile_key = 0;   // tile shape (KParams::tile_shift) and tuning key 20 (0 = automatic)
    int order_skip = 0;             // short launches since the last tile-order sort
    bool order_sorted = false;      // a sort ran since the scene upload
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
    int* d_frame = nullptr;                      // progressive graph frame counter
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int graph_frames = 0;
    // a captured graph bakes in the scratch pointer it was captured with: that buffer stays
    // alive (owned here once ensure_rgb has moved on to a larger one) until drop_graph
    float* graph_rgb = nullptr;
    std::vector<float*> graph_owned;
    // ---- noise estimate and adaptive sampling (pt_ctx_noise.h).  pt_set_moments: the luminance moments beside
    // accum, the frames folded into them since the image last restarted (host count), and the summary's device
    // block and pinned host copy (k_noise)
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
    // ---- denoised view (pt_ctx_denoise.h; pt_denoise): the two guide planes (N.rgb, Z) and (A.rgb, 0)
    // with the guide_frames they hold, the filter's ping-pong state planes, its result and the result's ACES view.  The
    // three rendered guide images pass through dn_state[0], dn_state[1] and dn_out on their way into the guide planes.
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
    // ---- reading, the 8-bit view, presentation and timing (pt_ctx_io.h)
    uchar4* rgba8 = nullptr;
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
    std::vector<hipEvent_t> ev_free;                               // recycled events
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending;     // launches not yet synced
    double total_ms = 0.0;
    int n_launches = 0;
    float last_ms = 0.0f;
    // ---- counters and debug readers (pt_ctx_debug.h)
    unsigned long long* d_counters = nullptr;
    unsigned long long last_counts[16] = {0};
    bool count_pending = false;
    unsigned long long n_line_launches[2] = {0, 0};   // render launches enqueued on a generic / a COMMON line (pt_debug_launches)
    bool last_swept = false;        // the last render launch enqueued ran the leaf sweep (pt_debug_sweep)
    bool last_pooled = false;       // ... ran k_render_pool (pt_debug_pool)
    // k_tile_order launches since the scene upload (pt_debug_tile_order): enqueued directly, and
    // per replay of the captured graph
    unsigned long long n_sorts = 0, graph_sorts = 0;
};

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

// Drains the context stream and every render slot's stream (before a buffer one of them may still read is replaced).
static hipError_t drain_streams(pt_ctx* c) {
    hipError_t e = hipStreamSynchronize(c->stream);
    for (int i = 0; i < kMaxSlots && e == hipSuccess; i++)
        if (c->rstream[i]) e = hipStreamSynchronize(c->rstream[i]);
    return e;
}
// The counters of a counting context, zeroed on the context stream in front of a render that counts.
static hipError_t reset_counters(pt_ctx* c) {
    return c->counting ? hipMemsetAsync(c->d_counters, 0, 16 * sizeof(unsigned long long), c->stream) : hipSuccess;
}

// The ACES epilogue (k_aces) of n RGBA32F pixels on `stream`.
static void launch_aces(hipStream_t stream, const float4* src, uchar4* dst, long long n) {
    hipLaunchKernelGGL(k_aces, dim3((unsigned)((n + 256 * kAcesPix - 1) / (256 * kAcesPix))), dim3(256), 0, stream, src, dst, n);
}
