// pt_kparams.h -- a section of the pt_render.hip translation unit, not a general-purpose header:
// pt_render.hip includes it once, after the project headers and its using-declarations.
// What the kernels and the host half share: the kernel argument block (DevScene, KParams), the
// counters, the kernels' view of the scene, the queue-head stride, and the few device helpers
// that both kernel sections (pt_render_sm.h, pt_post_kernels.h) use.
namespace {

struct DevScene {
    const float4* nodes;
    // the state-machine kernel's LDS image of the same tree (pt_upload_scene): node planes
    // with WalkLinks (byte offsets, 16 * index)
    const float4* walk_lds;
    const float4* walk_sk;   // the culling walk's images: walk_lds with a ninth image of sinks
    const float4* tris;
    const float4* mats;
    const float4* spheres;
    // the 4-wide quantised tree of the global-memory walk (pt_wide.h): records (4 float4 per
    // index) and the exact leaf boxes (2 float4 per index, axis-paired like the node records)
    const float4* wrec;
    const float4* wlbox;
    int n_nodes, n_spheres;
};

struct KParams {
    DevScene sc;
    float4* accum;                 // rows_local x W
    float cam[12];                 // pos, fwd, right, up (per-dispatch constants)
    int W, H, row0, row_stride, rows_local;
    int x_limit, y_limit;          // PT_FLAG_REF_DISPATCH footprint
    int frame_first, n_frames, acc_first;
    int max_bounce, mode, flags, rpp;
    unsigned long long* counters;  // [5] when counting
    unsigned int* work_counter;    // persistent kernel pixel queue
    int n_slots, n_mats;           // triangle slots / materials (LDS staging sizes)
    int n_top;                     // global-memory scene: nodes [0, n_top) staged in LDS
    int walk_np;                   // LDS walk image: nodes per image plane (n_nodes, or kPadNodes)
    int scene_fast;                // every box coordinate inside the exact-reciprocal guard
    int leaf_thresh, shade_thresh; // wave scheduling thresholds of the state-machine kernel
    int trav_floor;                // ... and the walk floor: fewer walking lanes end a walk phase
    int compact_max;               // leaf phase: compact the edge tests of at most this many pairs (<= 63)
    int pull_batch;                // frame-split mode: queue ids a wave reserves per queue atomic (>= 32)
    unsigned* reset_work;          // k_accum_frames zeroes these queue heads (an overlap slot's) for its next use
    const int* frame_dev;          // progressive graph: device frame counter (null = use frame_first)
    int frame_offset;              // this launch's frame offset from *frame_dev
    const unsigned* tile_perm;     // queue order of the tiles, entries (ty << 16) | tx (null = raster order)
    int tile_shift;                // tiles of 64 pixels: (8 << tile_shift) columns x (8 >> tile_shift) local rows
    unsigned* tile_cost;           // per-tile segment counts of this launch (null = off)
    // frame-split work items (state-machine kernel): a queue item is (pixel, `group`
    // consecutive frames); with rgb != null the lane stores each frame's pixel colour (12 B)
    // to rgb[3 * (k * pixels + pixel)] (frame planes: the accumulate pass reads coalesced)
    // and k_accum_frames applies the running mean in frame order.
    // group = n_frames and rgb = null: the lane owns all frames and accumulates in registers.
    int group;
    float* rgb;                    // 3 floats per (frame, pixel)
    uchar4* aces_out;              // k_accum_frames: also the ACES view of the new image (or null)
    float rW, rH;                  // RN(1/W), RN(1/H) (host IEEE division) for the camera ray
    float fW, fH;                  // W, H as binary32 (kernel arguments: uniform, no VGPR)
    unsigned grp_magic;            // ceil(2^32 / n_groups) when item * n_groups < 2^32 for every item, else 0
    // root box (min.x, max.x, min.y, max.y, min.z, max.z) and its first child (-1: the root is
    // a leaf): a ray starting inside the root box hits it, so the walk may start at the child
    float root_box[6];
    int root_child;
    int shade_lds;                 // global-memory scene: materials + spheres staged in LDS too
    int cons_walk;                 // LDS scene: the culling walk (slab_oct_cons, exact leaf re-test)
    float cons_m[3];               // ... 2^-19 * the scene's largest |coordinate| per axis, rounded up
    float win_slack[3];            // ... the scene's window slack per axis (ptc::window_slack)
    float win_lo;                  // ... c_lo of the window clause: ptc::kWindowLo, or -inf (off, Moller-Trumbore)
    int wide_top;                  // wide walk (WIDE instantiations): records [0, wide_top) staged in LDS
    float wide_cw[3];              // ... 2^-18 * the scene's largest |coordinate| per axis, rounded up (WRay)
    int leaf_cert;                 // culling / wide walk: skip the exact leaf re-test where the hit certifies it
    float2* moments;               // k_accum_frames<.., true>: luminance moments (S1, S2) beside accum (pt_noise.h)
    const float4* sweep_tab;       // the leaf sweep's table (ptp::kSweep), 2 quads per leaf in chain order
    int n_sweep;                   // ... its leaves (<= ptl::kSweepMaxLeaves)
    int sweep;                     // LDS scene, 256 threads: guarded rays sweep the leaf boxes instead of walking
    int sweep_root;                // ... after the root box's own test (the camera stands outside the root box)
    // tiles in this launch's queue: the queue holds queue_tiles * n_groups * 64 ids.  The whole tile grid for every
    // launch but an adaptive one (pt_render_adaptive), whose tile_perm lists only the tiles still active
    unsigned queue_tiles;
};

struct Cnt {
    uint32_t seg, nodes, tri, sph, hits;
    // counting-build diagnostics: per phase, wave iterations (counted once per wave by the
    // first active lane) and active lanes summed over those iterations
    uint32_t tw, tl, lw, ll, sw, sl;
    uint32_t slow;   // segments outside the exact-reciprocal guard (IEEE-division walk)
    uint32_t nan;    // segments whose ray has a NaN component (can never hit)
};
constexpr int kNumCounters = 13;

// The state-machine kernel's view of the scene (pt_render_sm.h: node_at / tri_quad / wrec_at).
struct SceneView {
    const float4* nodes;
    const float4* tris;
    const float4* mats;
    const float4* spheres;
    int np, tp;    // plane strides (float4) of the state-machine kernel's LDS copy
    float cm[3];   // culling walk: 2^-19 * the scene's largest |coordinate| per axis (slab_oct_cons)
    float ws[3], clo;   // ... the scene's window slack and the window clause's c_lo (pt_cull.h)
    const float4* wrec;    // wide walk: records (global), their first `wtop` staged in LDS planes
    const float4* wlbox;   // ... exact leaf boxes
    int wtop;
    float cw[3];
};

// work-queue head stride (unsigned): each context stream / overlap slot has its own head on
// its own 128-B line
constexpr int kQueueStride = 32;

// Progressive mode (hipGraph replay): the frame range comes from a device counter, and
// accumulate = 0 only on frame 1 -- the reference's run loop after a reset
// (ogl_path_trace.h:164,199-203).
__device__ __forceinline__ void resolve_frames(KParams& p) {
    if (p.frame_dev) {
        p.frame_first = *p.frame_dev + p.frame_offset;
        p.acc_first = p.frame_first != 1;
    }
}

// Non-temporal 16-B accesses (streamed data that must not evict the scene from L2/MALL).
__device__ __forceinline__ void nt_store3(float* dst, f3 v) {
    __builtin_nontemporal_store(v.x, dst);
    __builtin_nontemporal_store(v.y, dst + 1);
    __builtin_nontemporal_store(v.z, dst + 2);
}
__device__ __forceinline__ f3 nt_load3(const float* src) {
    return mk(__builtin_nontemporal_load(src), __builtin_nontemporal_load(src + 1), __builtin_nontemporal_load(src + 2));
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

}  // namespace
