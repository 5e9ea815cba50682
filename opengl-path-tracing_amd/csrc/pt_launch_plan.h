// pt_launch_plan.h -- the render's launch policy: which k_render_sm instantiation a launch runs, with what grid,
// workgroup, dynamic LDS and queue parameters.  Plain C++, no HIP, no allocation: enqueue_render (pt_render.hip) does
// the stateful rest, and tests/test_launch_plan.py runs these functions on the CPU -- every rule leaves the image
// bit-exact, so a wrong one shows on the GPU only as lost speed or a fault.
#pragma once

#include <stddef.h>

namespace ptl {

// --- constants shared with the device code (pt_render.hip includes this header)
#ifndef PT_PAD_NODES
#define PT_PAD_NODES 67
#endif
// Scenes of at most kPadNodes nodes get walk images padded to kPadNodes nodes per plane, so the hi half of a node
// sits at the compile-time offset 16 * kPadNodes from its lo half (an immediate ds_read_b128 offset instead of an
// address add per walk step).  67: consecutive images start 134 16-B granules apart, 6 mod 16, spreading them over
// the LDS bank groups.
constexpr int kPadNodes = PT_PAD_NODES;
constexpr unsigned kPullBatch = 32;     // queue ids a wave reserves per queue atomic, at least

// --- host-side constants of the rules
constexpr size_t kLdsCu = 160 * 1024;         // a CU's LDS on gfx950; one workgroup may hold all of it
constexpr size_t kLdsSceneMax = 152 * 1024;   // stage the scene in LDS up to this size (lds_staged)
constexpr size_t kLdsSceneSmall = 48 * 1024;  // staged by 256-thread workgroups in every configuration
constexpr int kShortLaunch = 16;        // frames of a short launch (split_mode, overlap, the accumulate pass)
constexpr int kWideTopMax = 1 << 14;    // wide records staged in LDS: what the block's LDS share holds
constexpr int kWideThreadsAuto = 256;   // threads per block of the wide walk (tuning key 17)
// overlapped short launches: render slots (tuning key 9).  A slot's scratch is reused only after the accumulate pass
// that read it.  Measured on 1080p Cornell one-frame launches (ms per frame, round 3): 1 slot (no overlap) 0.80, 2
// slots 0.60, 3 slots 0.62, 4 slots 0.66 -- more slots put more renders in flight, whose blocks then held the CUs
// before the accumulate passes (and with them the slots) came free.  With the blocks-per-CU cap (key 18) and
// presentation on the context stream (round 4; render only / every frame shown at lag 2): 2 slots at 6 blocks per CU
// 0.516 / 0.522-0.547, 3 slots at 6 0.509 / 0.525, 3 at 5 0.505 / 0.527, 3 at 4 0.503 / 0.532, 4 at 4-5 0.615 / 0.59.
constexpr int kMaxSlots = 4, kAutoSlots = 3;
// the accumulate pass (k_accum_frames): pixels per thread of the short and the long variant
#ifndef PT_ACCUM_PIX
#define PT_ACCUM_PIX 4
#endif
constexpr int kAccumPix = PT_ACCUM_PIX, kAccumPixLong = 2;
// The leaf sweep ("The leaf sweep"): scenes of at most this many leaves test every leaf box once per segment instead
// of walking the tree.  A lane's candidate leaves are one 32-bit mask, so 32 is the ceiling.  24 by the A/B on seeded
// soups and quad rows of 5 to 32 leaves (HISTORY.md, round 12; profiles/ab/r12_leaf_sweep/cap_ab.txt): +1.5 to +4.7% at 5, 8,
// 11, 16, 21, 24 and 25 leaves against the culling walk, and from about 30 leaves the sink image costs a resident
// workgroup, so such scenes run neither.  The sweep costs 18 vector instructions per leaf and segment whatever the
// ray: it loses where the walk ends after two or three nodes (-28% on a 27-leaf soup seen across a large floor), and
// the cap bounds that loss.  PT_SWEEP_MAX_LEAVES overrides it for A/B builds.
#ifndef PT_SWEEP_MAX_LEAVES
#define PT_SWEEP_MAX_LEAVES 24
#endif
constexpr int kSweepMaxLeaves = PT_SWEEP_MAX_LEAVES;
static_assert(kSweepMaxLeaves >= 1 && kSweepMaxLeaves <= 32, "a lane's candidate set is one 32-bit mask");
// The shade threshold of a sweeping launch.  Without a walk phase the wave runs the leaf phase whenever fewer lanes
// than this wait to shade, so the threshold alone sets the lane use of both phases: swept on C2's generic line
// (256-frame launches, ms) 24: 110.1, 32: 106.8, 40: 98.2, 44: 94.7, 48: 93.3, 56: 92.8, 62: 99.9.
#ifndef PT_SWEEP_SHADE_THRESH
#define PT_SWEEP_SHADE_THRESH 56
#endif
constexpr int kSweepShadeThresh = PT_SWEEP_SHADE_THRESH;
// The path pool of the specialised swept line (pt_pool.h): paths per wave, threads per workgroup and
// the resident waves per SIMD its kernel is built for.  A pool costs 80 B of LDS per path, so the paths per wave trade
// lane use against resident waves.  Same-process A/B against the swept line of k_render_sm (7 waves per SIMD), C2's
// 1024-frame launch / the 1080p/8 share (profiles/ab/r13_path_pool/ab_table.txt; noise floor 0.3% / 0.5%), as
// paths x threads (waves per CU): 64x256 (24) -8.9% / -11.4%, 80x256 (20) +0.5 / -1.8, 96x256 (16) +1.5 / -0.3,
// 128x256 (12) -5.0 / -7.6, 128x448 (14) +2.6 / -0.5, 112x512 (16) +8.5 / +5.7, 116x512 (16) +9.4 / +6.6, 112x1024
// (16) +8.9, 120x1024 (16) +10.0 on C2 (one workgroup per CU: not measured on the share); 96x576 (18 waves in two
// nine-wave workgroups) -28%.  116 paths is the most that two 512-thread workgroups hold beside their scene copies.
// PT_POOL_* override the values for A/B builds.
#ifndef PT_POOL_PATHS
#define PT_POOL_PATHS 116
#endif
#ifndef PT_POOL_THREADS
#define PT_POOL_THREADS 512
#endif
#ifndef PT_POOL_WAVES
#define PT_POOL_WAVES 4
#endif
#ifndef PT_POOL_DEFAULT
#define PT_POOL_DEFAULT 1      // 0: builds without the pool as default (A/B)
#endif
constexpr int kPoolPaths = PT_POOL_PATHS, kPoolThreads = PT_POOL_THREADS, kPoolWaves = PT_POOL_WAVES;
constexpr bool kPoolDefault = PT_POOL_DEFAULT != 0;

// What ptp::pack_scene (pt_scene_pack.h) learns about a scene (pt_ctx holds one by value).
struct SceneFacts {
    int n_nodes = 0, n_spheres = 0, n_mats = 0, n_slots = 0, n_top = 0, walk_np = 1, scene_fast = 0;
    // the tree is a full binary tree threaded in preorder whose internal boxes contain their children's
    // (pt_bvh_culling_ok): the LDS walk may cull with slab_oct_cons (tuning key 15 = 1: off)
    bool walk_nested = false;
    bool wide_ok = false;           // the scene has a wide tree (pt_wide.h)
    int n_wide = 0;                 // wide index space (records + leaves)
    bool leaf_cert_ok = false;      // every leaf box contains its triangles' vertices (pt_wide.h certificate)
    size_t lds_bytes = 0, lds_bytes_sk = 0;   // the LDS copy without / with the culling walk's sink image
    float root_box[6] = {0, 0, 0, 0, 0, 0};
    int root_child = -1;
    float cons_m[3] = {0, 0, 0};    // KParams::cons_m
    float win_slack[3] = {0, 0, 0}; // KParams::win_slack (ptc::window_slack)
    bool win_bad = false;           // the scene is outside the window clause's conditions (pt_cull.h): no clause
    float wide_cw[3] = {0, 0, 0};
    int n_leaves = 0;               // leaf pairs (n_slots / 2)
    // the scene has a sweep table (ptp::kSweep): a nested tree inside the scene half of the exact-reciprocal guard and
    // the window clause's conditions, of at most kSweepMaxLeaves leaves whose pair indices follow the chain order
    bool sweep_ok = false;
};

// The pt_set_tuning values and the kernel variant (pt_ctx holds one by value).
struct Tuning {
    // 0 = automatic: 52/44 when the scene is staged in LDS (best on C2 since the octant walk), 20/24 when the walk
    // reads global memory (re-swept after the leaf compaction: +2% on the C3 stand-in, +3% on C4 over 16/32; leaf 20
    // re-swept in round 2: C3 +1.3%, C4 +0.6% over 16); walk floor 5 / 6 (LDS: 8 until the culling walk made a walk
    // step cheaper; re-swept with the sink walk: 5 +0.9% over 3, 2-8 within 1%) (+0.8% on C2, +0.5% on C3 over no
    // floor) -- tools/probe.py sweeps
    int leaf_thresh = 0, shade_thresh = 0, minw = 0, trav_floor = 0, compact_max = 63, pull_batch = 0;
    int group_force = 0;            // key 5: frames per work item (KParams::group), 0 = automatic
    int cons_off = 0;               // key 15: 1 = no culling walk
    int wide_off = 0;               // key 16: 1 = the binary global walk
    int wide_threads = 0;           // key 17: threads per block of the wide walk (0 = automatic)
    int overlap_bpc = 0;            // key 18: render blocks per CU of overlapped short launches (0 = automatic)
    int cert_off = 0;               // key 19: 1 = always run the exact leaf re-test
    int overlap_slots = kAutoSlots; // key 9 (1 = one stream, no overlap)
    // key 8, frame-split scratch budget: a render needing more is issued as back-to-back launches (default min(32
    // GiB, a quarter of the device memory))
    size_t scratch_budget = 0;
    int variant = 0;                // pt_set_kernel: 0, or 3 = the scene stays in global memory
    bool adaptive = true;           // key 2: adaptive tile order
    int common_off = 0;             // key 21: 1 = never the specialised default-path kernel (LaunchPlan::common)
    int win_off = 0;                // key 22: 1 = the culling walk without its window clause (pt_cull.h)
    int sweep_off = 0;              // key 23: 1 = no leaf sweep (the culling walk instead)
    int pool_off = 0;               // key 24: 1 = no path pool (k_render_sm's swept line instead)
};

// the context's share of the image and its device; what else a launch depends on
struct Image {
    int width, rows_local, n_tiles, rpp, flags, n_cu;
    unsigned persist_blocks;
    int tile_shift = 0;             // work-queue tiles of (8 << tile_shift) x (8 >> tile_shift) pixels (tuning key 20)
};
struct State {
    bool counting, moments, aces_fuse;
    // a launch of pt_render_adaptive: Image::n_tiles is its list of active tiles, not the grid.  A synchronous batch on
    // the context's stream (no overlap slot) on the generic line of its key (the COMMON build writes tile costs
    // unconditionally, and these launches record none)
    bool adaptive = false;
};

// A k_render_sm instantiation by its template arguments (pt_render_kernels.h lists them).
struct KernelKey { bool count, lds; int minw; bool multi, split, padn; int nt; bool wide; };
inline bool operator==(const KernelKey& a, const KernelKey& b) {
    return a.count == b.count && a.lds == b.lds && a.minw == b.minw && a.multi == b.multi && a.split == b.split &&
           a.padn == b.padn && a.nt == b.nt && a.wide == b.wide;
}

struct LaunchPlan {
    bool lds, wide, cons_walk, leaf_cert, split, overlap, shade_lds;
    int nt, mw, group, pull_batch, leaf_thresh, shade_thresh, trav_floor, n_top, wide_top;
    unsigned grp_magic, blocks;
    size_t dyn_lds_bytes;
    bool accum_long, accum_moments, aces_out;   // the accumulate pass of a split launch ...
    unsigned accum_blocks;                      // ... and its grid (256 threads per block)
    KernelKey key;
    // The launch may run the key's line of PT_RENDER_KERNELS_COMMON (pt_render_kernels.h): the instantiation that
    // holds the default configuration's launch-uniform facts as constants (common_launch).  Beside the key, not in
    // it: the launch still has its generic line, which enqueue_render takes when a fact only it can see fails.
    bool common;
    // Guarded rays sweep the scene's leaf boxes instead of walking (pt_cull.h, sweep_mask).  The COMMON line is built
    // with it on and with it off; a generic LDS line reads it as a kernel argument.
    bool sweep;
    // The launch may run k_render_pool (pt_render_pool.h) instead of the COMMON swept line: path state in a
    // wave-private LDS pool of pool_paths paths, pool_nt threads per workgroup, pool_blocks workgroups of
    // pool_lds_bytes dynamic LDS each.  Beside the generic fields, which keep their values: enqueue_render takes the
    // line they describe when a fact only it can see fails (common_params_ok, the bounce limit of the packing).
    bool pool;
    int pool_paths, pool_nt;
    unsigned pool_blocks;
    size_t pool_lds_bytes;
};

// The template arguments of the one line built with COMMON (the default path of a Cornell-sized scene).
constexpr KernelKey kCommonKey = {false, true, 7, false, true, true, 256, false};

// Whether the LDS walk culls (also pt_stats_ex[15]), and the bound on a launch's queue ids.
bool cons_walk_on(const SceneFacts& f, const Tuning& t, bool counting);
bool window_cull_on(const SceneFacts& f, const Tuning& t, int flags, bool counting);
bool sweep_on(const SceneFacts& f, const Tuning& t, bool counting);
unsigned long long id_limit(const Tuning& t, const Image& im);

// Everything a launch of n_frames decides before it touches HIP.  `graph`: the launch is captured
// (pt_progressive_setup), its frame range read on the device.
LaunchPlan plan_launch(const SceneFacts& f, const Tuning& t, const Image& im, const State& s, int n_frames,
                       bool graph);

// Frames of one launch for a render of n_frames (1..n_frames): a longer render is issued as back-to-back launches of
// at most this many frames.
int launch_frames(const SceneFacts& f, const Tuning& t, const Image& im, const State& s, int n_frames);

// Colour scratch of a launch: 12 B per pixel-frame in frame-split mode, none in register mode.
size_t scratch_bytes(const LaunchPlan& plan, const Image& im, int n_frames);

}  // namespace ptl
