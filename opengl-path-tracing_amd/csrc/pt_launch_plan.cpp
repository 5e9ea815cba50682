// pt_launch_plan.cpp -- the render's launch rules (pt_launch_plan.h), each with the measurement that set it.  No rule
// changes an image; tests/test_launch_plan.py pins their results (tests/golden/launch_plans.txt) and checks the
// invariants the kernel relies on.
#include "pt_launch_plan.h"

#include "pt_pool.h"

#include "../../include/pt_api.h"

#include <algorithm>
#include <cmath>

namespace ptl {

// Resident waves per SIMD of the render kernel: tuning key 3, else 7 for LDS scenes (72 VGPRs, a few spilled: +0.8%
// on C2 over 6, which was +5% over 5; 8 spills 20+ and loses 7%), 6 for global-memory scenes (7 leaves fewer top
// nodes per block in LDS: -6% on the C3 stand-in).
static int resident_waves(int minw, bool lds) { return minw ? minw : (lds ? 7 : 6); }

// Whether the state-machine kernel stages the scene in LDS: up to kLdsSceneSmall always; up to kLdsSceneMax when wide
// workgroups share the copy (lds_threads' configuration: not counting, automatic occupancy, one ray per pixel).
// Variant 3 forces the global-memory walk.
static bool lds_staged(const SceneFacts& f, const Tuning& t, const Image& im, const State& s) {
    if (t.variant == 3) return false;
    if (f.lds_bytes <= kLdsSceneSmall) return true;
    return !s.counting && !t.minw && im.rpp == 1 && f.lds_bytes <= kLdsSceneMax;
}

// Whether the state-machine kernel's LDS walk culls: the tree qualifies (walk_nested), key 15 leaves
// it on, nothing is counted, and the sink image (32 B per node beside the 16 N octant records) costs no resident
// block -- a scene whose copy just fits mw blocks per CU in 160 KiB would otherwise lose a block per CU, far more
// than the walk gains (+7%).  The occupancy compared is the LDS one, whether or not the launch stages.
bool cons_walk_on(const SceneFacts& f, const Tuning& t, bool counting) {
    if (!f.walk_nested || t.cons_off || counting) return false;
    const size_t mw = (size_t)resident_waves(t.minw, true);
    const auto blocks = [mw](size_t b) { return b ? std::min(mw, kLdsCu / b) : mw; };
    return blocks(f.lds_bytes_sk) >= blocks(f.lds_bytes);
}

// Whether the culling walk runs with the window clause (pt_cull.h; also pt_debug_window_cull): the walk culls, key 22
// leaves the clause on, the scene is inside the conditions of the clause's lemma, and triangles are accepted by
// hit_triangle, whose window the lemma is about.
bool window_cull_on(const SceneFacts& f, const Tuning& t, int flags, bool counting) {
    return cons_walk_on(f, t, counting) && !t.win_off && !f.win_bad && !(flags & PT_FLAG_MOLLER_TRUMBORE);
}

// Whether the guarded rays of an LDS launch sweep the leaf boxes instead of walking ("The leaf sweep"): the launch
// would run the culling walk, the scene has a sweep table, and key 23 leaves it on.
bool sweep_on(const SceneFacts& f, const Tuning& t, bool counting) {
    return cons_walk_on(f, t, counting) && f.sweep_ok && !t.sweep_off;
}

// Whether a global-memory launch walks the wide tree: the scene has one (a nested tree), it lies
// inside the scene half of the exact-reciprocal guard (otherwise no lane could use it), tuning key 16 leaves it on,
// nothing is counted (counting builds keep the binary walk: their counts are the reference's), and the occupancy is
// one the wide instantiations cover (5-7 waves per SIMD; automatic 6).
static bool wide_walk_on(const SceneFacts& f, const Tuning& t, bool counting) {
    return f.wide_ok && f.scene_fast && !t.wide_off && !counting && t.minw != 8;
}

// Threads per workgroup of the state-machine kernel on an LDS-staged scene of `lds` bytes: the k = 1..4 waves per
// SIMD per workgroup that make the most resident waves, min(floor(160 KiB / lds), floor(7 / k)) * k (7 waves per SIMD
// is the kernel's register budget), the narrowest on a tie: 256 threads down to a 23 KiB copy, then 512 / 768 / 1024
// (6, 6, 4 waves per SIMD at 32 / 54 / 160 KiB).  The wide instantiations are the default configuration's
// (non-counting, one ray per pixel, automatic occupancy); other launches keep 256 threads.
static int lds_threads(const Tuning& t, const Image& im, const State& s, size_t lds) {
    if (s.counting || t.minw || im.rpp > 1 || !lds) return 256;
    const int per_cu = (int)(kLdsCu / lds);     // copies resident per CU
    int best_k = 1, best = 0;
    for (int k = 1; k <= 4; k++) {      // k waves per SIMD per workgroup, at most 7 per SIMD
        const int waves = std::min(per_cu, 7 / k) * k;
        if (waves > best) { best = waves; best_k = k; }
    }
    return 256 * best_k;
}

// Frames per work item of the state-machine kernel (KParams::group).  Items of a few frames keep every resident lane
// busy to the end of a launch and let the per-GPU share of a multi-GPU split (fewer pixels than lanes at 1080p/8) use
// the whole chip; the per-frame colours go to a buffer and k_accum_frames applies the running mean in frame order.
// Measured (C2 scene, 64-frame launches): 8 frames per item +6% over whole-pixel items on one GPU, 2-4 frames +85% on
// a 1080p/8 share.  group == n_frames is the register mode (a lane owns all frames of a pixel and accumulates in
// registers).  The counting build follows the same plan: with whole-pixel items a 1080p/8 share of a 1024-frame
// launch would run each lane through 1024 frames in sequence (minutes). Round 6: the frames per item follow the
// frames each resident lane renders in the launch, F = pixels * frames / resident lanes.  An item costs a fixed pull
// and set-up o plus g frames of c each, and a launch ends in a tail of about half an item, so the time per lane is
// about F c + (F / g) o + g c / 2: least at g = sqrt(2 F o / c).  Fitted to same-process A/Bs of C2's 1024-frame
// launch (profiles/ab/r06f_*): a 1080p/8 share (F = 578) is fastest at 9-12 frames per item (+1.4% over 16), a
// 1080p/4 share (F = 1157) at 12, the whole image (F = 4628) at 16 or more; global-memory scenes cost about 5x more
// per frame (c), so about sqrt(5) fewer. The caps: C2 16 +0.5% over 8; C3 stand-in 4 +8% over 8.
static int plan_group(const SceneFacts& f, const Tuning& t, const Image& im, const State& s, int n_frames) {
    if (t.group_force > 0) return std::min(t.group_force, n_frames);
    const bool lds_scene = lds_staged(f, t, im, s);
    const double lanes = (double)im.n_cu * 4.0 * resident_waves(t.minw, lds_scene) * 64.0;
    // (an adaptive launch renders the pixels of its active tiles only: few tiles make short items, so that the
    // shortened queue still has an item for every resident wave)
    const double px = s.adaptive ? (double)im.n_tiles * 64.0 : (double)im.rows_local * im.width;
    const double F = px * n_frames / lanes;
    int g = (int)(std::sqrt(F) * (lds_scene ? 0.416 : 0.19) + 0.5);
    g = std::max(1, std::min(g, lds_scene ? 16 : 4));
    return std::min(g, n_frames);
}

// Whether a launch of n_frames with frames-per-item `group` runs in frame-split mode (colour planes +
// k_accum_frames).  Register mode (group == n_frames: a lane owns whole pixels, the running mean in registers) pulls
// one queue id per lane without batching, which is right for long items.  But a launch of a few frames has items of a
// few segments, and the chip-wide queue counter then throttles the kernel: one 1080p frame per launch (the
// reference's one dispatch per displayed frame) took 3.2 ms of kernel time, against 0.5 ms per frame in long
// launches.  In automatic mode such launches use the split path and its batched reservations; pt_set_tuning key 5 >=
// n_frames still forces register mode.
static bool split_mode(const Tuning& t, const State& s, int n_frames, int group) {
    // the moments of the noise estimate are kept by the accumulate pass: with them on every launch is split, also
    // whole-pixel items (tuning key 5 >= n_frames)
    if (s.moments) return true;
    if (group < n_frames) return true;
    return t.group_force == 0 && n_frames <= kShortLaunch;
}

// Queue ids are 32-bit: a launch's items * 64 plus what the resident waves can reserve past the end stay below 2^32.
// A wave reserves max(pull_batch, 64) ids per queue atomic and, once the queue has run dry, at most two more
// reservations (the one that crossed the end and one more; its lanes then finish), so the overshoot is at most
// (resident waves) * 2 * max(pull_batch, 64), with at most persist_blocks * 4 resident waves (256-thread blocks) and
// pull_batch at most 1024 (tuning key 4) or 256 (automatic).
unsigned long long id_limit(const Tuning& t, const Image& im) {
    const unsigned long long pb = (unsigned long long)std::max(256, t.pull_batch);
    const unsigned long long slack = (unsigned long long)im.persist_blocks * 4ull * 2ull * pb;
    return (1ull << 32) - slack - (1ull << 20);
}

// The largest frame count whose frame-split scratch (12 B per pixel-frame) fits the budget and whose queue ids stay
// 32-bit.  Only the first of a render's launches uses the caller's accumulate flag, so the result is that of n_frames
// dispatches (pt_api.h).
int launch_frames(const SceneFacts& f, const Tuning& t, const Image& im, const State& s, int n_frames) {
    const unsigned long long px = (unsigned long long)std::max(im.rows_local, 1) * (unsigned long long)im.width;
    const unsigned long long tiles64 = (unsigned long long)std::max(im.n_tiles, 1) * 64ull;
    const unsigned long long lim = id_limit(t, im);
    int n = n_frames;
    for (;;) {
        const int g = plan_group(f, t, im, s, n);
        if (!split_mode(t, s, n, g)) return n;    // register mode: no scratch, one group
        // one frame per launch always runs, even when its scratch exceeds the budget (so n strictly decreases to at
        // most 1: the loop ends)
        const unsigned long long by_budget = std::max(1ull, (unsigned long long)t.scratch_budget / (px * 12ull));
        const unsigned long long ng = (unsigned long long)((n + g - 1) / g);
        const unsigned long long by_ids = (lim / tiles64) * (unsigned long long)g;
        if (((unsigned long long)n <= by_budget && ng * tiles64 < lim) || n == 1) return n;
        const unsigned long long m = std::min<unsigned long long>({(unsigned long long)n - 1, by_budget, by_ids});
        n = (int)std::max<unsigned long long>(m, 1ull);
    }
}

// The instantiation a launch runs: the template arguments of a pt_render_kernels.h line.
static KernelKey kernel_key(bool counting, bool lds, bool wide, bool split, int mw, int rpp, int nt, int walk_np) {
    const bool multi = rpp > 1;
    if (wide) {     // global-memory wide walk (never counting, never LDS)
        if (multi) return {false, false, 6, true, split, false, 256, true};   // raysPerPixel > 1: built for 6 waves, 256 threads
        if (nt == 512 || nt == 768) return {false, false, 6, false, split, false, nt, true};
        if (nt == 1024) return {false, false, 4, false, split, false, 1024, true};
        return {false, false, mw == 5 || mw == 7 ? mw : 6, false, split, false, 256, true};
    }
    // an LDS copy shared by a wide workgroup (lds_threads): the register budget of the waves that are resident (6, 6,
    // 4 per SIMD), not of 7
    if (nt == 512 || nt == 768) return {false, true, 6, false, split, false, nt, false};
    if (nt > 256) return {false, true, 4, false, split, false, 1024, false};
    if (counting) return {true, lds, 5, multi, split, false, 256, false};     // counting builds: 5 waves, binary walks
    // split launches of one ray per pixel have builds for 8 and 7 waves per SIMD ...
    if (split && mw == 8 && !multi) return {false, lds, 8, false, true, false, 256, false};
    // ... the 7-wave LDS one with the padded node count as a compile-time offset
    if (split && mw == 7 && !multi) return {false, lds, 7, false, true, lds && walk_np == kPadNodes, 256, false};
    // every other launch (register mode and raysPerPixel > 1 at 7 or 8 included) runs the 6- or 5-wave build
    return {false, lds, mw >= 6 ? 6 : 5, multi, split, false, 256, false};
}

// Whether a launch may run the COMMON instantiation of its key: every fact that kernel holds as a
// constant is true of this launch.  The key says the rest: not counting, the scene staged in LDS with images padded
// to kPadNodes, one ray per pixel, frame-split, 7 waves per SIMD, 256 threads.  What the planner cannot see -- the
// display mode, a learned tile order, a footprint that clips -- enqueue_render checks.
static bool common_launch(const SceneFacts& f, const Tuning& t, const Image& im, const LaunchPlan& p) {
    if (t.common_off || t.win_off || f.win_bad || !(p.key == kCommonKey)) return false;   // (the window clause's c_lo is a constant there)
    // no tuning key in the way: automatic occupancy, 8 x 8 tiles, the culling walk.  The thresholds and the walk
    // floor stay kernel arguments (as constants 52 / 44 / 5 they measured 1.1% slower on C2: the sink walk's yield
    // test then takes 6 more vector instructions), but a launch that overrides one keeps the generic line, so a
    // threshold sweep compares one kernel with itself.
    if (t.minw || t.leaf_thresh || t.shade_thresh || t.trav_floor || im.tile_shift != 0 || !p.cons_walk) return false;
    if (im.flags != 0) return false;
    return f.n_spheres == 1 && f.scene_fast != 0 && f.walk_nested && f.root_child >= 0;
}

LaunchPlan plan_launch(const SceneFacts& f, const Tuning& t, const Image& im, const State& s, int n_frames,
                       bool graph) {
    LaunchPlan p{};
    const bool lds_scene = lds_staged(f, t, im, s);
    p.lds = t.variant == 0 && lds_scene;
    // the global-memory walk of a nested tree takes the wide tree (pt_wide.h)
    p.wide = !p.lds && wide_walk_on(f, t, s.counting);
    p.cons_walk = cons_walk_on(f, t, s.counting);     // set for global scenes too (the kernel reads it when LDS)
    // the certificate stands on hit_triangle's plane distance: not in Moller-Trumbore mode. The wide walk only: on
    // the LDS culling walk (C2, VALU-bound, the box re-read from LDS) its ~40 VALU per leaf phase cost more than the
    // re-test (-1.9%, same-process A/B r05c)
    p.leaf_cert = f.leaf_cert_ok && !t.cert_off && !(im.flags & PT_FLAG_MOLLER_TRUMBORE) && p.wide;
    p.leaf_thresh = t.leaf_thresh ? t.leaf_thresh : (lds_scene ? 52 : 20);
    // (a sweeping launch has its own, kSweepShadeThresh: set below, once the workgroup is known)
    p.shade_thresh = t.shade_thresh ? t.shade_thresh : (lds_scene ? 44 : 24);
    // walk floor: 5 for the small LDS scenes (C2), 8 for the wide-workgroup ones (keysweep on the 150 / 380-triangle
    // stand-ins: +0.8% / +1.2% over 5), 6 for global memory
    p.trav_floor = t.trav_floor ? t.trav_floor : (lds_scene ? (f.lds_bytes > kLdsSceneSmall ? 8 : 5) : 6);
    p.group = plan_group(f, t, im, s, n_frames);
    p.split = split_mode(t, s, n_frames, p.group);
    const unsigned long long n_groups = (unsigned long long)((n_frames + p.group - 1) / p.group);
    // queue ids reserved per queue atomic: on an LDS-staged scene an item of one or two frames is a few short
    // segments, and the chip-wide counter then limits the launch (one 1080p Cornell frame per launch: 1.14 ms kernel
    // time with 32 ids per reservation, 0.97 with 128; 4K 3.44 -> 2.64 ms; 4-frame launches 0.83 -> 0.62 ms per
    // frame).  A wave that reserves more ids than it soon needs lengthens the launch tail instead, so longer items
    // and the global-memory scenes' long segments keep 32 (C3 stand-in, one frame per launch: 3.19 ms with 32, 3.63
    // with 128).  With overlapped one-frame launches (2 slots) 256 ids beat 128 (0.594 vs 0.603 ms per 1080p frame;
    // 64: 0.689).  Tuning key 4 overrides.
    //
    // Otherwise (round 3 sweep, same process) the best reservation follows the queue ids a resident wave takes over
    // the launch, I, and the frames per item, g: about I / (8 g), between 32 and 256.  Global-memory scenes (C3
    // stand-in): one-frame launches best at 48 (+4% over 32), 4-frame 128 (+3.8%), 8-frame 64 (+1.9%), 16-frame 32,
    // 32-frame 64 (+1%), 64-frame 128 (+1.3%), 256-frame 192-256 (+2.2%; C4 +2.1%); C2's 1024-frame launch 128
    // (+0.9%).  Fewer ids per wave than that make the queue atomic's round trip frequent; more leave the last waves
    // holding a long reservation in the launch tail.
    {
        const double waves = (double)im.n_cu * 4.0 * resident_waves(0, lds_scene);   // the fit ignores key 3
        const double ids = (double)im.n_tiles * (double)n_groups * 64.0;
        const int fit = 16 * (int)(ids / std::max(waves, 1.0) / (8.0 * p.group) / 16.0 + 0.5);
        const int auto_batch = std::max((int)kPullBatch, std::min(256, fit));
        p.pull_batch = t.pull_batch ? t.pull_batch
                                    : (lds_scene && p.group <= 2 ? (p.group == 1 ? 256 : 64) : auto_batch);
    }
    {   // exact item / n_groups by ceil(2^32 / n_groups) when item * n_groups < 2^32 for every
        // item (then floor(item * m / 2^32) = floor(item / n_groups)), else the division
        const unsigned long long items = (unsigned long long)im.n_tiles * n_groups;
        p.grp_magic = (n_groups > 1 && items * n_groups < (1ull << 32)) ? (unsigned)(((1ull << 32) + n_groups - 1) / n_groups) : 0u;
    }
    // Overlapped short launches: a short frame-split render (the reference's one dispatch per displayed frame,
    // ogl_path_trace.h:160-204) ends in a tail of nearly empty waves.  Its render kernel runs on an overlap slot (own
    // stream, colour scratch and queue counter) so the next render's waves fill the CUs that this one's tail frees
    // (enqueue_render). Not for captured graphs or counting.
    p.overlap = t.overlap_slots > 1 && !graph && !s.counting && !s.adaptive && n_frames <= kShortLaunch && p.split;
    const size_t lds = p.lds ? (p.cons_walk ? f.lds_bytes_sk : f.lds_bytes) : 0;
    // the wide walk's workgroup: wider ones share one LDS copy of more top records (tuning key 17); raysPerPixel > 1
    // keeps 256 threads
    const int wide_nt = (p.wide && im.rpp == 1) ? (t.wide_threads ? t.wide_threads : kWideThreadsAuto) : 256;
    p.nt = p.lds ? lds_threads(t, im, s, lds) : (p.wide ? wide_nt : 256);
    p.mw = resident_waves(t.minw, p.lds);
    {
        // persistent grid: enough resident waves to fill every SIMD; surplus blocks find the queue empty and exit.
        // Never more blocks than 8x8 tiles (64 lanes per tile).
        const unsigned items = (unsigned)im.n_tiles * (unsigned)n_groups;   // 64-lane items
        const unsigned wpb = (unsigned)p.nt / 64u;                           // waves per block
        p.blocks = std::min<unsigned>(im.persist_blocks * 256u / (unsigned)p.nt, std::max(1u, (items + wpb - 1) / wpb));
    }
    // Overlapped short renders (tuning key 18): at most this many 256-thread blocks per CU (automatic: one fewer than
    // resident, two fewer with 3+ render slots), so the accumulate pass and the ACES view of the previous render find
    // free slots beside the next render instead of waiting for its blocks to retire.  1080p Cornell, one frame per
    // dispatch (tools/interactive_fps.py): 0.534 -> 0.514 ms per frame, and 0.68 -> 0.55-0.58 with every frame shown
    // (pt_present, lag 2); accumulate pass 243 -> 103 us.  Round 5, 3 slots, 600-800 frames
    // (profiles/ab/r05i_interactive_sweep.json, r05j_*): render only, 2 / 3 / 4 / 5 blocks per CU 0.513 / 0.473 /
    // 0.537 / 0.493 ms per frame; every frame presented at lag 2, 3 blocks 0.55-0.62 against 0.530 at 5.  So 3 slots
    // take 3 blocks per CU, or 5 when the caller presented after the previous render (aces_fuse).
    if (p.overlap && p.nt == 256) {
        const int bpc = t.overlap_bpc ? t.overlap_bpc
                      : t.overlap_slots >= 3 ? (s.aces_fuse ? std::max(1, p.mw - 2) : 3)
                                             : std::max(1, p.mw - 1);
        p.blocks = std::min<unsigned>(p.blocks, (unsigned)(bpc * im.n_cu));
    }
    // global scene: the top nodes staged per block, at most what mw blocks per CU fit in its 160 KiB of LDS (the
    // first K of the breadth-first numbering, any K <= n_top)
    p.n_top = p.mw > 6 ? std::min(f.n_top, (int)kLdsCu / p.mw / 32 - 8) : f.n_top;
    // materials + spheres beside the top nodes when they are small (<= 4 KiB)
    const size_t shade_bytes = (size_t)(3 * f.n_mats + 2 * f.n_spheres) * 16;
    p.shade_lds = shade_bytes <= 4096;
    const size_t shade_lds_bytes = p.shade_lds ? shade_bytes : 0;
    if (p.wide) {   // top records: 48 B each, within the block's share of the CU's LDS
        // (256-thread blocks: one per resident wave per SIMD, the instantiation's 5-7; the raysPerPixel > 1 one is
        // built for 6)
        const size_t blocks_cu = wide_nt == 1024 ? 1
                               : (wide_nt == 256 ? (size_t)(im.rpp > 1 ? 6 : std::min(std::max(p.mw, 5), 7))
                                                 : (size_t)(6 * 256 / wide_nt));
        // (1 KiB below the even share: the allocation granule must not cost a block per CU)
        p.wide_top = (int)std::min<size_t>({(size_t)f.n_wide, (size_t)kWideTopMax,
                                            (kLdsCu / blocks_cu - shade_lds_bytes - 1024) / 48});
    }
    // what k_render_sm stages: the scene copy, or the top records / nodes and the shading records
    p.dyn_lds_bytes = p.lds ? lds : (p.wide ? (size_t)p.wide_top * 48 : (size_t)p.n_top * 32) + shade_lds_bytes;
    p.key = kernel_key(s.counting, p.lds, p.wide, p.split, p.mw, im.rpp, p.nt, f.walk_np);
    p.common = !s.adaptive && common_launch(f, t, im, p);
    // the sweep is in the 256-thread LDS lines only (a scene with a sweep table is far below the wide workgroups' sizes)
    p.sweep = p.lds && p.nt == 256 && sweep_on(f, t, s.counting);
    if (p.sweep && !t.shade_thresh) p.shade_thresh = kSweepShadeThresh;
    {
        // The path pool: the specialised swept line only, not on an overlap slot (below), the
        // packed fields of a path hold this launch (pt_pool.h; the bounce limit is enqueue_render's to check), and the
        // pools and the trimmed scene -- triangle slots, materials, the sphere, the leaf boxes -- fit the CU's LDS.
        // Workgroups per CU: what the LDS holds (1 KiB below the even share, for the allocation granule), at most
        // kPoolWaves waves per SIMD, the kernel's register budget.  The condition is the overlap slot, not the launch's
        // length: a launch of 1 to 16 frames on the context's stream (a captured graph's, or with key 9 = 1) pools, and
        // gains (same-process A/B against k_render_sm with key 9 = 1, 1080p Cornell: 1-frame launches +18.8%, 4-frame
        // +4.3%, 16-frame +5.0%, 64-frame +5.6%); overlapped launches were not measured with the pool.  The pool runs only at that occupancy, the one
        // its constants were measured at: one wave per SIMD fewer already loses to k_render_sm (128 x 256 at 3 waves:
        // -5% on C2), so a scene whose trimmed copy costs a workgroup per CU (more than about 5.6 KB) keeps k_render_sm.
        // The leaf boxes are staged as the signed table the sweep reads by ray sign, 3 quads per leaf (pt_cull.h; the
        // exact re-test reads its positive variants): Cornell 3,728 B; 24 leaves of 48 slots and 13 materials 4,880 B.
        p.pool_paths = kPoolPaths, p.pool_nt = kPoolThreads;
        const int wpb = kPoolThreads / 64;
        const size_t scene = (size_t)(4 * f.n_slots + 3 * f.n_mats + 2 * f.n_spheres + 3 * f.n_leaves) * 16;
        p.pool_lds_bytes = ptpool::block_bytes(kPoolPaths, wpb, scene);
        const int full_cu = 4 * kPoolWaves / wpb;
        const int per_cu = (int)std::min<size_t>(kLdsCu / (p.pool_lds_bytes + 1024), (size_t)full_cu);
        p.pool = kPoolDefault && !t.pool_off && p.common && p.sweep && !p.overlap && per_cu >= 1 && per_cu == full_cu &&
                 ptpool::pack_ok(im.width, im.rows_local, n_frames, 0, f.n_slots, f.n_spheres);
        const unsigned long long paths = (unsigned long long)im.n_tiles * n_groups * 64ull, per_block = (unsigned long long)(kPoolPaths * wpb);
        p.pool_blocks = (unsigned)std::min<unsigned long long>((unsigned long long)std::max(per_cu, 1) * (unsigned long long)std::max(im.n_cu, 1),
                                                               std::max(1ull, (paths + per_block - 1) / per_block));
    }
    if (p.split) {  // the accumulate pass: the long variant loads 8 frames per group
        p.accum_long = n_frames > kShortLaunch;
        p.accum_moments = s.moments;
        // a presenting caller's view of the new image, written by the same pass (not inside a captured graph: its
        // replays are not followed by pt_present_begin's check)
        p.aces_out = s.aces_fuse && !graph;
        const long long px = (long long)im.rows_local * im.width, per_block = 256 * (p.accum_long ? kAccumPixLong : kAccumPix);
        p.accum_blocks = (unsigned)((px + per_block - 1) / per_block);
    }
    return p;
}

size_t scratch_bytes(const LaunchPlan& plan, const Image& im, int n_frames) {
    if (!plan.split) return 0;
    return (size_t)std::max(im.rows_local, 1) * (size_t)im.width * (size_t)n_frames * 3 * sizeof(float);
}

}  // namespace ptl
