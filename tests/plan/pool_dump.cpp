// pool_dump -- the launch planner's path-pool decision (csrc/pt_launch_plan.cpp) on the CPU for
// tests/test_pool_plan.py.  Reads cases on stdin, one per line: the 40 integers of plan_dump's case
// (tests/golden/launch_plans.txt's header) and then root_child, n_leaves, sweep_ok, sweep_off, pool_off, adaptive.
// Prints per case: pool common sweep pool_paths pool_nt pool_blocks pool_lds_bytes overlap, the workgroups per CU
// (pool_blocks is at most that many per CU), and `same` = 1 when every generic plan field is equal with tuning key
// 24 at 0 and at 1.
#include "../../opengl-path-tracing_amd/csrc/pt_launch_plan.h"

#include <cstdio>
#include <cstdlib>

static bool same_generic(const ptl::LaunchPlan& a, const ptl::LaunchPlan& b) {
    return a.lds == b.lds && a.wide == b.wide && a.cons_walk == b.cons_walk && a.leaf_cert == b.leaf_cert &&
           a.split == b.split && a.overlap == b.overlap && a.shade_lds == b.shade_lds && a.nt == b.nt && a.mw == b.mw &&
           a.group == b.group && a.pull_batch == b.pull_batch && a.leaf_thresh == b.leaf_thresh &&
           a.shade_thresh == b.shade_thresh && a.trav_floor == b.trav_floor && a.n_top == b.n_top &&
           a.wide_top == b.wide_top && a.grp_magic == b.grp_magic && a.blocks == b.blocks &&
           a.dyn_lds_bytes == b.dyn_lds_bytes && a.accum_long == b.accum_long && a.accum_moments == b.accum_moments &&
           a.aces_out == b.aces_out && a.accum_blocks == b.accum_blocks && a.key == b.key && a.common == b.common &&
           a.sweep == b.sweep;
}

int main() {
    constexpr int kIn = 46;
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        long long v[kIn];
        int n = 0;
        for (char* s = line; n < kIn; n++) {
            char* e;
            v[n] = strtoll(s, &e, 10);
            if (e == s) break;
            s = e;
        }
        if (n != kIn) { fprintf(stderr, "pool_dump: a case is %d integers\n", kIn); return 2; }
        ptl::SceneFacts f;
        ptl::Tuning t;
        int i = 0;
        f.n_nodes = (int)v[i++]; f.n_spheres = (int)v[i++]; f.n_mats = (int)v[i++]; f.n_slots = (int)v[i++];
        f.n_top = (int)v[i++]; f.walk_np = (int)v[i++]; f.scene_fast = (int)v[i++]; f.walk_nested = v[i++] != 0;
        f.wide_ok = v[i++] != 0; f.n_wide = (int)v[i++]; f.leaf_cert_ok = v[i++] != 0;
        f.lds_bytes = (size_t)v[i++]; f.lds_bytes_sk = (size_t)v[i++];
        t.leaf_thresh = (int)v[i++]; t.shade_thresh = (int)v[i++]; t.minw = (int)v[i++]; t.trav_floor = (int)v[i++];
        t.compact_max = (int)v[i++]; t.pull_batch = (int)v[i++]; t.group_force = (int)v[i++]; t.cons_off = (int)v[i++];
        t.wide_off = (int)v[i++]; t.wide_threads = (int)v[i++]; t.overlap_bpc = (int)v[i++]; t.cert_off = (int)v[i++];
        t.overlap_slots = (int)v[i++]; t.scratch_budget = (size_t)v[i++]; t.variant = (int)v[i++];
        ptl::Image im;
        im.width = (int)v[i++]; im.rows_local = (int)v[i++]; im.n_tiles = (int)v[i++]; im.rpp = (int)v[i++];
        im.flags = (int)v[i++]; im.n_cu = (int)v[i++]; im.persist_blocks = (unsigned)v[i++];
        ptl::State s;
        s.counting = v[i++] != 0; s.moments = v[i++] != 0; s.aces_fuse = v[i++] != 0;
        const int n_frames = (int)v[i++];
        const bool graph = v[i++] != 0;
        f.root_child = (int)v[i++];
        f.n_leaves = (int)v[i++];
        f.sweep_ok = v[i++] != 0;
        t.sweep_off = (int)v[i++];
        t.pool_off = (int)v[i++];
        s.adaptive = v[i++] != 0;
        const ptl::LaunchPlan p = ptl::plan_launch(f, t, im, s, n_frames, graph);
        ptl::Tuning t0 = t, t1 = t;
        t0.pool_off = 0, t1.pool_off = 1;
        const ptl::LaunchPlan p0 = ptl::plan_launch(f, t0, im, s, n_frames, graph), p1 = ptl::plan_launch(f, t1, im, s, n_frames, graph);
        const unsigned per_cu = (p.pool_blocks + (unsigned)im.n_cu - 1) / (unsigned)im.n_cu;
        printf("%d %d %d %d %d %u %zu %d %u %d\n", p.pool, p.common, p.sweep, p.pool_paths, p.pool_nt, p.pool_blocks,
               p.pool_lds_bytes, p.overlap, per_cu, same_generic(p0, p1) && !p1.pool);
    }
    return 0;
}
