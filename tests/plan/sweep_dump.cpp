// sweep_dump -- the launch planner's `sweep` flag (csrc/pt_launch_plan.cpp, sweep_on) on the CPU for
// tests/test_leaf_sweep.py.  Reads cases on stdin, one per line: the 43 integers of common_dump's case
// (tests/plan/common_dump.cpp) and then n_leaves, sweep_ok, win_bad, sweep_off; prints "sweep common cons_walk key".
#include "../../opengl-path-tracing_amd/csrc/pt_launch_plan.h"

#include <cstdio>
#include <cstdlib>

int main() {
    constexpr int kIn = 47;
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
        if (n != kIn) { fprintf(stderr, "sweep_dump: a case is %d integers\n", kIn); return 2; }
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
        im.tile_shift = (int)v[i++];
        t.common_off = (int)v[i++];
        f.n_leaves = (int)v[i++];
        f.sweep_ok = v[i++] != 0;
        f.win_bad = v[i++] != 0;
        t.sweep_off = (int)v[i++];
        const ptl::LaunchPlan p = ptl::plan_launch(f, t, im, s, n_frames, graph);
        const ptl::KernelKey& k = p.key;
        printf("%d %d %d %d,%d,%d,%d,%d,%d,%d,%d\n", p.sweep, p.common, p.cons_walk, k.count, k.lds, k.minw, k.multi, k.split,
               k.padn, k.nt, k.wide);
    }
    return 0;
}
