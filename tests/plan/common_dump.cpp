// common_dump -- the launch planner's `common` flag (csrc/pt_launch_plan.cpp, common_launch) on the
// CPU for tests/test_common_plan.py.
//   common_dump            reads cases on stdin, one per line: the 40 integers of plan_dump's case
//                          (tests/golden/launch_plans.txt's header) and then root_child, tile_shift,
//                          common_off; prints "common key" per case
//   common_dump --kernels  prints the key of every line of PT_RENDER_KERNELS_COMMON
#include "../../opengl-path-tracing_amd/csrc/pt_launch_plan.h"
#include "../../opengl-path-tracing_amd/csrc/pt_render_kernels.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static void print_key(const ptl::KernelKey& k) {
    printf("%d,%d,%d,%d,%d,%d,%d,%d", k.count, k.lds, k.minw, k.multi, k.split, k.padn, k.nt, k.wide);
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--kernels")) {
#define X(C, L, MW, M, S, P, NT, W) print_key(ptl::KernelKey{C, L, MW, M, S, P, NT, W}); printf("\n");
        PT_RENDER_KERNELS_COMMON(X)
#undef X
        return 0;
    }
    constexpr int kIn = 43;
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
        if (n != kIn) { fprintf(stderr, "common_dump: a case is %d integers\n", kIn); return 2; }
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
        const ptl::LaunchPlan p = ptl::plan_launch(f, t, im, s, n_frames, graph);
        printf("%d ", p.common);
        print_key(p.key);
        printf("\n");
    }
    return 0;
}
