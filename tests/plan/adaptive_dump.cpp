// adaptive_dump -- plan_dump for the launches of pt_render_adaptive: the same 40-integer cases on
// stdin and the same "case | plan" lines, but planned with State::adaptive set, as
// enqueue_adaptive (pt_ctx_noise.h) does, n_tiles being the launch's list of active tiles.  After
// the plan_dump fields come `overlap` and `common` once more, named, for tests/test_adaptive_plan.py.
#include "../../opengl-path-tracing_amd/csrc/pt_launch_plan.h"

#include <cstdio>
#include <cstdlib>

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        long long v[40];
        int n = 0;
        for (char* s = line; n < 40; n++) {
            char* e;
            v[n] = strtoll(s, &e, 10);
            if (e == s) break;
            s = e;
        }
        if (n != 40) { fprintf(stderr, "adaptive_dump: a case is 40 integers\n"); return 2; }
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
        s.adaptive = true;
        const int n_frames = (int)v[i++];
        const bool graph = v[i++] != 0;
        const ptl::LaunchPlan p = ptl::plan_launch(f, t, im, s, n_frames, graph);
        for (int k = 0; k < 40; k++) printf("%lld ", v[k]);
        printf("| %d %d %d %d %d %d %d %d %d %d %d %u %d %d %d %d %d %u %zu %d %d %d %u ", p.lds, p.wide, p.cons_walk,
               p.leaf_cert, p.split, p.overlap, p.shade_lds, p.nt, p.mw, p.group, p.pull_batch, p.grp_magic, p.leaf_thresh,
               p.shade_thresh, p.trav_floor, p.n_top, p.wide_top, p.blocks, p.dyn_lds_bytes, p.accum_long, p.accum_moments,
               p.aces_out, p.accum_blocks);
        const ptl::KernelKey& k = p.key;
        printf("%d,%d,%d,%d,%d,%d,%d,%d", k.count, k.lds, k.minw, k.multi, k.split, k.padn, k.nt, k.wide);
        printf(" %d %zu %llu %d %d\n", ptl::launch_frames(f, t, im, s, n_frames), ptl::scratch_bytes(p, im, n_frames),
               ptl::id_limit(t, im), p.overlap, p.common);
    }
    return 0;
}
