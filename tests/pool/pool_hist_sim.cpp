// pool_hist_sim.cpp -- tests/pool/pool_sim.cpp's cost model with the candidate histogram as an argument: one wave, P
// paths, the two ready lists and the phase rule of pt_pool.h, driven with a given distribution of candidates per
// segment (tests/pool/plane_window_sim.cpp reports the filtered one) through refill and drain.
//   pool_hist_sim P items h0 h1 h2 h3 h4 [shade_cost leaf_cost list_cost]
// h0..h3: the shares of segments with 0..3 candidates, h4: with 4 to 6 (drawn evenly, as pool_sim draws them).
// The same generator, draw order and per-pass costs as pool_sim: with pool_sim's own histogram (0.137 0.487 0.246
// 0.082 0.048) it prints pool_sim's figures, which tests/test_plane_window.py checks.  The invariants of the lists
// are pool_sim's to check, not this driver's.  Prints one JSON line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pt_pool.h"

using namespace ptpool;

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static double rnd01() { return rnd() / 16777216.0; }
static double g_h[4];
static int draw_candidates() {
    const double u = rnd01();
    if (u < g_h[0]) return 0;
    if (u < g_h[0] + g_h[1]) return 1;
    if (u < g_h[0] + g_h[1] + g_h[2]) return 2;
    if (u < g_h[0] + g_h[1] + g_h[2] + g_h[3]) return 3;
    return 4 + (int)(rnd() % 3u);
}

struct Path { int item = -1, segs_left = 0, cands = 0; bool seg = false, retired = false; };

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: pool_hist_sim P items h0 h1 h2 h3 h4 [shade_cost leaf_cost list_cost]\n"); return 2; }
    const int P = atoi(argv[1]);
    const long long n_items = atoll(argv[2]);
    for (int i = 0; i < 4; i++) g_h[i] = atof(argv[3 + i]);
    const double c_shade = argc > 8 ? atof(argv[8]) : 720.0, c_leaf = argc > 9 ? atof(argv[9]) : 450.0;
    const double c_list = argc > 10 ? atof(argv[10]) : 30.0;
    if (P < 1 || P > kMaxPaths) return 2;
    std::vector<Path> path(P);
    std::vector<unsigned char> list(list_bytes(P) < P ? P : list_bytes(P));
    for (int i = 0; i < P; i++) list[i] = (unsigned char)i;
    Lists L = {P, 0};
    long long next_item = 0, passes[2] = {0, 0}, lanes[2] = {0, 0}, segments = 0, visits = 0;
    while (L.nS + L.nL > 0) {
        const int phase = choose(L), n = take(L, phase);
        int idx[kLanes], to[kLanes];
        for (int lane = 0; lane < n; lane++) idx[lane] = list[pop_index(L, phase, n, lane, P)];
        drop(L, phase, n);
        passes[phase]++;
        lanes[phase] += n;
        for (int lane = 0; lane < n; lane++) {
            Path& p = path[idx[lane]];
            if (phase == kShade) {
                if (p.seg) { segments++; p.seg = false; }
                if (p.item >= 0 && p.segs_left == 0) p.item = -1;
                if (p.item < 0) {
                    if (next_item >= n_items) { p.retired = true; to[lane] = -1; continue; }
                    p.item = (int)next_item++;
                    p.segs_left = 1 + (int)(rnd() % 9u);
                }
                p.segs_left--;
                p.seg = true;
                p.cands = draw_candidates();
                visits += p.cands;
                to[lane] = p.cands ? kLeaf : kShade;
            } else {
                p.cands--;
                to[lane] = p.cands ? kLeaf : kShade;
            }
        }
        int rank[2] = {0, 0};
        for (int lane = 0; lane < n; lane++)
            if (to[lane] >= 0) list[push_index(L, to[lane], rank[to[lane]]++, P)] = (unsigned char)idx[lane];
        grow(L, kShade, rank[kShade]);
        grow(L, kLeaf, rank[kLeaf]);
    }
    const double valu = segments ? (passes[0] * (c_shade + c_list) + passes[1] * (c_leaf + c_list)) / (double)segments : 0.0;
    printf("{\"P\": %d, \"segments\": %lld, \"visits_per_segment\": %.4f, \"shade_passes\": %lld, \"leaf_passes\": %lld, "
           "\"shade_lane_use\": %.4f, \"leaf_lane_use\": %.4f, \"wave_valu_per_segment\": %.2f}\n",
           P, segments, segments ? visits / (double)segments : 0.0, passes[0], passes[1],
           passes[0] ? lanes[0] / (64.0 * passes[0]) : 0.0, passes[1] ? lanes[1] / (64.0 * passes[1]) : 0.0, valu);
    return 0;
}
