// pool_sim.cpp -- CPU model of the per-wave path pool (pt_pool.h): one wave, P paths, the two ready lists and the
// phase rule, driven with the candidate distribution of C2's segments (leaf_sweep_sim: 13.7% none, 48.7% one, 24.6%
// two, 8.2% three, 4.8% more) through refill from a work queue and the drain at its end.
//   pool_sim P items [shade_cost leaf_cost list_cost]
// Checks at every pass: every path is in exactly one place (a list entry, running, or retired), nothing is lost or
// duplicated, and while the queue has work a pass runs at least min(64, ceil(P / 2)) lanes.  Prints one JSON line:
// the lane use per pass and the modelled wave-VALU per segment from the per-pass costs.
// Exit code 0: every check held.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pt_pool.h"

using namespace ptpool;

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static double rnd01() { return rnd() / 16777216.0; }
static int draw_candidates() {
    const double u = rnd01();
    if (u < 0.137) return 0;
    if (u < 0.137 + 0.487) return 1;
    if (u < 0.137 + 0.487 + 0.246) return 2;
    if (u < 0.137 + 0.487 + 0.246 + 0.082) return 3;
    return 4 + (int)(rnd() % 3u);
}

struct Path { int item = -1, segs_left = 0, cands = 0; bool seg = false, retired = false; };

int main(int argc, char** argv) {
    const int P = argc > 1 ? atoi(argv[1]) : 96;
    long long items = argc > 2 ? atoll(argv[2]) : 20000;
    const double c_shade = argc > 3 ? atof(argv[3]) : 720.0, c_leaf = argc > 4 ? atof(argv[4]) : 450.0;
    const double c_list = argc > 5 ? atof(argv[5]) : 30.0;
    if (P < 1 || P > kMaxPaths) return 2;
    const long long n_items = items;
    std::vector<Path> path(P);
    std::vector<unsigned char> list(list_bytes(P) < P ? P : list_bytes(P));
    std::vector<long long> done(n_items, 0);     // segments finished per item: each exactly its own count
    std::vector<int> want(n_items, 0);
    for (int i = 0; i < P; i++) list[i] = (unsigned char)i;
    Lists L = {P, 0};
    long long next_item = 0, passes[2] = {0, 0}, lanes[2] = {0, 0}, segments = 0, violations = 0, short_passes = 0;
    const int floor_lanes = std::min(kLanes, (P + 1) / 2);
    while (L.nS + L.nL > 0) {
        // invariant: the list entries are distinct live paths, and every live path is in one list
        std::vector<int> seen(P, 0);
        for (int i = 0; i < L.nS; i++) seen[list[i]]++;
        for (int i = 0; i < L.nL; i++) seen[list[P - 1 - i]]++;
        for (int i = 0; i < P; i++)
            if (seen[i] != (path[i].retired ? 0 : 1)) violations++;
        if (L.nS + L.nL > P) violations++;
        const int phase = choose(L), n = take(L, phase);
        // the pigeonhole bound, while no path has retired (the queue has work)
        if (next_item < n_items && n < floor_lanes) short_passes++;
        int idx[kLanes];
        for (int lane = 0; lane < n; lane++) idx[lane] = list[pop_index(L, phase, n, lane, P)];
        drop(L, phase, n);
        passes[phase]++;
        lanes[phase] += n;
        int to[kLanes];      // the new state: kShade, kLeaf or -1 = retired
        for (int lane = 0; lane < n; lane++) {
            Path& p = path[idx[lane]];
            if (p.retired) violations++;
            if (phase == kShade) {
                if (p.cands != 0) violations++;
                if (p.seg) {                            // a finished segment
                    done[p.item]++;
                    segments++;
                    p.seg = false;
                }
                if (p.item >= 0 && p.segs_left == 0) p.item = -1;
                if (p.item < 0) {
                    if (next_item >= n_items) { p.retired = true; to[lane] = -1; continue; }
                    p.item = (int)next_item++;
                    p.segs_left = want[p.item] = 1 + (int)(rnd() % 9u);     // a path of 1..9 segments
                }
                p.segs_left--;                          // set up the next segment
                p.seg = true;
                p.cands = draw_candidates();
                to[lane] = p.cands ? kLeaf : kShade;
            } else {
                if (p.cands <= 0) violations++;
                p.cands--;
                to[lane] = p.cands ? kLeaf : kShade;
            }
        }
        int rank[2] = {0, 0};
        for (int lane = 0; lane < n; lane++) {
            if (to[lane] < 0) continue;
            list[push_index(L, to[lane], rank[to[lane]]++, P)] = (unsigned char)idx[lane];
        }
        grow(L, kShade, rank[kShade]);
        grow(L, kLeaf, rank[kLeaf]);
    }
    long long lost = 0;
    for (long long i = 0; i < n_items; i++) lost += done[i] != want[i];
    for (int i = 0; i < P; i++) lost += !path[i].retired;
    lost += next_item != n_items;
    const double np = (double)(passes[0] + passes[1]);
    const double use = (lanes[0] + lanes[1]) / (64.0 * np);
    const double valu = segments ? (passes[0] * (c_shade + c_list) + passes[1] * (c_leaf + c_list)) / (double)segments : 0.0;
    printf("{\"P\": %d, \"segments\": %lld, \"shade_passes\": %lld, \"leaf_passes\": %lld, \"lane_use\": %.4f, "
           "\"shade_lane_use\": %.4f, \"leaf_lane_use\": %.4f, \"wave_valu_per_segment\": %.2f, \"violations\": %lld, "
           "\"lost\": %lld, \"short_passes\": %lld, \"floor_lanes\": %d}\n",
           P, segments, passes[0], passes[1], use, lanes[0] / (64.0 * passes[0]),
           passes[1] ? lanes[1] / (64.0 * passes[1]) : 0.0, valu, violations, lost, short_passes, floor_lanes);
    return (violations || lost || short_passes) ? 1 : 0;
}
