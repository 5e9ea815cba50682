// pt_pool.h -- the per-wave path pool of swept tiny scenes: the state record of a path, its
// packing limits, the LDS layout and the two ready lists of a wave.  Plain host/device code, no HIP, like
// pt_cull.h and pt_wide.h: the CPU model tests/pool/pool_sim.cpp runs these functions.
//
// With the leaf sweep a guarded ray never walks, so a path waits in one of two states: to SHADE (finish a
// segment, pull work, set up the next segment) or at a LEAF (candidate bits left in `bi`).  A wave owns P paths
// in LDS and may hand any path to any lane.  Every path is in exactly one of: the SHADE list, the LEAF list,
// running in the current pass, retired.  Between passes nothing runs, so nS + nL = P - retired, and the longer
// list holds at least half of the live paths: with P = 128 and no path retired every pass runs 64 full lanes.
#pragma once

#include <stdint.h>

#include "pt_math.h"

namespace ptpool {

constexpr int kLanes = 64;
constexpr int kMaxPaths = 128;      // list entries are one byte; two full passes' worth of paths
constexpr int kRecDwords = 20;      // one path: five 16-byte chunks
constexpr int kChunks = kRecDwords / 4;

// The record, chunk by chunk.  A chunk is what one ds_read_b128 moves; chunk c of path i sits at quad c * P + i of
// the wave's pool, so the 16 lanes of a ds_read_b128 group that hold consecutive paths cover all 64 banks, and
// after compaction (arbitrary path indices) two lanes of a group collide only when their paths are equal mod 16.
//   0: o.xyz, t                       (LEAF reads; LEAF writes t)
//   1: d.xyz, bi                      (LEAF reads; LEAF writes bi)
//   2: inc.xyz, hprim | bounce        (LEAF reads and writes the fourth dword)
//   3: col.xyz, rng state
//   4: lx | crow, aidx, k | kend, pcost | tile-report flag
// rd is not stored: the LEAF pass rebuilds it by rcp_fast from the same d, the same bits.
enum : int { kChunkO = 0, kChunkD = 1, kChunkInc = 2, kChunkCol = 3, kChunkItem = 4 };

// Quad index of chunk c of path i in a pool of P paths.
PT_HD int quad_of(int c, int i, int P) { return c * P + i; }
// Bytes of one wave's pool: the records, then the list array (one byte per path, padded to 16).
PT_HD int list_bytes(int P) { return (P + 15) & ~15; }
PT_HD int wave_bytes(int P) { return P * kRecDwords * 4 + list_bytes(P); }

// --- packing.  The limits the packed fields assume (pack_ok: the planner refuses the pool where one fails).
//   lx | crow << 16        : width <= 65535 and local rows <= 65535; 0xffffffff = no work item
//   k | kend << 16         : frames per launch <= 65535
//   (hprim + 2) | (bounce + 1) << 16 : hprim in [-2, n_slots) with one sphere (-2) and -1 = no hit, n_slots + 2 <=
//                            65535; bounce in [-1, max_bounce + 1], max_bounce <= 65533
//   pcost | report << 31   : segments of one work item, at most group * (max_bounce + 2) < 2^31
constexpr uint32_t kNoItem = 0xffffffffu;
PT_HD bool pack_ok(int width, int rows_local, int n_frames, int max_bounce, int n_slots, int n_spheres) {
    return width >= 1 && width <= 65535 && rows_local >= 0 && rows_local <= 65535 && n_frames >= 1 &&
           n_frames <= 65535 && max_bounce >= 0 && max_bounce <= 65533 && n_slots >= 0 && n_slots <= 65533 &&
           n_spheres == 1 && (long long)n_frames * (long long)(max_bounce + 2) < (1ll << 31);
}
PT_HD uint32_t pack_xy(int lx, int crow) { return (uint32_t)lx | ((uint32_t)crow << 16); }
PT_HD int xy_lx(uint32_t v) { return (int)(v & 0xffffu); }
PT_HD int xy_crow(uint32_t v) { return (int)(v >> 16); }
PT_HD uint32_t pack_k(int k, int kend) { return (uint32_t)k | ((uint32_t)kend << 16); }
PT_HD int k_k(uint32_t v) { return (int)(v & 0xffffu); }
PT_HD int k_kend(uint32_t v) { return (int)(v >> 16); }
PT_HD uint32_t pack_hit(int hprim, int bounce) { return (uint32_t)(hprim + 2) | ((uint32_t)(bounce + 1) << 16); }
PT_HD int hit_hprim(uint32_t v) { return (int)(v & 0xffffu) - 2; }
PT_HD int hit_bounce(uint32_t v) { return (int)(v >> 16) - 1; }
PT_HD uint32_t with_hprim(uint32_t v, int hprim) { return (v & 0xffff0000u) | (uint32_t)(hprim + 2); }
PT_HD uint32_t pack_cost(uint32_t pcost, bool report) { return pcost | (report ? 0x80000000u : 0u); }
PT_HD uint32_t cost_of(uint32_t v) { return v & 0x7fffffffu; }
PT_HD bool cost_report(uint32_t v) { return (v >> 31) != 0u; }

// --- the two ready lists: stacks growing from the two ends of one P-entry byte array.  SHADE entries are
// [0, nS), LEAF entries [P - nL, P).  They fit exactly: a path is in one list, running, or retired.
enum : int { kShade = 0, kLeaf = 1 };
struct Lists { int nS, nL; };   // wave-uniform

// The phase rule: the list with more ready paths (SHADE on a tie: it is what refills the pool).
PT_HD int choose(const Lists& l) { return l.nS >= l.nL ? kShade : kLeaf; }
// Paths of the pass: up to one per lane.
PT_HD int take(const Lists& l, int phase) {
    const int n = phase == kShade ? l.nS : l.nL;
    return n < kLanes ? n : kLanes;
}
// Array index lane `lane` (< n) pops, from the top of the chosen stack; the caller then drops n entries.
PT_HD int pop_index(const Lists& l, int phase, int n, int lane, int P) {
    return phase == kShade ? l.nS - n + lane : P - l.nL + lane;
}
PT_HD void drop(Lists& l, int phase, int n) {
    if (phase == kShade) l.nS -= n; else l.nL -= n;
}
// Array index at which the lane of rank `rank` (set bits of the pushing ballot below it) stores its path.
PT_HD int push_index(const Lists& l, int phase, int rank, int P) {
    return phase == kShade ? l.nS + rank : P - 1 - l.nL - rank;
}
PT_HD void grow(Lists& l, int phase, int n) {
    if (phase == kShade) l.nS += n; else l.nL += n;
}

// What the planner needs: the LDS of a workgroup of `waves` waves beside `scene_bytes` of trimmed scene, and the
// workgroups a CU holds.
PT_HD size_t block_bytes(int P, int waves, size_t scene_bytes) {
    return ((scene_bytes + 15) & ~(size_t)15) + (size_t)waves * (size_t)wave_bytes(P);
}

}  // namespace ptpool
