// pt_scene_pack.h -- scene validation and the device layouts, as host data.  Plain C++, no HIP, no
// device allocation: pt_upload_scene (pt_render.hip) copies the packed buffers to the device as they are, and
// tests/test_scene_pack.py runs the packer on the CPU -- a wrong offset in a walk image otherwise shows only as a
// wrong image or a fault on the GPU.
#pragma once

#include "pt_cull.h"
#include "pt_launch_plan.h"
#include "pt_math.h"

#include <stddef.h>

#include <string>
#include <vector>

namespace ptp {

// The device buffers of a scene, 16-byte quads each.  pt_ctx, pt__scene_replicate_layout and
// pt_group_upload_scene index by this list.
enum SceneBuf {
    kNodes,        // axis-paired node records, 2 quads per node, in the top numbering
    kTris,         // 8 quads per leaf: its two triangles (plane, v0, v1, v2)
    kMats,         // 3 quads per material
    kSpheres,      // 2 quads per sphere
    kWalk,         // the LDS walk's 8 octant images (links as byte offsets)
    kWalkSink,     // ... the culling walk's copy with its ninth image of sinks (nested trees)
    kWideRec,      // the wide tree's records, kWideStride quads each (pt_wide.h)
    kWideLeafBox,  // its exact leaf boxes, 2 quads per index
    kWideNodes,    // kNodes with leaf codes numbered by the wide index
    kWideTris,     // kTris numbered by the wide index
    kBufs,         // the buffers above: the rows of tests/golden/scene_packs.txt list exactly these
    // the leaf sweep's table (pt_cull.h, sweep_mask): per leaf in chain order -- the order the reference walk reaches
    // them -- 2 quads, {lo.x, hi.x, lo.y, hi.y}, {lo.z, hi.z, its pair index, the chain position of pair k (the
    // inverse map)}; only for a scene with sweep_ok.  A sweeping kernel stages the triangle slots in chain order.
    kSweep = kBufs,
    // the ray query's leaf table (pt_query.h): per leaf slot pair k one quad {tri0, tri1, 0, 0} as integer bits, the
    // reference triangle indices (b.data[0], b.data[1]) a hit record reports
    kLeafTris,
    kBufsAll       // every device buffer of a scene
};

// global-memory scenes: the first kTopNodes device nodes (breadth-first from the root) are
// staged in LDS, 24 KiB per workgroup (6 workgroups per CU stay resident)
constexpr int kTopNodes = 768;
// quads per device record of the wide tree: the three quads of pt_wide.h packed (48 B) or on a 64-B stride
#ifndef PT_WIDE_STRIDE
#define PT_WIDE_STRIDE 3
#endif
constexpr int kWideStride = PT_WIDE_STRIDE;

struct Quad { float x, y, z, w; };
static_assert(sizeof(Quad) == 16, "a device quad");

struct PackedScene {
    std::vector<float> buf[kBufsAll];   // 4 floats per quad
    ptl::SceneFacts facts;
};

// Quads of buffer b of a scene with these facts (0: the scene has no such buffer).  pack_scene fills exactly this
// many (it refuses with an internal error otherwise); pt__scene_replicate_layout allocates by it.
size_t buf_quads(const ptl::SceneFacts& f, int b);

// The checks of the counts and pointers alone, pack_scene's first step (pt_upload_scene runs them before it touches
// the device): PT_OK, or PT_E_ARG / PT_E_SCENE with `err` set.
int check_scene_args(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                     const float* spheres, int n_spheres, std::string& err);

// Validates the scene (std140 records: 16 floats per triangle and material, 12 per node, 8 per sphere) and packs
// its device buffers and facts into `out`.  PT_OK, or PT_E_ARG / PT_E_SCENE with `err` set and `out` unspecified.
int pack_scene(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
               const float* spheres, int n_spheres, PackedScene& out, std::string& err);

// --- the rules below are also what the CPU walk models run (tests/wide/wide_sim.cpp, tests/cull/window_cull_sim.cpp)

// A triangle's stored plane (n, d0): quad 0 of its device record, which the plane test reads alone.
inline Quad tri_plane(const float* t) {
    const pt::f3 v0 = pt::mk(t[0], t[1], t[2]), v1 = pt::mk(t[4], t[5], t[6]), v2 = pt::mk(t[8], t[9], t[10]);
    const pt::f3 n = pt::normalize(pt::cross(v1 - v0, v2 - v0));
    return {n.x, n.y, n.z, -pt::dot(n, v0)};
}
// Coplanar leaf pair: both triangles carry the same (n, d0) up to the sign of zero components (the two halves of an
// OBJ quad, a single-triangle leaf's copy), flagged in the leaf code (bit 1).  hit_triangle's plane distance
// -(dot(n,o) + d0) / dot(n,d) is then the same for both wherever it can pass the leaf's acceptance tests: a zero
// factor of either sign only changes the sign of zero intermediate sums, so the two quotients are bitwise equal or
// both +-0, +-inf or NaN, which fail t > 1e-4 / t >= 1e-4 alike.  NaN (a degenerate triangle) never compares equal:
// such pairs are not flagged.
inline bool same_plane(const Quad& A, const Quad& B) { return A.x == B.x && A.y == B.y && A.z == B.z && A.w == B.w; }

// Device node numbering: the first kTopNodes nodes in breadth-first order of the walk links from the root (the nodes
// nearly every walk passes: the global-memory walk keeps them in LDS, node_at), the rest in their original order.
// Links are renumbered with the nodes, so every walk visits the same node sequence; the root stays node 0.  The
// links must be valid (pack_scene validates them first).
inline std::vector<int> top_numbering(const float* bvh, int n_nodes) {
    std::vector<int> pos(n_nodes, -1);
    int nx = 0;
    std::vector<int> q;
    if (n_nodes > 0) { pos[0] = nx++; q.push_back(0); }
    for (size_t qi = 0; qi < q.size() && nx < kTopNodes; qi++) {
        const float* nd = bvh + 12 * (size_t)q[qi];
        for (int l = 10; l < 12; l++) {
            const int t = (int)nd[l];
            if (t >= 0 && pos[t] < 0 && nx < kTopNodes) { pos[t] = nx++; q.push_back(t); }
        }
    }
    for (int i = 0; i < n_nodes; i++)
        if (pos[i] < 0) pos[i] = nx++;
    return pos;
}

// The leaf re-test certificate (ptw::leaf_certificate) and the window clause need each leaf box to contain its
// triangles' vertices -- the reference builder expands leaf boxes over them (bvh.h:29-52); an uploaded tree is
// checked, not assumed.  Leaf triangle indices must be valid.
inline bool leaves_contain_tris(const float* bvh, int n_nodes, const float* tris) {
    for (int i = 0; i < n_nodes; i++) {
        const float* nd = bvh + 12 * (size_t)i;
        if (!(nd[8] > -1.0f)) continue;
        for (int k = 0; k < 2; k++) {
            const float* t = tris + 16 * (size_t)(int)nd[8 + k];
            for (int v = 0; v < 3; v++)
                for (int q = 0; q < 3; q++)
                    if (!(nd[q] <= t[4 * v + q] && t[4 * v + q] <= nd[4 + q])) return false;
        }
    }
    return true;
}

// KParams::cons_m: every box lies in the root box (nested), so M_i = the root's largest |coordinate| bounds each
// |coordinate| on axis i; 2^-19 M_i rounded up (within 2^-24 relative).
inline void cons_margin(const float* bvh, float cons_m[3]) {
    for (int q = 0; q < 3; q++) {
        const double m = fmax(fabs((double)bvh[q]), fabs((double)bvh[4 + q]));
        cons_m[q] = (float)ldexp(m * (1.0 + 0x1p-20), -19);
    }
}

// The window clause of the culling walk (pt_cull.h): its lemma needs a nested tree, leaf boxes that contain their
// triangles and every triangle inside the conditions window_slack checks.  True with the scene's slack in ws, or
// false (SceneFacts::win_bad) with ws = 0: the walk then runs without the clause.
inline bool window_clause(bool nested, bool leaves_ok, const float* bvh, int n_nodes, const float* tris, float ws[3]) {
    ws[0] = ws[1] = ws[2] = 0.0f;
    return nested && leaves_ok && ptc::window_slack(bvh, n_nodes, tris, ws);
}

}  // namespace ptp
