// pt_scene_pack.cpp -- scene validation and the device layouts as host data (pt_scene_pack.h).
#include "pt_scene_pack.h"

#include "pt_wide.h"
#include "../../include/pt_api.h"
#include "../../include/pt_scene.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

namespace ptp {

using ptl::kPadNodes;

namespace {

int fail(std::string& err, int code, const std::string& msg) {
    err = msg;
    return code;
}

// an int's bits in a float field, and back
float as_float(int v) {
    float f;
    std::memcpy(&f, &v, 4);
    return f;
}
int as_int(float f) {
    int v;
    std::memcpy(&v, &f, 4);
    return v;
}

// A triangle's device record at q[0..3].
void put_tri(Quad* q, const float* t) {
    q[0] = tri_plane(t);                        // the plane test reads this quad alone
    q[1] = {t[0], t[1], t[2], 0.0f};            // .w: the LDS walk's continuation (below)
    q[2] = {t[4], t[5], t[6], as_float((int)t[12])};
    q[3] = {t[8], t[9], t[10], 0.0f};
}

// The threaded BVH: every walk must terminate, leaves have hit == miss, and every index is in range.  Counts the
// leaves into leaf_slot (by reference node index, -1 for an internal node).
int validate(const float* tris, int n_tris, const float* bvh, int n_nodes, int n_mats, const float* spheres,
             int n_spheres, std::vector<int>& leaf_slot, int& n_leaves, std::string& err) {
    leaf_slot.assign(n_nodes, -1);
    n_leaves = 0;
    for (int i = 0; i < n_nodes; i++) {
        const float* nd = bvh + 12 * (size_t)i;
        bool leaf = nd[8] > -1.0f;
        // the shader's int(float) truncates; values outside (-2, n) -- NaN included -- are
        // rejected before any cast (a float-to-int cast out of range is undefined)
        const auto in_open = [](float v, float lo, float hi) { return v > lo && v < hi; };
        if (!in_open(nd[10], -2.0f, (float)n_nodes) || !in_open(nd[11], -2.0f, (float)n_nodes))
            return fail(err, PT_E_SCENE, "BVH link out of range at node " + std::to_string(i));
        int hl = (int)nd[10], ml = (int)nd[11];
        if (leaf) {
            if (!in_open(nd[8], -1.0f, (float)n_tris) || !in_open(nd[9], -1.0f, (float)n_tris))
                return fail(err, PT_E_SCENE, "leaf triangle index out of range at node " + std::to_string(i));
            int t0 = (int)nd[8], t1 = (int)nd[9];
            if (t0 < 0 || t0 >= n_tris || t1 < 0 || t1 >= n_tris)
                return fail(err, PT_E_SCENE, "leaf triangle index out of range at node " + std::to_string(i));
            if (hl != ml) return fail(err, PT_E_SCENE, "leaf with hit link != miss link is unsupported");
            leaf_slot[i] = n_leaves++;
        } else if (hl < 0) {
            return fail(err, PT_E_SCENE, "internal node without a hit link at node " + std::to_string(i));
        }
    }
    // acyclicity of the (hit, miss) link graph reachable from node 0.  The state-machine
    // kernel relies on it: a walk then visits each node at most once, so the reference's
    // steps < numNodes bound (:393) cannot bind and no step counter is kept.
    if (n_nodes > 0) {
        std::vector<unsigned char> color(n_nodes, 0);
        std::vector<std::pair<int, int>> st;
        st.emplace_back(0, 0);
        color[0] = 1;
        while (!st.empty()) {
            auto& top = st.back();
            const float* nd = bvh + 12 * (size_t)top.first;
            if (top.second >= 2) { color[top.first] = 2; st.pop_back(); continue; }
            int nx = (int)nd[10 + top.second];
            top.second++;
            if (nx < 0) continue;
            if (color[nx] == 1) return fail(err, PT_E_SCENE, "BVH links form a cycle");
            if (color[nx] == 0) { color[nx] = 1; st.emplace_back(nx, 0); }
        }
    }
    for (int i = 0; i < n_tris; i++) {
        const float fm = tris[16 * (size_t)i + 12];
        if (!(fm > -1.0f && fm < (float)n_mats)) return fail(err, PT_E_SCENE, "triangle material index out of range");
    }
    for (int i = 0; i < n_spheres; i++) {
        const float fm = spheres[8 * (size_t)i + 4];
        if (!(fm > -1.0f && fm < (float)n_mats)) return fail(err, PT_E_SCENE, "sphere material index out of range");
    }
    return PT_OK;
}

}  // namespace

int check_scene_args(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                     const float* spheres, int n_spheres, std::string& err) {
    if (n_tris < 0 || n_nodes < 0 || n_mats < 0 || n_spheres < 0) return fail(err, PT_E_ARG, "negative count");
    if ((n_tris && !tris) || (n_nodes && !bvh) || (n_mats && !mats) || (n_spheres && !spheres))
        return fail(err, PT_E_ARG, "null array with nonzero count");
    if (n_nodes > (1 << 24) || n_tris > (1 << 24)) return fail(err, PT_E_SCENE, "scene exceeds 2^24 records");
    if (n_mats == 0 && (n_nodes > 0 || n_spheres > 0)) return fail(err, PT_E_SCENE, "no materials");
    return PT_OK;
}

size_t buf_quads(const ptl::SceneFacts& f, int b) {
    const size_t np = (size_t)f.walk_np, ni = f.wide_ok ? (size_t)f.n_wide : 0;
    switch (b) {
    case kNodes: return 2 * (size_t)std::max(f.n_nodes, 1);
    case kTris: return 8 * (size_t)std::max(f.n_slots / 2, 1);
    case kMats: return 3 * (size_t)std::max(f.n_mats, 1);
    case kSpheres: return 2 * (size_t)std::max(f.n_spheres, 1);
    case kWalk: return 16 * np;
    case kWalkSink: return f.walk_nested ? 18 * np : 0;
    case kWideRec: return kWideStride * ni;
    case kWideLeafBox: return 2 * ni;
    case kWideNodes: return ni ? buf_quads(f, kNodes) : 0;
    case kWideTris: return 8 * ni;
    case kSweep: return f.sweep_ok ? 2 * (size_t)f.n_leaves : 0;
    case kLeafTris: return (size_t)std::max(f.n_slots / 2, 1);
    default: return 0;
    }
}

int pack_scene(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
               const float* spheres, int n_spheres, PackedScene& out, std::string& err) {
    int rc = check_scene_args(tris, n_tris, bvh, n_nodes, mats, n_mats, spheres, n_spheres, err);
    if (rc) return rc;
    std::vector<int> leaf_slot;
    int n_leaves = 0;
    rc = validate(tris, n_tris, bvh, n_nodes, n_mats, spheres, n_spheres, leaf_slot, n_leaves, err);
    if (rc) return rc;
    for (auto& b : out.buf) b.clear();
    // buffer b as n zeroed quads
    const auto quads = [&out](int b, size_t n) {
        out.buf[b].assign(4 * n, 0.0f);
        return reinterpret_cast<Quad*>(out.buf[b].data());
    };
    ptl::SceneFacts& sf = out.facts;
    sf = ptl::SceneFacts();

    // --- transpose to device layouts
    const std::vector<int> pos = top_numbering(bvh, n_nodes);
    std::vector<int> slot_of(n_nodes, -1);           // leaf slot by device node index
    std::vector<unsigned char> cop_of(n_nodes, 0);   // coplanar leaf pair, by reference node index
    Quad* const dn = quads(kNodes, 2 * (size_t)std::max(n_nodes, 1));
    Quad* const dt = quads(kTris, 8 * (size_t)std::max(n_leaves, 1));
    Quad* const dlt = quads(kLeafTris, (size_t)std::max(n_leaves, 1));
    for (int i = 0; i < n_nodes; i++) {
        const float* nd = bvh + 12 * (size_t)i;
        int a, b;
        if (leaf_slot[i] >= 0) {
            int s = leaf_slot[i];
            int t0 = (int)nd[8], t1 = (int)nd[9];
            put_tri(&dt[8 * (size_t)s], tris + 16 * (size_t)t0);
            put_tri(&dt[8 * (size_t)s + 4], tris + 16 * (size_t)t1);
            dlt[s] = {as_float(t0), as_float(t1), 0.0f, 0.0f};
            const bool cop = same_plane(dt[8 * (size_t)s], dt[8 * (size_t)s + 4]);
            a = ~((s << 2) | (cop ? 2 : 0) | (t0 == t1 ? 1 : 0));
            cop_of[i] = cop ? 1 : 0;
            b = (int)nd[11];
            slot_of[pos[i]] = s;
        } else {
            a = pos[(int)nd[10]];
            b = (int)nd[11];
        }
        if (b >= 0) b = pos[b];
        // axis-paired: (min, max) of one axis in adjacent registers for packed-f32 slabs
        const size_t j = (size_t)pos[i];
        dn[2 * j] = {nd[0], nd[4], nd[1], nd[5]};
        dn[2 * j + 1] = {nd[2], nd[6], as_float(a), as_float(b)};
    }
    Quad* const dm = quads(kMats, 3 * (size_t)std::max(n_mats, 1));
    for (int i = 0; i < n_mats; i++) {
        const float* m = mats + 16 * (size_t)i;
        float s = m[12];
        dm[3 * (size_t)i] = {m[0], m[1], m[2], m[13]};
        dm[3 * (size_t)i + 1] = {m[4] * s, m[5] * s, m[6] * s, m[14]};
        dm[3 * (size_t)i + 2] = {m[8], m[9], m[10], 0.0f};
    }
    Quad* const ds = quads(kSpheres, 2 * (size_t)std::max(n_spheres, 1));
    for (int i = 0; i < n_spheres; i++) {
        const float* s = spheres + 8 * (size_t)i;
        ds[2 * (size_t)i] = {s[0], s[1], s[2], s[3] * s[3]};
        ds[2 * (size_t)i + 1] = {as_float((int)s[4]), 0, 0, 0};
    }
    // LDS walk images of the state-machine kernel (WalkLinks in the kernel source): per ray
    // octant k the node planes (bounds of the axes whose bit is set in k swapped) with links
    // as byte offsets (16 * (2N * k + index)) and a leaf's hit link -2 - code; the leaf's
    // next-right (image-0 offset) goes to its first triangle's quad 1 .w
    const size_t N = (size_t)(n_nodes <= kPadNodes ? kPadNodes : n_nodes);   // nodes per image plane
    Quad* const dwl = quads(kWalk, 16 * N);
    for (int k = 0; k < 8; k++) {
        const int base = 16 * 2 * (int)N * k;
        for (int i = 0; i < n_nodes; i++) {
            Quad lo = dn[2 * (size_t)i], hi = dn[2 * (size_t)i + 1];
            const int a = as_int(hi.z), b = as_int(hi.w);
            const bool leaf = a < 0;
            const int ha = leaf ? -2 - ~a : base + 16 * a, hb = b >= 0 ? base + 16 * b : -1;
            hi.z = as_float(ha);
            hi.w = as_float(hb);
            if (k & 1) std::swap(lo.x, lo.y);
            if (k & 2) std::swap(lo.z, lo.w);
            if (k & 4) std::swap(hi.x, hi.y);
            dwl[2 * N * k + i] = lo;
            dwl[2 * N * k + N + i] = hi;
            if (leaf && k == 0) {
                dt[8 * (size_t)slot_of[i] + 1].w = as_float(hb);
                dt[8 * (size_t)slot_of[i] + 7].w = as_float(16 * i);   // the culling walk's exact leaf re-test
            }
        }
    }
    // The culling walk's copy of the walk images: the 8 octant images plus a
    // ninth of "sinks" -- node records whose links both point to themselves.  A leaf's hit link
    // leads to its sink (index 1 + k for leaf pair k) and the chain's end (-1) to sink 0, so a
    // lane that stopped keeps stepping in place: the walk step needs no exec mask, and a lane
    // walks while its position lies below the sink image.  A leaf's coplanar flag moves to
    // slot 2k+1 quad 1 .w (the sink index carries only k).
    const bool nested = pt_bvh_culling_ok(bvh, n_nodes) == 1;   // pt_scene.cpp
    if (nested) {
        out.buf[kWalkSink].reserve(4 * 18 * N);
        out.buf[kWalkSink] = out.buf[kWalk];
        out.buf[kWalkSink].resize(4 * 18 * N, 0.0f);
        Quad* const dsk = reinterpret_cast<Quad*>(out.buf[kWalkSink].data());
        const int sink0 = 16 * 2 * (int)N * 8;
        for (int k = 0; k < 8; k++) {
            for (int i = 0; i < n_nodes; i++) {
                Quad& hi = dsk[2 * N * k + N + i];
                int a = as_int(hi.z), b = as_int(hi.w);
                if (a <= -2) a = sink0 + 16 * (1 + ((-2 - a) >> 2));
                if (b == -1) b = sink0;
                hi.z = as_float(a);
                hi.w = as_float(b);
            }
        }
        for (int i = 0; i <= n_leaves; i++) {
            const float self = as_float(sink0 + 16 * i);
            dsk[16 * N + N + i] = {0, 0, self, self};
        }
        for (int i = 0; i < n_nodes; i++)
            if (leaf_slot[i] >= 0) dt[8 * (size_t)leaf_slot[i] + 5].w = as_float((int)cop_of[i]);
    }
    // The wide tree of the global-memory walk (pt_wide.h): nested trees only
    // (the superset argument), built whatever the scene size -- variant 3 sends any scene to
    // the global walk.  Its index g numbers records and leaves; leaf g's triangles go to slots
    // 2g, 2g + 1 of a second triangle array and its exact box to wlbox[2g], and a second copy
    // of the device nodes carries leaf codes g << 2 | coplanar << 1 | single for the binary
    // walk of the lanes outside the guard.
    ptw::WideTree wt;
    const bool wide = nested && ptw::wide_build(bvh, n_nodes, cop_of.data(), wt) == 0;
    if (wide) {
        const size_t nr = (size_t)wt.n_index;
        out.buf[kWideNodes] = out.buf[kNodes];
        Quad* const dnw = reinterpret_cast<Quad*>(out.buf[kWideNodes].data());
        Quad* const dtw = quads(kWideTris, 8 * nr);
        for (int i = 0; i < n_nodes; i++) {
            const float* nd = bvh + 12 * (size_t)i;
            if (leaf_slot[i] < 0) continue;
            const int g = wt.g_of[i], t0 = (int)nd[8], t1 = (int)nd[9];
            // a leaf no walk reaches (not in the nested tree from the root, which is all the
            // links of reachable nodes lead to) has no index: nothing to place
            if (g < 0) continue;
            dnw[2 * (size_t)pos[i] + 1].z = as_float(~((g << 2) | (cop_of[i] ? 2 : 0) | (t0 == t1 ? 1 : 0)));
            put_tri(&dtw[8 * (size_t)g], tris + 16 * (size_t)t0);
            put_tri(&dtw[8 * (size_t)g + 4], tris + 16 * (size_t)t1);
        }
        // the builder's leaf boxes as they are, and the kWideStride used quads of each of its 64-B records
        out.buf[kWideLeafBox] = std::move(wt.lbox);
        if (kWideStride == ptw::kRecQuads) {
            out.buf[kWideRec] = std::move(wt.rec);
        } else {
            out.buf[kWideRec].resize(nr * kWideStride * 4);
            for (size_t i = 0; i < nr; i++)
                std::memcpy(&out.buf[kWideRec][i * kWideStride * 4], &wt.rec[i * 16], kWideStride * sizeof(Quad));
        }
        sf.n_wide = wt.n_index;
        std::memcpy(sf.wide_cw, wt.cw, sizeof(sf.wide_cw));
    }

    // --- the scene's facts (the launch planner's input)
    sf.n_nodes = n_nodes;
    sf.n_spheres = n_spheres;
    sf.n_mats = n_mats;
    sf.n_slots = 2 * n_leaves;
    sf.n_top = std::min(n_nodes, kTopNodes);
    // exact-reciprocal slab guard, scene half: every box coordinate is 0
    // or has magnitude in [2^-40, 2^60], and min <= max on every axis (the octant images'
    // near-first order, slab_oct)
    sf.scene_fast = 1;
    for (int i = 0; i < n_nodes && sf.scene_fast; i++) {
        const float* nd = bvh + 12 * (size_t)i;
        for (int q = 0; q < 7; q++) {
            if (q == 3) continue;
            float a = std::fabs(nd[q]);
            if (!(nd[q] == 0.0f || (a >= 0x1p-40f && a <= 0x1p60f))) { sf.scene_fast = 0; break; }
        }
        if (!(nd[0] <= nd[4] && nd[1] <= nd[5] && nd[2] <= nd[6])) sf.scene_fast = 0;
    }
    sf.walk_nested = nested;
    sf.wide_ok = wide;
    sf.leaf_cert_ok = leaves_contain_tris(bvh, n_nodes, tris);
    sf.win_bad = !window_clause(nested, sf.leaf_cert_ok, bvh, n_nodes, tris, sf.win_slack);
    if (n_nodes > 0) cons_margin(bvh, sf.cons_m);
    sf.walk_np = (int)N;
    sf.lds_bytes = (size_t)(16 * N + 4 * sf.n_slots + 3 * n_mats + 2 * n_spheres) * sizeof(Quad);
    sf.lds_bytes_sk = sf.lds_bytes + 2 * N * sizeof(Quad);
    sf.root_child = -1;
    if (n_nodes > 0) {
        const Quad r0 = dn[0], r1 = dn[1];
        const float box[6] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y};
        std::memcpy(sf.root_box, box, sizeof(box));
        const int a = as_int(r1.z);
        sf.root_child = a >= 0 ? a : -1;
    }
    // The leaf sweep's table (pt_cull.h, sweep_mask; DESIGN.md §5.6, "The leaf sweep"): the leaves in chain order -- an internal node
    // leads to its hit link, a leaf to its miss link, which in a nested tree passes every node in preorder -- each
    // with its own box in the reference order and its triangle-pair index, and beside them the inverse map (entry p's
    // last word: the chain position of pair p).  A lane's candidates are the bits of one word, bit k = chain position
    // k, so the scene qualifies only when it has at most kSweepMaxLeaves leaves and the chain reaches all of them.  Its
    // test is the culling walk's with the window clause, on exact quotients: the nested tree, the clause's conditions
    // and the scene half of the guard as there.
    sf.n_leaves = n_leaves;
    sf.sweep_ok = false;
    if (nested && !sf.win_bad && sf.scene_fast && n_leaves >= 1 && n_leaves <= ptl::kSweepMaxLeaves) {
        std::vector<int> chain;
        for (int i = 0; i >= 0 && (int)chain.size() <= n_leaves;) {
            const float* nd = bvh + 12 * (size_t)i;
            if (leaf_slot[i] >= 0) chain.push_back(i);
            i = (int)nd[leaf_slot[i] >= 0 ? 11 : 10];
        }
        if ((int)chain.size() == n_leaves) {   // (an orphan leaf, which no walk reaches, has no position)
            Quad* const dsw = quads(kSweep, 2 * (size_t)n_leaves);
            for (int k = 0; k < n_leaves; k++) {
                const float* nd = bvh + 12 * (size_t)chain[k];
                const int pair = leaf_slot[chain[k]];
                dsw[2 * k] = {nd[0], nd[4], nd[1], nd[5]};
                dsw[2 * k + 1].x = nd[2];
                dsw[2 * k + 1].y = nd[6];
                dsw[2 * k + 1].z = as_float(pair);
                dsw[2 * pair + 1].w = as_float(k);
            }
            sf.sweep_ok = true;
        }
    }
    for (int b = 0; b < kBufsAll; b++)
        if (out.buf[b].size() != 4 * buf_quads(sf, b))
            return fail(err, PT_E_SCENE, "internal: scene buffer " + std::to_string(b) + " has not the size of its facts");
    return PT_OK;
}

}  // namespace ptp
