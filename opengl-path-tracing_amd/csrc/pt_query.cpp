// pt_query.cpp -- the ray query on the host (include/pt_api.h: pt_intersect_host, pt_pixel_rays).  Plain host code:
// the scene goes through ptp::pack_scene as an upload's does, and every ray runs ptq::cast (pt_query.h), the per-ray
// code the device kernel runs, on the packed buffers.  The CPU suite (tests/test_query_host.py) checks it against a
// numpy restatement of the reference bit for bit, and the GPU suite checks pt_intersect against this.
#include "pt_query.h"

#include "pt_scene_pack.h"

#include <cstring>
#include <string>

namespace {

struct HostScene {
    const ptp::Quad* nodes;
    const ptp::Quad* tris;
    const ptp::Quad* spheres;
    const ptp::Quad* leaf;
    int nn, ns;
    bool fast;
    int n_nodes() const { return nn; }
    int n_spheres() const { return ns; }
    bool scene_fast() const { return fast; }
    void node(int i, ptp::Quad& lo, ptp::Quad& hi) const { lo = nodes[2 * (size_t)i], hi = nodes[2 * (size_t)i + 1]; }
    ptp::Quad tri(int slot, int k) const { return tris[4 * (size_t)slot + k]; }
    ptp::Quad sphere(int i, int k) const { return spheres[2 * (size_t)i + k]; }
    ptp::Quad leaf_tris(int pair) const { return leaf[pair]; }
};

const ptp::Quad* quads_of(const ptp::PackedScene& p, int b) { return reinterpret_cast<const ptp::Quad*>(p.buf[b].data()); }

}  // namespace

extern "C" {

int pt_pixel_rays(int width, int height, const float cam[12], const int* xy, long long n, pt_ray* rays_out) {
    if (width <= 0 || height <= 0 || width > 65536 || height > 65536 || !cam || n < 0) return PT_E_ARG;
    if (n > 0 && (!xy || !rays_out)) return PT_E_ARG;
    float basis[12];
    ptq::camera_basis(cam, width, height, basis);
    for (long long i = 0; i < n; i++) ptq::pixel_ray(basis, width, height, xy[2 * i], xy[2 * i + 1], &rays_out[i]);
    return PT_OK;
}

int pt_intersect_host(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                      const float* spheres, int n_spheres, int ctx_flags, const pt_ray* rays, long long n, pt_hit* hits,
                      int query_flags) {
    if (n < 0 || (query_flags & ~PT_QUERY_ANY_HIT) || (ctx_flags & ~PT_FLAG_ALL)) return PT_E_ARG;
    if (n > 0 && (!rays || !hits)) return PT_E_ARG;
    ptp::PackedScene packed;
    std::string err;
    const int rc = ptp::pack_scene(tris, n_tris, bvh, n_nodes, mats, n_mats, spheres, n_spheres, packed, err);
    if (rc) return rc;
    const HostScene sc = {quads_of(packed, ptp::kNodes), quads_of(packed, ptp::kTris), quads_of(packed, ptp::kSpheres),
                          quads_of(packed, ptp::kLeafTris), packed.facts.n_nodes, packed.facts.n_spheres,
                          packed.facts.scene_fast != 0};
    const bool any = (query_flags & PT_QUERY_ANY_HIT) != 0;
    for (long long i = 0; i < n; i++) {
        const pt_ray& r = rays[i];
        const ptq::Hit h = ptq::cast<ptp::Quad>(sc, pt::mk(r.o[0], r.o[1], r.o[2]), pt::mk(r.d[0], r.d[1], r.d[2]),
                                                r.t_max, ctx_flags, any);
        const pt_hit out = {h.t, h.kind, h.prim, h.mat, {h.n.x, h.n.y, h.n.z, 0.0f}, {h.p.x, h.p.y, h.p.z, 0.0f}};
        hits[i] = out;
    }
    return PT_OK;
}

}  // extern "C"
