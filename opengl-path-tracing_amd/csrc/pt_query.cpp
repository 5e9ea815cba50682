// pt_query.cpp -- the ray query on the host (include/pt_api.h: pt_intersect_host, pt_pixel_rays).  Plain host code:
// the scene goes through ptp::pack_scene as an upload's does, and every ray runs ptq::cast (pt_query.h), the per-ray
// code the device kernel runs, on the packed buffers.  The CPU suite (tests/test_query_host.py) checks it against a
// numpy restatement of the reference bit for bit, and the GPU suite checks pt_intersect against this.
// The scene accessor over the packed buffers and the settings checks are pt_host_scene.h's, shared by the four twins.
#include "pt_query.h"

#include "pt_host_scene.h"

#include <cstring>
#include <string>

extern "C" {

int pt_pixel_rays(int width, int height, const float cam[12], const int* xy, long long n, pt_ray* rays_out) {
    if (width <= 0 || height <= 0 || width > 65536 || height > 65536 || !cam || n < 0) return PT_E_ARG;
    if (n > 0 && (!xy || !rays_out)) return PT_E_ARG;
    float basis[12];
    pti::camera_basis(cam, width, height, basis);
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
    const pth::HostScene sc = pth::host_scene(packed);
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
