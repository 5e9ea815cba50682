// query_host_san.cpp -- TEST INFRASTRUCTURE: pt_intersect_host and pt_pixel_rays under ASan + UBSan (with
// float-cast-overflow), built by tests/test_query_sanitize.py with csrc/pt_query.cpp, pt_scene_pack.cpp, pt_wide.cpp
// and pt_scene.cpp -- host code only, a stand-alone program.  Each argument is a scene file the test wrote
// (5 int32 counts: triangles, nodes, materials, spheres, rays; then the std140 float records and the 32-byte rays).
// Every scene is cast with the file's rays (the families of tests/query_cases.py) and with rays of random bit
// patterns in every field, closest and any-hit, under every context flag; then node arrays the packer must reject
// are offered, which must come back with its error and without a read outside the arrays.
#include "../../include/pt_api.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// pt_scene.cpp (linked for pt_bvh_culling_ok) refers to the GPU builder; this binary is host-only
extern "C" int pt_bvh_build_gpu(const float*, int, float*, int, int*, int) { return PT_E_HIP; }

namespace {

uint32_t g_state = 0x9e3779b9u;
uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 17;
    g_state ^= g_state << 5;
    return g_state;
}
float bits_float(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

struct Scene {
    std::vector<float> tris, nodes, mats, sph;
    std::vector<pt_ray> rays;
    int nt = 0, nn = 0, nm = 0, ns = 0;
};

bool load(const char* path, Scene& s) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t c[5];
    bool ok = std::fread(c, 4, 5, f) == 5;
    if (ok) {
        s.nt = c[0], s.nn = c[1], s.nm = c[2], s.ns = c[3];
        s.tris.resize(16 * (size_t)c[0]), s.nodes.resize(12 * (size_t)c[1]), s.mats.resize(16 * (size_t)c[2]);
        s.sph.resize(8 * (size_t)c[3]), s.rays.resize((size_t)c[4]);
        ok = std::fread(s.tris.data(), 4, s.tris.size(), f) == s.tris.size() &&
             std::fread(s.nodes.data(), 4, s.nodes.size(), f) == s.nodes.size() &&
             std::fread(s.mats.data(), 4, s.mats.size(), f) == s.mats.size() &&
             std::fread(s.sph.data(), 4, s.sph.size(), f) == s.sph.size() &&
             std::fread(s.rays.data(), sizeof(pt_ray), s.rays.size(), f) == s.rays.size();
    }
    std::fclose(f);
    return ok;
}

int cast(const Scene& s, const std::vector<float>& nodes, const std::vector<pt_ray>& rays, int flags, int qflags,
         std::vector<pt_hit>& hits) {
    hits.resize(rays.size());
    return pt_intersect_host(s.tris.data(), s.nt, nodes.data(), s.nn, s.mats.data(), s.nm, s.sph.data(), s.ns, flags,
                             rays.data(), (long long)rays.size(), hits.data(), qflags);
}

// a hit record is well formed: its indices lie in the scene
bool well_formed(const Scene& s, const pt_hit& h) {
    if (h.kind == PT_HIT_NONE) return h.prim == -1 && h.mat == -1 && std::isinf(h.t) && h.t > 0;
    if (h.mat < 0 || h.mat >= s.nm) return false;
    if (h.kind == PT_HIT_SPHERE) return h.prim >= 0 && h.prim < s.ns;
    return h.kind == PT_HIT_TRIANGLE && h.prim >= 0 && h.prim < s.nt;
}

}  // namespace

int main(int argc, char** argv) {
    long long casts = 0, rejected = 0;
    for (int a = 1; a < argc; a++) {
        Scene s;
        if (!load(argv[a], s)) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        // rays of random bit patterns: every field any binary32 (NaNs, infinities, subnormals, both zeros), and a
        // share with ordinary origins and directions so that walks go deep
        std::vector<pt_ray> wild(600);
        for (size_t i = 0; i < wild.size(); i++) {
            pt_ray& r = wild[i];
            float* w = &r.o[0];
            for (int k = 0; k < 8; k++) w[k] = bits_float(rnd());
            if (i % 3 == 0)
                for (int k = 0; k < 3; k++) r.o[k] = (float)(rnd() % 2001) * 0.005f - 5.0f, r.d[k] = (float)(rnd() % 2001) * 0.001f - 1.0f;
            if (i % 6 == 0) r.t_max = INFINITY;
        }
        std::vector<pt_hit> hits;
        const int flags[] = {0, PT_FLAG_NO_SPHERES, PT_FLAG_NO_TRIANGLES, PT_FLAG_MOLLER_TRUMBORE,
                             PT_FLAG_NO_SPHERES | PT_FLAG_MOLLER_TRUMBORE};
        for (int fl : flags)
            for (int q = 0; q < 2; q++)
                for (const std::vector<pt_ray>* rays : {&s.rays, &wild}) {
                    if (cast(s, s.nodes, *rays, fl, q, hits) != PT_OK) { std::fprintf(stderr, "%s: rejected\n", argv[a]); return 1; }
                    for (const pt_hit& h : hits)
                        if (!well_formed(s, h)) { std::fprintf(stderr, "%s: malformed hit record\n", argv[a]); return 1; }
                    casts += (long long)rays->size();
                }
        // node arrays the packer must reject (PT_E_SCENE), each from the good one
        if (s.nn > 0) {
            const float bad_links[] = {NAN, INFINITY, -INFINITY, (float)s.nn, -2.0f, 3.0e9f, -3.0e9f};
            for (float v : bad_links)
                for (int field = 10; field < 12; field++) {
                    std::vector<float> nodes = s.nodes;
                    nodes[12 * (size_t)(rnd() % (uint32_t)s.nn) + field] = v;
                    const int rc = cast(s, nodes, wild, 0, 0, hits);
                    // (-2 in the hit link of a leaf is its miss link's partner: hit != miss, rejected too)
                    if (rc != PT_E_SCENE) { std::fprintf(stderr, "%s: link %g accepted (%d)\n", argv[a], v, rc); return 1; }
                    rejected++;
                }
            const float bad_tris[] = {NAN, INFINITY, (float)s.nt, 3.0e9f};
            for (float v : bad_tris) {
                std::vector<float> nodes = s.nodes;
                int leaf = 0;
                while (leaf < s.nn && !(nodes[12 * (size_t)leaf + 8] > -1.0f)) leaf++;
                if (leaf == s.nn) break;
                nodes[12 * (size_t)leaf + 9] = v;
                const int rc = cast(s, nodes, wild, 0, 0, hits);
                if (rc != PT_E_SCENE) { std::fprintf(stderr, "%s: leaf index %g accepted (%d)\n", argv[a], v, rc); return 1; }
                rejected++;
            }
            {   // a cycle: the root's miss link back to the root
                std::vector<float> nodes = s.nodes;
                nodes[11] = 0.0f;
                if (!(nodes[8] > -1.0f)) {
                    if (cast(s, nodes, wild, 0, 0, hits) != PT_E_SCENE) { std::fprintf(stderr, "%s: cycle accepted\n", argv[a]); return 1; }
                    rejected++;
                }
            }
        }
        if (pt_intersect_host(s.tris.data(), -1, s.nodes.data(), s.nn, s.mats.data(), s.nm, s.sph.data(), s.ns, 0,
                              wild.data(), 1, hits.data(), 0) != PT_E_ARG) return 1;
        if (pt_intersect_host(s.tris.data(), s.nt, s.nodes.data(), s.nn, s.mats.data(), s.nm, s.sph.data(), s.ns, 0,
                              nullptr, 1, hits.data(), 0) != PT_E_ARG) return 1;
    }
    // pt_pixel_rays: cameras of random bit patterns, pixels of any int
    for (int i = 0; i < 200; i++) {
        float cam[12];
        for (float& c : cam) c = i % 2 ? bits_float(rnd()) : (float)(rnd() % 2001) * 0.01f - 10.0f;
        int xy[16];
        for (int& v : xy) v = (int)rnd();
        pt_ray rays[8];
        if (pt_pixel_rays(1 + (int)(rnd() % 65536u), 1 + (int)(rnd() % 65536u), cam, xy, 8, rays) != PT_OK) return 1;
    }
    if (pt_pixel_rays(0, 1, nullptr, nullptr, 0, nullptr) != PT_E_ARG) return 1;
    std::printf("query_host_san ok: %lld casts, %lld rejected node arrays\n", casts, rejected);
    return 0;
}
