// trace_host_san.cpp -- TEST INFRASTRUCTURE: pt_trace_host and pt_pixel_seeds under ASan + UBSan (with
// float-cast-overflow), built by tests/test_trace_sanitize.py with csrc/pt_trace.cpp, pt_query.cpp, pt_scene_pack.cpp,
// pt_wide.cpp and pt_scene.cpp -- host code only, a stand-alone program.  Each argument is a scene file in the layout
// of query_host_san.cpp (5 int32 counts: triangles, nodes, materials, spheres, rays; then the std140 float records and
// the 32-byte rays).  Every scene is traced with the file's rays and with rays of random bit patterns in every field,
// under every context flag, display mode and a few bounce limits, overwriting and over a prior of random bit
// patterns; then a node array the packer must reject is offered.
#include "../../include/pt_api.h"

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// pt_scene.cpp (linked for pt_bvh_culling_ok) refers to the GPU builder; this binary is host-only
extern "C" int pt_bvh_build_gpu(const float*, int, float*, int, int*, int) { return PT_E_HIP; }

namespace {

uint32_t g_state = 0x2545f491u;
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

int trace(const Scene& s, const std::vector<float>& nodes, const std::vector<pt_ray>& rays, const unsigned* seeds,
          int flags, int max_bounce, int mode, int frame_first, int n_frames, int acc, std::vector<float>& rgba) {
    return pt_trace_host(s.tris.data(), s.nt, nodes.data(), s.nn, s.mats.data(), s.nm, s.sph.data(), s.ns, flags,
                         max_bounce, mode, rays.data(), seeds, (long long)rays.size(), frame_first, n_frames, acc,
                         rgba.data());
}

}  // namespace

int main(int argc, char** argv) {
    long long traced = 0;
    for (int a = 1; a < argc; a++) {
        Scene s;
        if (!load(argv[a], s)) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        // rays of random bit patterns: every field any binary32, and a share with ordinary origins and directions
        std::vector<pt_ray> wild(300);
        for (size_t i = 0; i < wild.size(); i++) {
            pt_ray& r = wild[i];
            float* w = &r.o[0];
            for (int k = 0; k < 8; k++) w[k] = bits_float(rnd());
            if (i % 3 == 0)
                for (int k = 0; k < 3; k++) r.o[k] = (float)(rnd() % 2001) * 0.005f - 5.0f, r.d[k] = (float)(rnd() % 2001) * 0.001f - 1.0f;
            if (i % 6 == 0) r.t_max = INFINITY;
        }
        const int flags[] = {0, PT_FLAG_NO_SKY, PT_FLAG_NO_SPHERES, PT_FLAG_NO_TRIANGLES, PT_FLAG_MOLLER_TRUMBORE,
                             PT_FLAG_NO_SPHERES | PT_FLAG_MOLLER_TRUMBORE | PT_FLAG_NO_AA};
        const int bounces[] = {0, 1, 8};
        for (const std::vector<pt_ray>* rays : {&s.rays, &wild}) {
            std::vector<unsigned> seeds(rays->size());
            for (unsigned& v : seeds) v = rnd();
            std::vector<float> rgba(4 * rays->size());
            int variant = 0;
            for (int fl : flags)
                for (int mode = 1; mode <= 4; mode++) {
                    const int mb = bounces[variant % 3], acc = variant & 1;
                    if (acc) for (float& v : rgba) v = bits_float(rnd());
                    const int first = variant % 5 == 4 ? INT_MAX - 2 : 1 + variant;
                    if (trace(s, s.nodes, *rays, (variant & 2) ? seeds.data() : nullptr, fl, mb, mode, first, 2, acc, rgba) != PT_OK) {
                        std::fprintf(stderr, "%s: rejected\n", argv[a]);
                        return 1;
                    }
                    if (!acc)       // the alpha of a fresh mean depends on the frame numbers alone
                        for (size_t i = 0; i < rays->size(); i++)
                            if (!(std::fabs(rgba[4 * i + 3] - 1.0f) < 1e-6f)) { std::fprintf(stderr, "%s: alpha of a fresh mean is not 1\n", argv[a]); return 1; }
                    traced += 2 * (long long)rays->size();
                    variant++;
                }
        }
        std::vector<float> rgba(4 * wild.size());
        if (s.nn > 0 && !(s.nodes[8] > -1.0f)) {   // a cycle: the root's miss link back to the root
            std::vector<float> nodes = s.nodes;
            nodes[11] = 0.0f;
            if (trace(s, nodes, wild, nullptr, 0, 5, 1, 1, 1, 0, rgba) != PT_E_SCENE) { std::fprintf(stderr, "%s: cycle accepted\n", argv[a]); return 1; }
        }
        if (trace(s, s.nodes, wild, nullptr, 0, 5, 1, INT_MAX, 1, 0, rgba) != PT_E_ARG) return 1;
        if (trace(s, s.nodes, wild, nullptr, 0, 5, 1, 0, 1, 0, rgba) != PT_E_ARG) return 1;
    }
    // pt_pixel_seeds: pixels of any int
    int xy[64];
    unsigned seeds[32];
    for (int i = 0; i < 100; i++) {
        for (int& v : xy) v = (int)rnd();
        if (pt_pixel_seeds(xy, 32, seeds) != PT_OK) return 1;
    }
    if (pt_pixel_seeds(nullptr, 1, seeds) != PT_E_ARG) return 1;
    std::printf("trace_host_san ok: %lld paths\n", traced);
    return 0;
}
