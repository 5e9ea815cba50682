// camera_host_san.cpp -- TEST INFRASTRUCTURE: pt_trace_camera_host and pt_camera_rays_host under ASan + UBSan (with
// float-cast-overflow), built by tests/test_camera_sanitize.py with csrc/pt_camera.cpp, pt_trace.cpp, pt_query.cpp,
// pt_scene_pack.cpp, pt_wide.cpp and pt_scene.cpp -- host code only, a stand-alone program.  Each argument is a scene
// file in the layout of query_host_san.cpp (5 int32 counts: triangles, nodes, materials, spheres, rays; then the std140
// float records and the 32-byte rays, which this program skips).  Every scene is traced through the four models, with
// and without anti-aliasing, overwriting and over a prior of random bit patterns; then through cameras whose every
// field is a random bit pattern (an accepted one must trace, a rejected one must return PT_E_ARG); then at the sizes
// 1 x 1 and 1 x 65536; and rays are made for pixel lists in no order.
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
        s.sph.resize(8 * (size_t)c[3]);
        ok = std::fread(s.tris.data(), 4, s.tris.size(), f) == s.tris.size() &&
             std::fread(s.nodes.data(), 4, s.nodes.size(), f) == s.nodes.size() &&
             std::fread(s.mats.data(), 4, s.mats.size(), f) == s.mats.size() &&
             std::fread(s.sph.data(), 4, s.sph.size(), f) == s.sph.size();
    }
    std::fclose(f);
    return ok;
}

int trace(const Scene& s, const pt_camera& c, int flags, int max_bounce, int mode, int frame_first, int n_frames, int acc,
          std::vector<float>& rgba) {
    return pt_trace_camera_host(s.tris.data(), s.nt, s.nodes.data(), s.nn, s.mats.data(), s.nm, s.sph.data(), s.ns, flags,
                                max_bounce, mode, &c, frame_first, n_frames, acc, rgba.data());
}

pt_camera camera(int model, int w, int h, int flags) {
    pt_camera c = {model, w, h, flags, {0.3f, -6.0f, 1.0f, 0.0f, 0.1f, 1.0f, -0.05f, 0.0f, 0, 0, 0, 0}, 0.1f, 5.0f, 6.0f, 0.0f};
    return c;
}

// what the header promises to reject, restated
bool must_reject(const pt_camera& c) {
    if (c.model < 0 || c.model > 3 || (c.flags & ~PT_CAM_NO_AA)) return true;
    if (c.width < 1 || c.width > 65536 || c.height < 1 || c.height > 65536) return true;
    if (c.model == PT_CAM_THIN_LENS && (std::isnan(c.aperture) || c.aperture < 0.0f || std::isnan(c.focus) || !(c.focus > 0.0f))) return true;
    if (c.model == PT_CAM_ORTHO && (std::isnan(c.ortho_width) || !(c.ortho_width > 0.0f))) return true;
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    long long traced = 0, accepted = 0, rejected = 0;
    for (int a = 1; a < argc; a++) {
        Scene s;
        if (!load(argv[a], s)) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        const int ctx_flags[] = {0, PT_FLAG_NO_SKY, PT_FLAG_MOLLER_TRUMBORE, PT_FLAG_NO_SPHERES | PT_FLAG_NO_AA};
        const int bounces[] = {0, 1, 8};
        int variant = 0;
        for (int model = 0; model < 4; model++)
            for (int cf = 0; cf < 2; cf++) {
                const pt_camera c = camera(model, 9, 7, cf);
                std::vector<float> rgba(4 * 9 * 7);
                for (int mode = 1; mode <= 4; mode++) {
                    const int acc = variant & 1, first = variant % 5 == 4 ? INT_MAX - 2 : 1 + variant;
                    if (acc) for (float& v : rgba) v = bits_float(rnd());
                    if (trace(s, c, ctx_flags[variant % 4], bounces[variant % 3], mode, first, 2, acc, rgba) != PT_OK) {
                        std::fprintf(stderr, "%s: model %d rejected\n", argv[a], model);
                        return 1;
                    }
                    if (!acc)       // the alpha of a fresh mean depends on the frame numbers alone
                        for (size_t i = 0; i < rgba.size() / 4; i++)
                            if (!(std::fabs(rgba[4 * i + 3] - 1.0f) < 1e-6f)) { std::fprintf(stderr, "%s: alpha of a fresh mean is not 1\n", argv[a]); return 1; }
                    traced += 2 * 9 * 7;
                    variant++;
                }
            }
        // cameras of arbitrary bit patterns: the model, the flag and the size from small ranges often enough to be accepted
        for (int k = 0; k < 400; k++) {
            pt_camera c;
            uint32_t w[sizeof(pt_camera) / 4];
            for (uint32_t& v : w) v = rnd();
            std::memcpy(&c, w, sizeof(c));
            if (k % 4 != 3) c.model = (int)(rnd() % 5), c.flags = (int)(rnd() % 3), c.width = (int)(rnd() % 7), c.height = (int)(rnd() % 6);
            if (k % 8 < 2) for (int j = 0; j < 12; j++) c.cam[j] = (float)(rnd() % 2001) * 0.005f - 5.0f;
            if (k % 8 == 0) c.aperture = 0.25f, c.focus = 3.0f, c.ortho_width = 5.0f;
            if (k % 4 == 3 && !must_reject(c)) c.width = c.width % 7 + 1, c.height = c.height % 6 + 1;   // keep an accepted one small
            std::vector<float> rgba(must_reject(c) ? 4 : 4 * (size_t)c.width * (size_t)c.height);
            const int rc = trace(s, c, 0, 3, 1, 1 + k, 2, 0, rgba);
            if (must_reject(c) ? rc != PT_E_ARG : rc != PT_OK) { std::fprintf(stderr, "%s: camera %d: rc %d\n", argv[a], k, rc); return 1; }
            (rc == PT_OK ? accepted : rejected)++;
            int xy[8];
            pt_ray rays[4];
            unsigned states[4];
            bool inside = true;
            for (int j = 0; j < 4; j++) {                 // pixels of any int: outside the image they are refused
                xy[2 * j] = (int)rnd(), xy[2 * j + 1] = (int)rnd();
                inside = inside && xy[2 * j] >= 0 && xy[2 * j] < c.width && xy[2 * j + 1] >= 0 && xy[2 * j + 1] < c.height;
            }
            if (pt_camera_rays_host(&c, xy, 4, 1 + k, rays, states) != (must_reject(c) || !inside ? PT_E_ARG : PT_OK)) {
                std::fprintf(stderr, "%s: camera %d: a pixel of any int\n", argv[a], k);
                return 1;
            }
            if (!must_reject(c))
                for (int j = 0; j < 4; j++) xy[2 * j] = (int)(rnd() % (unsigned)c.width), xy[2 * j + 1] = (int)(rnd() % (unsigned)c.height);
            const int rr = pt_camera_rays_host(&c, xy, 4, 1 + k, rays, (k & 1) ? states : nullptr);
            if (must_reject(c) ? rr != PT_E_ARG : rr != PT_OK) { std::fprintf(stderr, "%s: camera %d: rays rc %d\n", argv[a], k, rr); return 1; }
        }
        // the smallest image and the tallest column
        for (int model = 0; model < 4; model++) {
            std::vector<float> one(4), column(4 * 65536);
            if (trace(s, camera(model, 1, 1, 0), 0, 8, 1, 1, 3, 0, one) != PT_OK) return 1;
            if (a == 1 && trace(s, camera(model, 1, 65536, model & 1), 0, 1, 1, 1, 1, 0, column) != PT_OK) return 1;
            traced += 3 + (a == 1 ? 65536 : 0);
        }
        std::vector<float> rgba(4);
        if (trace(s, camera(0, 1, 1, 0), 0, 5, 1, INT_MAX, 1, 0, rgba) != PT_E_ARG) return 1;
        if (trace(s, camera(0, 1, 1, 0), 0, 5, 1, 0, 1, 0, rgba) != PT_E_ARG) return 1;
        if (s.nn > 0 && !(s.nodes[8] > -1.0f)) {   // a cycle: the root's miss link back to the root
            Scene bad = s;
            bad.nodes[11] = 0.0f;
            if (trace(bad, camera(1, 1, 1, 0), 0, 5, 1, 1, 1, 0, rgba) != PT_E_SCENE) { std::fprintf(stderr, "%s: cycle accepted\n", argv[a]); return 1; }
        }
    }
    // rays for pixel lists in no order: backwards, repeated, and scattered over a 65536 x 65536 image
    for (int model = 0; model < 4; model++) {
        const pt_camera c = camera(model, 65536, 65536, model & 1);
        std::vector<int> xy;
        for (int i = 0; i < 500; i++) xy.push_back((int)(rnd() % 65536)), xy.push_back((int)(rnd() % 65536));
        for (int i = 99; i >= 0; i--) xy.push_back(i), xy.push_back(65535 - i);
        for (int i = 0; i < 20; i++) xy.push_back(65535), xy.push_back(65535);
        const long long n = (long long)xy.size() / 2;
        std::vector<pt_ray> rays((size_t)n);
        std::vector<unsigned> states((size_t)n);
        for (int frame : {1, 2986, INT_MAX - 1})
            if (pt_camera_rays_host(&c, xy.data(), n, frame, rays.data(), states.data()) != PT_OK) return 1;
        if (pt_camera_rays_host(&c, xy.data(), n, 0, rays.data(), states.data()) != PT_E_ARG) return 1;
        if (pt_camera_rays_host(nullptr, xy.data(), n, 1, rays.data(), states.data()) != PT_E_ARG) return 1;
    }
    if (accepted < 50 || rejected < 50) { std::fprintf(stderr, "the random cameras are one-sided: %lld accepted, %lld rejected\n", accepted, rejected); return 1; }
    std::printf("camera_host_san ok: %lld paths, %lld random cameras accepted, %lld rejected\n", traced, accepted, rejected);
    return 0;
}
