// film_host_san.cpp -- TEST INFRASTRUCTURE: pt_film_expose_host under ASan + UBSan (with float-cast-overflow), built by
// tests/test_film_sanitize.py with csrc/pt_film.cpp, pt_query.cpp, pt_scene_pack.cpp, pt_wide.cpp and pt_scene.cpp --
// host code only, a stand-alone program.  Each argument is a scene file in the layout of query_host_san.cpp (5 int32
// counts: triangles, nodes, materials, spheres, rays; then the std140 float records and the 32-byte rays, which this
// program skips).  Every scene is exposed through the four models, restarting and over priors of random bit patterns
// in all three planes, with guide_frames below, inside and above the frame range and every guides_held it allows; then
// through cameras whose every field is a random bit pattern (an accepted one must expose, a rejected one must return
// PT_E_ARG); then at the sizes 1 x 1 and 1 x 65536.
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

// The three planes of a film of w x h pixels, each allocated to its exact size so that ASan sees every overrun.
struct Planes {
    std::vector<float> rgba, mom, gd;
    Planes(size_t px, bool random) : rgba(4 * px), mom(2 * px), gd(8 * px) {
        if (random)
            for (std::vector<float>* v : {&rgba, &mom, &gd})
                for (float& x : *v) x = bits_float(rnd());
    }
};

int expose(const Scene& s, const pt_camera& c, int flags, int max_bounce, int mode, int guide_frames, int frame_first,
           int n_frames, int acc, int frames_before, int held, Planes& p, int* held_out) {
    return pt_film_expose_host(s.tris.data(), s.nt, s.nodes.data(), s.nn, s.mats.data(), s.nm, s.sph.data(), s.ns, flags,
                               max_bounce, mode, &c, guide_frames, frame_first, n_frames, acc, frames_before, held,
                               p.rgba.data(), p.mom.data(), p.gd.data(), held_out);
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

// guides_held after an exposure, by the header's rule
int held_rule(int first, int n, int held, int G) {
    const long long last = (long long)first + n - 1;
    if (held < G && first <= held + 1 && last >= held + 1) return (int)(last < G ? last : G);
    return held;
}

}  // namespace

int main(int argc, char** argv) {
    long long paths = 0, accepted = 0, rejected = 0;
    for (int a = 1; a < argc; a++) {
        Scene s;
        if (!load(argv[a], s)) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        const int ctx_flags[] = {0, PT_FLAG_NO_SKY, PT_FLAG_MOLLER_TRUMBORE, PT_FLAG_NO_SPHERES | PT_FLAG_NO_AA};
        const int bounces[] = {0, 1, 8};
        int variant = 0;
        for (int model = 0; model < 4; model++)
            for (int cf = 0; cf < 2; cf++) {
                const pt_camera c = camera(model, 9, 7, cf);
                // frames first .. first + 2 against guide_frames 1 (below a range that starts later), 2, 4 and 9 (above)
                for (int G : {1, 2, 4, 9})
                    for (int held = 0; held <= G; held += (G > 4 ? 4 : 1)) {
                        const int acc = variant & 1, mode = 1 + variant % 4;
                        const int first = variant % 7 == 6 ? INT_MAX - 3 : 1 + variant % 5;
                        Planes p(9 * 7, true);
                        const std::vector<float> gd_before = p.gd;
                        int out = -1;
                        if (expose(s, c, ctx_flags[variant % 4], bounces[variant % 3], mode, G, first, 3, acc, variant % 11, held, p, &out) != PT_OK) {
                            std::fprintf(stderr, "%s: model %d G %d held %d rejected\n", argv[a], model, G, held);
                            return 1;
                        }
                        const int want = held_rule(first, 3, held, G);
                        if (out != want) { std::fprintf(stderr, "%s: guides_held %d, want %d\n", argv[a], out, want); return 1; }
                        if (want == held && std::memcmp(gd_before.data(), p.gd.data(), 4 * gd_before.size()) != 0) {
                            std::fprintf(stderr, "%s: guides written without a guide frame\n", argv[a]);
                            return 1;
                        }
                        if (!acc)       // the alpha of a fresh mean depends on the frame numbers alone
                            for (size_t i = 0; i < p.rgba.size() / 4; i++)
                                if (!(std::fabs(p.rgba[4 * i + 3] - 1.0f) < 1e-6f)) { std::fprintf(stderr, "%s: alpha of a fresh mean is not 1\n", argv[a]); return 1; }
                        paths += 3 * 9 * 7;
                        variant++;
                    }
            }
        // cameras of arbitrary bit patterns: the model, the flag and the size from small ranges often enough to be accepted
        for (int k = 0; k < 300; k++) {
            pt_camera c;
            uint32_t w[sizeof(pt_camera) / 4];
            for (uint32_t& v : w) v = rnd();
            std::memcpy(&c, w, sizeof(c));
            if (k % 4 != 3) c.model = (int)(rnd() % 5), c.flags = (int)(rnd() % 3), c.width = (int)(rnd() % 7), c.height = (int)(rnd() % 6);
            if (k % 8 < 2) for (int j = 0; j < 12; j++) c.cam[j] = (float)(rnd() % 2001) * 0.005f - 5.0f;
            if (k % 8 == 0) c.aperture = 0.25f, c.focus = 3.0f, c.ortho_width = 5.0f;
            if (k % 4 == 3 && !must_reject(c)) c.width = c.width % 7 + 1, c.height = c.height % 6 + 1;   // keep an accepted one small
            Planes p(must_reject(c) ? 1 : (size_t)c.width * (size_t)c.height, true);
            const int G = 1 + (int)(rnd() % 4), held = (int)(rnd() % (unsigned)(G + 1));
            const int rc = expose(s, c, 0, 3, 1, G, 1 + k % 3, 2, k & 1, k, held, p, nullptr);
            if (must_reject(c) ? rc != PT_E_ARG : rc != PT_OK) { std::fprintf(stderr, "%s: camera %d: rc %d\n", argv[a], k, rc); return 1; }
            (rc == PT_OK ? accepted : rejected)++;
        }
        // the smallest image and the tallest column
        for (int model = 0; model < 4; model++) {
            Planes one(1, false), column(65536, false);
            int out = -1;
            if (expose(s, camera(model, 1, 1, 0), 0, 8, 1, 2, 1, 3, 0, 0, 0, one, &out) != PT_OK || out != 2) return 1;
            if (a == 1 && (expose(s, camera(model, 1, 65536, model & 1), 0, 1, 1, 3, 1, 1, 0, 0, 0, column, &out) != PT_OK || out != 1)) return 1;
            paths += 3 + (a == 1 ? 65536 : 0);
        }
        Planes p(1, false);
        const pt_camera c = camera(0, 1, 1, 0);
        if (expose(s, c, 0, 5, 1, 2, INT_MAX, 1, 0, 0, 0, p, nullptr) != PT_E_ARG) return 1;      // frame range
        if (expose(s, c, 0, 5, 1, 2, 0, 1, 0, 0, 0, p, nullptr) != PT_E_ARG) return 1;
        if (expose(s, c, 0, 5, 1, 2, 1, 0, 0, 0, 0, p, nullptr) != PT_E_ARG) return 1;
        if (expose(s, c, 0, 5, 1, 2, 1, 1, 2, 0, 0, p, nullptr) != PT_E_ARG) return 1;            // accumulate_first
        if (expose(s, c, 0, 5, 1, 0, 1, 1, 0, 0, 0, p, nullptr) != PT_E_ARG) return 1;            // guide_frames
        if (expose(s, c, 0, 5, 1, 2, 1, 1, 0, -1, 0, p, nullptr) != PT_E_ARG) return 1;           // frames_before
        if (expose(s, c, 0, 5, 1, 2, 1, 1, 0, 0, 3, p, nullptr) != PT_E_ARG) return 1;            // guides_held > guide_frames
        if (expose(s, c, 0, 5, 1, 2, 1, 1, 0, 0, -1, p, nullptr) != PT_E_ARG) return 1;
        if (expose(s, c, 0, 5, 5, 2, 1, 1, 0, 0, 0, p, nullptr) != PT_E_ARG) return 1;            // display mode
        if (pt_film_expose_host(s.tris.data(), s.nt, s.nodes.data(), s.nn, s.mats.data(), s.nm, s.sph.data(), s.ns, 0, 5, 1, &c,
                                2, 1, 1, 0, 0, 0, p.rgba.data(), nullptr, p.gd.data(), nullptr) != PT_E_ARG) return 1;
        if (s.nn > 0 && !(s.nodes[8] > -1.0f)) {   // a cycle: the root's miss link back to the root
            Scene bad = s;
            bad.nodes[11] = 0.0f;
            if (expose(bad, camera(1, 1, 1, 0), 0, 5, 1, 2, 1, 1, 0, 0, 0, p, nullptr) != PT_E_SCENE) { std::fprintf(stderr, "%s: cycle accepted\n", argv[a]); return 1; }
        }
    }
    if (accepted < 40 || rejected < 40) { std::fprintf(stderr, "the random cameras are one-sided: %lld accepted, %lld rejected\n", accepted, rejected); return 1; }
    std::printf("film_host_san ok: %lld paths, %lld random cameras accepted, %lld rejected\n", paths, accepted, rejected);
    return 0;
}
