// TEST INFRASTRUCTURE: the pipelined leaf sweep (pt_cull.h sweep_mask_piped, the form k_render_pool runs; DESIGN.md
// §5.12, "Round 16") against the plain loop (ptc::sweep_mask), both compiled for the host from the kernel's header.
// The two run the same sweep_hit and sweep_push on the same values in the same order, so their masks must be equal:
//   (1) over seeded random rays inside the exact-reciprocal guard -- all eight octants, t0 finite and infinite --
//       and random finite tables, for every n in 0..32 and every depth D in 1, 2, 3, 4, 8 (so n = D - 1, D, D + 1,
//       counts that are no multiple of the 2 D unroll, 24 and 32 are all among them);
//   (2) over the Cornell rays of the sweep model (tests/cull/leaf_sweep_sim.cpp draws them the same way): camera rays
//       of a 1920x1080 grid and their diffuse bounces along the reference's walk, on the packer's own sweep table.
// usage: sweep_piped_check scene.bin [stride]
// Output: one line "random R cornell C octants O infinite I mismatches M"; exit status 1 on a mismatch.
#include "../../opengl-path-tracing_amd/csrc/pt_cull.h"
#include "../../opengl-path-tracing_amd/csrc/pt_scene_pack.h"
#include "../../include/pt_api.h"
#include "../ref_walk.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// pt_scene.cpp (linked for pt_bvh_culling_ok) refers to the GPU builder; this binary is host-only
extern "C" int pt_bvh_build_gpu(const float*, int, float*, int, int*, int) { return PT_E_HIP; }

using pt::f3;
using pt::mk;

namespace {

long mismatches = 0;

template <int D>
void one_depth(const ptc::SweepRay& sr, float t0, float c_lo, const ptp::Quad* table, int n, unsigned want) {
    const unsigned got = ptc::sweep_mask_piped<D>(sr, t0, c_lo, table, n);
    if (got != want) {
        if (mismatches < 10) std::fprintf(stderr, "D %d n %d t0 %a: plain %08x piped %08x\n", D, n, t0, want, got);
        mismatches++;
    }
}

unsigned all_depths(const ptc::SweepRay& sr, float t0, float c_lo, const ptp::Quad* table, int n) {
    const unsigned want = ptc::sweep_mask(sr, t0, c_lo, table, n);
    one_depth<1>(sr, t0, c_lo, table, n, want);
    one_depth<2>(sr, t0, c_lo, table, n, want);
    one_depth<3>(sr, t0, c_lo, table, n, want);
    one_depth<4>(sr, t0, c_lo, table, n, want);
    one_depth<8>(sr, t0, c_lo, table, n, want);
    return want;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: sweep_piped_check scene.bin [stride]\n"); return 2; }
    const int stride = argc > 2 ? std::atoi(argv[2]) : 16;

    // (1) random rays and tables
    uint32_t st = 88172645u;
    auto rnd = [&]() { return pt::random01(st); };
    long n_random = 0, n_inf = 0, octants = 0, set_bits = 0;
    for (int round = 0; round < 40; round++) {
        ptp::Quad table[64];
        const float size = std::ldexp(1.0f, (int)(pt::next_random(st) % 9u) - 4);
        for (int k = 0; k < 32; k++) {
            float lo[3], hi[3];
            for (int q = 0; q < 3; q++) {
                const float a = (2.0f * rnd() - 1.0f) * size, b = (2.0f * rnd() - 1.0f) * size;
                lo[q] = std::min(a, b);
                hi[q] = (pt::next_random(st) % 8u) == 0 ? lo[q] : std::max(a, b);   // flat boxes too
            }
            table[2 * k] = {lo[0], hi[0], lo[1], hi[1]};
            table[2 * k + 1] = {lo[2], hi[2], 0.0f, 0.0f};
        }
        const float cm[3] = {size * 0x1p-19f, size * 0x1p-19f, size * 0x1p-19f}, ws[3] = {size * 0x1p-18f, 0.0f, size * 0x1p-20f};
        for (int ray = 0; ray < 24; ray++) {
            const unsigned oct = (unsigned)(ray % 8);
            octants |= 1l << oct;
            const f3 o = mk((2.0f * rnd() - 1.0f) * size * 1.5f, (2.0f * rnd() - 1.0f) * size * 1.5f,
                            (ray % 5) == 0 ? 0.0f : (2.0f * rnd() - 1.0f) * size * 1.5f);
            // components in [2^-20, 2] by magnitude, the sign from the octant
            auto comp = [&](bool neg) {
                const float m = (pt::next_random(st) % 6u) == 0 ? std::ldexp(1.0f + rnd(), -1 - (int)(pt::next_random(st) % 19u))
                                                                : 0.05f + 0.95f * rnd();
                return neg ? -m : m;
            };
            const f3 d = mk(comp(oct & 1u), comp(oct & 2u), comp(oct & 4u));
            if (!ref::in_guard(o, d)) { std::fprintf(stderr, "a random ray is outside the guard\n"); return 2; }
            const f3 rd = mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z));
            f3 ol, oh;
            ptc::cull_addends(o, rd, cm, ws, ol, oh);
            const ptc::SweepRay sr = ptc::sweep_ray(rd, ol, oh);
            const bool inf = (ray % 3) == 0;
            const float t0 = inf ? INFINITY : size * (0.01f + 3.0f * rnd());
            n_inf += inf;
            for (int n = 0; n <= 32; n++) {
                set_bits += __builtin_popcount(all_depths(sr, t0, (ray & 1) ? ptc::kWindowLo : -INFINITY, table, n));
                n_random++;
            }
        }
    }
    if (octants != 0xff || set_bits == 0) { std::fprintf(stderr, "the random rays do not exercise the sweep\n"); return 2; }

    // (2) the sweep model's Cornell rays on the packer's table
    if (!ref::load_scene(argv[1]) || ref::nt < 1 || ref::nn < 1) return 2;
    int n_mats = 1;
    for (int i = 0; i < ref::nt; i++) n_mats = std::max(n_mats, (int)ref::tris[16 * (size_t)i + 12] + 1);
    for (int i = 0; i < ref::ns; i++) n_mats = std::max(n_mats, (int)ref::sph[8 * (size_t)i + 4] + 1);
    const std::vector<float> mats(16 * (size_t)n_mats, 0.0f);
    ptp::PackedScene packed;
    std::string err;
    if (ptp::pack_scene(ref::tris.data(), ref::nt, ref::nodes.data(), ref::nn, mats.data(), n_mats,
                        ref::ns ? ref::sph.data() : nullptr, ref::ns, packed, err)) {
        std::fprintf(stderr, "pack_scene: %s\n", err.c_str());
        return 2;
    }
    if (!packed.facts.sweep_ok) { std::fprintf(stderr, "the scene has no sweep table\n"); return 2; }
    const int n_sweep = packed.facts.n_leaves;
    const ptp::Quad* table = reinterpret_cast<const ptp::Quad*>(packed.buf[ptp::kSweep].data());
    const int Wd = 1920, Hd = 1080;
    const f3 pos = mk(ref::cam[0], ref::cam[1], ref::cam[2]);
    const f3 fwd = pt::normalize(mk(ref::cam[4], ref::cam[5], ref::cam[6]));
    const f3 right = pt::normalize(pt::cross(fwd, mk(0, 0, 1)));
    const f3 up = (pt::normalize(pt::cross(right, fwd)) * (float)Hd) / (float)Wd;
    long n_cornell = 0;
    for (int y = 0; y < Hd; y += stride)
        for (int x = 0; x < Wd; x += stride) {
            uint32_t s = pt::seed(x, y, 1);
            const float u = ((float)x + pt::random01(s)) / (float)Wd - 0.5f;
            const float v = ((float)y + pt::random01(s)) / (float)Hd - 0.5f;
            f3 o = pos, d = pt::normalize((fwd + right * u) + up * v);
            for (int bnc = 0; bnc <= 8; bnc++) {
                const float t0 = ref::sphere_t(o, d);
                if (ref::in_guard(o, d)) {
                    const f3 rd = mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z));
                    f3 ol, oh;
                    ptc::cull_addends(o, rd, packed.facts.cons_m, packed.facts.win_slack, ol, oh);
                    all_depths(ptc::sweep_ray(rd, ol, oh), t0, ptc::kWindowLo, table, n_sweep);
                    n_cornell++;
                }
                const ref::RefOut ro = ref::ref_walk(o, d, t0, [](int, bool, float) {}, [](int, float, bool, float) {});
                if (ro.tri < 0) break;
                const float* tr = &ref::tris[16 * (size_t)ro.tri];
                const f3 v0 = ref::ld3(tr), v1 = ref::ld3(tr + 4), v2 = ref::ld3(tr + 8);
                f3 n = pt::normalize(pt::cross(v1 - v0, v2 - v0));
                if (pt::dot(n, d) > 0.0f) n = n * -1.0f;
                o = o + d * ro.t;
                d = pt::normalize(n + pt::random_unit_vector(s));
            }
        }
    std::printf("random %ld cornell %ld octants %ld infinite %ld mismatches %ld\n", n_random, n_cornell, octants, n_inf, mismatches);
    return mismatches ? 1 : 0;
}
