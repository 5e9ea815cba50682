// TEST INFRASTRUCTURE: the signed leaf sweep (pt_cull.h sweep_mask_signed_piped on the signed table, the form
// k_render_pool runs; DESIGN.md §5.12, "Round 17") against the plain loop on the {lo, hi} table (ptc::sweep_mask), both
// compiled for the host from the kernel's header.  The signed table is built by the kernel's own builder
// (ptc::sweep_signed_quad) and read through the kernel's own pair index (ptc::sweep_signed_pair); the masks must be
// equal, mask for mask, at the depths D = 1, 2, 3, 4:
//   (1) seeded random rays inside the exact-reciprocal guard -- all eight octants, t0 finite and infinite, with and
//       without the window clause -- on random finite tables, at every n in 1..32;
//   (2) the Cornell rays of the sweep model (tests/cull/leaf_sweep_sim.cpp draws them the same way) on the packer's own
//       sweep table, whose signed image is also compared with the packer's records float by float;
//   (3) adversarial families, each at every n in 1..32, where the two forms could part if the argument beside
//       ptc::sweep_hit_signed were wrong (a zero of another sign, an inner fma that is not exact):
//         d_edge       direction components of magnitude 2^-20 and 2, both signs
//         zero_bound   bounds equal to 0, so that a product bound * rd is an exact zero
//         zero_addend  addends ol, oh of +0 and -0 (given directly, not through cull_addends), bounds of 0 among them
//         flat         boxes with lo == hi on one or more axes
//         t0_inf       t0 = +inf
//         t0_low       t0 just above the window's low end (the next float above 1e-4)
//       For every family the run counts the cases that reach a box whose verdict is true and those that reach one
//       whose verdict is false: the generators are chosen so that both happen (tests/test_sweep_signed.py requires it).
// usage: sweep_signed_check scene.bin [stride]
// Output: one line of "name count" pairs; exit status 1 on a mismatch.
#include "../../opengl-path-tracing_amd/csrc/pt_cull.h"
#include "../../opengl-path-tracing_amd/csrc/pt_scene_pack.h"
#include "../../include/pt_api.h"
#include "../ref_walk.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// pt_scene.cpp (linked for pt_bvh_culling_ok) refers to the GPU builder; this binary is host-only
extern "C" int pt_bvh_build_gpu(const float*, int, float*, int, int*, int) { return PT_E_HIP; }

using pt::f3;
using pt::mk;

namespace {

struct Pair { float x, y; };    // what one 8-byte read of the signed table returns: (near, far)

long mismatches = 0, builder_bad = 0, octants = 0;

// The signed image of the first n entries of a {lo, hi} table, by the kernel's builder.
std::vector<Pair> signed_table(const ptp::Quad* table, int n) {
    std::vector<Pair> s((size_t)ptc::kSignedPairs * (size_t)n);
    for (int k = 0; k < n; k++)
        for (int axis = 0; axis < ptc::kSignedQuads; axis++) {
            float q[4];
            ptc::sweep_signed_quad(table[2 * k], table[2 * k + 1], axis, q);
            s[(size_t)ptc::kSignedPairs * k + 2 * axis] = {q[0], q[1]};
            s[(size_t)ptc::kSignedPairs * k + 2 * axis + 1] = {q[2], q[3]};
        }
    return s;
}

template <int D>
void one_depth(f3 rd, f3 ol, f3 oh, float t0, float c_lo, const Pair* s, int n, unsigned want, const char* what) {
    const unsigned got = ptc::sweep_mask_signed_piped<D>(rd, ol, oh, t0, c_lo, s + ptc::sweep_signed_pair(rd.x, 0),
                                                         s + ptc::sweep_signed_pair(rd.y, 1), s + ptc::sweep_signed_pair(rd.z, 2), n);
    if (got != want) {
        if (mismatches < 10) std::fprintf(stderr, "%s D %d n %d t0 %a: plain %08x signed %08x\n", what, D, n, t0, want, got);
        mismatches++;
    }
}

// One ray on the first n boxes: the plain mask, compared with the signed one at every depth.
unsigned check(f3 rd, f3 ol, f3 oh, float t0, float c_lo, const ptp::Quad* table, const Pair* s, int n, const char* what) {
    octants |= 1l << ((rd.x > 0.0f ? 0 : 1) | (rd.y > 0.0f ? 0 : 2) | (rd.z > 0.0f ? 0 : 4));
    const unsigned want = ptc::sweep_mask(ptc::sweep_ray(rd, ol, oh), t0, c_lo, table, n);
    one_depth<1>(rd, ol, oh, t0, c_lo, s, n, want, what);
    one_depth<2>(rd, ol, oh, t0, c_lo, s, n, want, what);
    one_depth<3>(rd, ol, oh, t0, c_lo, s, n, want, what);
    one_depth<4>(rd, ol, oh, t0, c_lo, s, n, want, what);
    return want;
}

uint32_t st = 2463534242u;
float rnd() { return pt::random01(st); }
unsigned pick(unsigned n) { return pt::next_random(st) % n; }
float sym(float size) { return (2.0f * rnd() - 1.0f) * size; }

enum Family { kDEdge, kZeroBound, kZeroAddend, kFlat, kT0Inf, kT0Low, kFamilies };
const char* const kFamilyName[kFamilies] = {"d_edge", "zero_bound", "zero_addend", "flat", "t0_inf", "t0_low"};
long fam_cases[kFamilies], fam_true[kFamilies], fam_false[kFamilies];

// A table of 32 boxes around the origin for one family: about half of them contain the origin's neighbourhood (so a
// ray from there finds verdicts of both kinds), with the family's feature in the bounds where it is one of bounds.
void family_table(Family f, float size, ptp::Quad* table) {
    for (int k = 0; k < 32; k++) {
        float lo[3], hi[3];
        const bool around = pick(2u) == 0;      // a box around the origin, or one anywhere
        for (int q = 0; q < 3; q++) {
            float a = around ? -rnd() * size : sym(size), b = around ? rnd() * size : sym(size);
            lo[q] = std::min(a, b), hi[q] = std::max(a, b);
            if ((f == kZeroBound || f == kZeroAddend) && pick(2u) == 0) {
                switch (pick(4u)) {             // a bound that is a zero, of either sign
                case 0: lo[q] = 0.0f; hi[q] = std::fabs(hi[q]); break;
                case 1: hi[q] = 0.0f; lo[q] = -std::fabs(lo[q]); break;
                case 2: lo[q] = -0.0f; hi[q] = std::fabs(hi[q]); break;
                default: lo[q] = hi[q] = 0.0f; break;
                }
            }
            if (f == kFlat && pick(2u) == 0) hi[q] = lo[q] = (pick(2u) == 0 ? 0.25f * sym(size) : lo[q]);
        }
        table[2 * k] = {lo[0], hi[0], lo[1], hi[1]};
        table[2 * k + 1] = {lo[2], hi[2], 0.0f, 0.0f};
    }
}

float dir_component(bool edge) {
    float m = 0.05f + 0.95f * rnd();
    if (edge) m = pick(2u) == 0 ? 0x1p-20f : 2.0f;
    return pick(2u) == 0 ? m : -m;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: sweep_signed_check scene.bin [stride]\n"); return 2; }
    const int stride = argc > 2 ? std::atoi(argv[2]) : 16;

    // (1) random rays and tables
    long n_random = 0, n_inf = 0, set_bits = 0;
    for (int round = 0; round < 40; round++) {
        ptp::Quad table[64];
        const float size = std::ldexp(1.0f, (int)pick(9u) - 4);
        for (int k = 0; k < 32; k++) {
            float lo[3], hi[3];
            for (int q = 0; q < 3; q++) {
                const float a = sym(size), b = sym(size);
                lo[q] = std::min(a, b);
                hi[q] = pick(8u) == 0 ? lo[q] : std::max(a, b);
            }
            table[2 * k] = {lo[0], hi[0], lo[1], hi[1]};
            table[2 * k + 1] = {lo[2], hi[2], 0.0f, 0.0f};
        }
        const std::vector<Pair> s = signed_table(table, 32);
        const float cm[3] = {size * 0x1p-19f, size * 0x1p-19f, size * 0x1p-19f}, ws[3] = {size * 0x1p-18f, 0.0f, size * 0x1p-20f};
        for (int ray = 0; ray < 24; ray++) {
            const unsigned oct = (unsigned)(ray % 8);
            const f3 o = mk(sym(size * 1.5f), sym(size * 1.5f), (ray % 5) == 0 ? 0.0f : sym(size * 1.5f));
            auto comp = [&](bool neg) {
                const float m = pick(6u) == 0 ? std::ldexp(1.0f + rnd(), -1 - (int)pick(19u)) : 0.05f + 0.95f * rnd();
                return neg ? -m : m;
            };
            const f3 d = mk(comp(oct & 1u), comp(oct & 2u), comp(oct & 4u));
            if (!ref::in_guard(o, d)) { std::fprintf(stderr, "a random ray is outside the guard\n"); return 2; }
            const f3 rd = mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z));
            f3 ol, oh;
            ptc::cull_addends(o, rd, cm, ws, ol, oh);
            const bool inf = (ray % 3) == 0;
            const float t0 = inf ? INFINITY : size * (0.01f + 3.0f * rnd());
            n_inf += inf;
            for (int n = 1; n <= 32; n++) {
                set_bits += __builtin_popcount(check(rd, ol, oh, t0, (ray & 1) ? ptc::kWindowLo : -INFINITY, table, s.data(), n, "random"));
                n_random++;
            }
        }
    }
    if (set_bits == 0) { std::fprintf(stderr, "the random rays do not exercise the sweep\n"); return 2; }

    // (3) the adversarial families
    for (int f = 0; f < kFamilies; f++)
        for (int round = 0; round < 12; round++) {
            ptp::Quad table[64];
            const float size = std::ldexp(1.0f, (int)pick(5u) - 2);
            family_table((Family)f, size, table);
            const std::vector<Pair> s = signed_table(table, 32);
            const float cm[3] = {size * 0x1p-19f, size * 0x1p-19f, size * 0x1p-19f}, ws[3] = {size * 0x1p-18f, 0.0f, size * 0x1p-20f};
            for (int ray = 0; ray < 16; ray++) {
                // an origin near the middle of the boxes, or exactly on it
                const f3 o = (f == kZeroAddend || pick(4u) == 0) ? mk(0, 0, 0) : mk(sym(0.3f * size), sym(0.3f * size), sym(0.3f * size));
                const f3 d = mk(dir_component(f == kDEdge && pick(3u) != 0), dir_component(f == kDEdge && pick(3u) != 0),
                                dir_component(f == kDEdge && pick(3u) != 0));
                if (!ref::in_guard(o, d)) { std::fprintf(stderr, "a %s ray is outside the guard\n", kFamilyName[f]); return 2; }
                const f3 rd = mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z));
                f3 ol, oh;
                ptc::cull_addends(o, rd, cm, ws, ol, oh);
                if (f == kZeroAddend) {         // zeros of either sign, some axes keeping a small margin
                    auto z = [&](float keep) { return pick(4u) == 0 ? keep : (pick(2u) == 0 ? 0.0f : -0.0f); };
                    ol = mk(z(ol.x), z(ol.y), z(ol.z));
                    oh = mk(z(oh.x), z(oh.y), z(oh.z));
                }
                float t0 = pick(3u) == 0 ? INFINITY : size * (0.01f + 3.0f * rnd());
                if (f == kT0Inf) t0 = INFINITY;
                if (f == kT0Low) t0 = std::nextafterf(0.0001f, 1.0f);
                const float c_lo = (f == kT0Low || pick(2u) == 0) ? ptc::kWindowLo : -INFINITY;
                for (int n = 1; n <= 32; n++) {
                    const unsigned m = check(rd, ol, oh, t0, c_lo, table, s.data(), n, kFamilyName[f]);
                    const unsigned all = n == 32 ? 0xffffffffu : (1u << n) - 1u;
                    fam_cases[f]++;
                    fam_true[f] += m != 0u;
                    fam_false[f] += (m & all) != all;
                }
            }
        }

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
    const std::vector<Pair> s = signed_table(table, n_sweep);
    {   // the builder against the packer's records, float by float: per leaf and axis {lo, hi, hi, lo}
        const float* rec = reinterpret_cast<const float*>(table);
        const float* sg = reinterpret_cast<const float*>(s.data());
        for (int k = 0; k < n_sweep; k++)
            for (int a = 0; a < 3; a++) {
                const float want[4] = {rec[8 * k + 2 * a], rec[8 * k + 2 * a + 1], rec[8 * k + 2 * a + 1], rec[8 * k + 2 * a]};
                if (std::memcmp(want, sg + 12 * k + 4 * a, sizeof want) != 0) builder_bad++;
                if (!(want[0] <= want[1])) builder_bad++;
            }
    }
    const int Wd = 1920, Hd = 1080;
    const f3 pos = mk(ref::cam[0], ref::cam[1], ref::cam[2]);
    const f3 fwd = pt::normalize(mk(ref::cam[4], ref::cam[5], ref::cam[6]));
    const f3 right = pt::normalize(pt::cross(fwd, mk(0, 0, 1)));
    const f3 up = (pt::normalize(pt::cross(right, fwd)) * (float)Hd) / (float)Wd;
    long n_cornell = 0;
    for (int y = 0; y < Hd; y += stride)
        for (int x = 0; x < Wd; x += stride) {
            uint32_t sd = pt::seed(x, y, 1);
            const float u = ((float)x + pt::random01(sd)) / (float)Wd - 0.5f;
            const float v = ((float)y + pt::random01(sd)) / (float)Hd - 0.5f;
            f3 o = pos, d = pt::normalize((fwd + right * u) + up * v);
            for (int bnc = 0; bnc <= 8; bnc++) {
                const float t0 = ref::sphere_t(o, d);
                if (ref::in_guard(o, d)) {
                    const f3 rd = mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z));
                    f3 ol, oh;
                    ptc::cull_addends(o, rd, packed.facts.cons_m, packed.facts.win_slack, ol, oh);
                    check(rd, ol, oh, t0, ptc::kWindowLo, table, s.data(), n_sweep, "cornell");
                    n_cornell++;
                }
                const ref::RefOut ro = ref::ref_walk(o, d, t0, [](int, bool, float) {}, [](int, float, bool, float) {});
                if (ro.tri < 0) break;
                const float* tr = &ref::tris[16 * (size_t)ro.tri];
                const f3 v0 = ref::ld3(tr), v1 = ref::ld3(tr + 4), v2 = ref::ld3(tr + 8);
                f3 n = pt::normalize(pt::cross(v1 - v0, v2 - v0));
                if (pt::dot(n, d) > 0.0f) n = n * -1.0f;
                o = o + d * ro.t;
                d = pt::normalize(n + pt::random_unit_vector(sd));
            }
        }
    std::printf("random %ld cornell %ld leaves %d octants %ld infinite %ld mismatches %ld builder_bad %ld", n_random, n_cornell,
                n_sweep, octants, n_inf, mismatches, builder_bad);
    for (int f = 0; f < kFamilies; f++)
        std::printf(" %s %ld %s_true %ld %s_false %ld", kFamilyName[f], fam_cases[f], kFamilyName[f], fam_true[f],
                    kFamilyName[f], fam_false[f]);
    std::printf("\n");
    return (mismatches || builder_bad) ? 1 : 0;
}
