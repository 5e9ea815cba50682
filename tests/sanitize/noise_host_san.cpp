// noise_host_san.cpp -- pt_noise_host (csrc/pt_noise.cpp over csrc/pt_noise.h, the device
// kernels' own per-pixel code) under ASan + UBSan with float-cast-overflow: moments of every
// bit pattern (NaN, infinities, negative and huge sums), every frame count class, targets of
// any value, with and without a footprint mask, and the refused arguments.  The float ->
// unsigned conversions of the quantiser must stay in range for all of them.  Host only.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow
//       -fno-sanitize-recover=all noise_host_san.cpp ../../opengl-path-tracing_amd/csrc/pt_noise.cpp
#include "../../include/pt_api.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

#define REQUIRE(x) do { if (!(x)) { std::printf("FAILED %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main() {
    const float specials[] = {0.0f, -0.0f, 1.0f, -1.0f, -0.01f, 1e-45f, 3.4e38f, -3.4e38f, bits(0x7F800000u),
                              bits(0xFF800000u), bits(0x7FC00000u), bits(0xFFC00001u)};
    const int n_special = (int)(sizeof(specials) / sizeof(specials[0]));
    const int counts[] = {2, 3, 16, 1 << 24, (1 << 24) + 1, 0x7FFFFFFF};
    for (int round = 0; round < 400; round++) {
        const size_t n = 1 + rnd() % 300;
        std::vector<float> mom(2 * n);
        std::vector<unsigned char> mask(n);
        for (size_t i = 0; i < 2 * n; i++) {
            const uint32_t r = rnd();
            mom[i] = (r & 3) == 0 ? specials[(r >> 2) % n_special] : bits(rnd() << 16 ^ rnd());
        }
        size_t inside = 0;
        for (size_t i = 0; i < n; i++) {
            mask[i] = (unsigned char)(rnd() % 3 ? 1 + rnd() % 255 : 0);
            inside += mask[i] != 0;
        }
        const int frames = counts[round % 6];
        const float target = round % 5 == 0 ? specials[(round / 5) % n_special] : bits(rnd() << 16 ^ rnd());
        pt_noise_stats all, in;
        REQUIRE(pt_noise_host(mom.data(), nullptr, n, frames, target, &all) == PT_OK);
        REQUIRE(pt_noise_host(mom.data(), mask.data(), n, frames, target, &in) == PT_OK);
        REQUIRE(all.pixels == n && in.pixels == inside && all.frames == frames && in.frames == frames);
        REQUIRE(all.max_q <= (64u << 16) && in.max_q <= all.max_q);
        REQUIRE(all.sum_q <= all.pixels * all.max_q && in.sum_q <= all.sum_q);
        REQUIRE(all.above <= all.pixels && in.above <= in.pixels && in.above <= all.above);
    }
    pt_noise_stats s;
    const float two[4] = {1.0f, 1.0f, 2.0f, 3.0f};
    REQUIRE(pt_noise_host(two, nullptr, 2, 1, 0.25f, &s) == PT_E_ARG);
    REQUIRE(pt_noise_host(two, nullptr, 2, -5, 0.25f, &s) == PT_E_ARG);
    REQUIRE(pt_noise_host(nullptr, nullptr, 2, 4, 0.25f, &s) == PT_E_ARG);
    REQUIRE(pt_noise_host(two, nullptr, 2, 4, 0.25f, nullptr) == PT_E_ARG);
    REQUIRE(pt_noise_host(nullptr, nullptr, 0, 4, 0.25f, &s) == PT_OK && s.pixels == 0 && s.max_q == 0);
    std::printf("noise_host_san ok\n");
    return 0;
}
