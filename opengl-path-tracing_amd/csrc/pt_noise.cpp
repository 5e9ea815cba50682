// pt_noise.cpp -- the noise summary on the host (include/pt_api.h: pt_noise_host).  Plain host
// code over pt_noise.h, the functions k_noise runs on the device: the CPU suite
// (tests/test_noise_host.py) checks them against a numpy restatement bit for bit, and the GPU
// suite checks pt_noise against this.
#include "pt_noise.h"

#include "../../include/pt_api.h"

extern "C" {

int pt_noise_host(const float* moments, const unsigned char* in_footprint, size_t n_pixels, int frames, float target,
                  pt_noise_stats* out) {
    if (!out || (!moments && n_pixels) || frames < 2) return PT_E_ARG;
    const unsigned tq = ptn::target_q(target);
    pt_noise_stats s = {0, 0, 0, 0, frames};
    for (size_t i = 0; i < n_pixels; i++) {
        if (in_footprint && !in_footprint[i]) continue;
        const unsigned q = ptn::quantise(moments[2 * i], moments[2 * i + 1], frames);
        s.pixels++;
        s.sum_q += q;
        s.above += q > tq;
        if (q > s.max_q) s.max_q = q;
    }
    *out = s;
    return PT_OK;
}

int pt_tile_retires_host(const float* moments, const unsigned char* in_footprint, size_t n_pixels, int frames,
                         float target, int* retires) {
    if (!retires) return PT_E_ARG;
    pt_noise_stats s;
    const int rc = pt_noise_host(moments, in_footprint, n_pixels, frames, target, &s);
    if (rc) return rc;
    *retires = ptn::tile_retires(s.sum_q, s.pixels, ptn::target_q(target)) ? 1 : 0;
    return PT_OK;
}

}  // extern "C"
