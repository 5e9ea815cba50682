// TEST INFRASTRUCTURE: the device twin.  The pinned headers (pt_math.h, pt_cull.h, pt_wide.h, pt_isect.h,
// pt_noise.h) are host- and device-callable, and the CPU suite runs their HOST compilation on
// millions of adversarial cases.  This program runs the same cases through their DEVICE compilation -- one plain
// kernel per family, one case per thread, the functions called as the render kernels call them -- and compares the
// result words with the host compilation's and with the independent references (twin_families.h), word for word.
// Where the device runs other text than the host (v_med3 for fminf, the ballot-fed v_addc_co of sweep_push,
// `if (__any(flush))`, v_ldexp, the compiler's division expansion) this is the only check that sees it at the hard
// inputs.  (The edge tests of the tri family restate tri_edges_at, csrc/pt_render_sm.h, as isect_check.cpp does.)
//
// Build: make -C opengl-path-tracing_amd build/device_twin   (with $(HIPFLAGS), the library's own flags)
//        make -C opengl-path-tracing_amd build/device_twin_nodiv   (a mutant: without the correctly rounded divide)
// usage: device_twin [--nudge] [--div N]
//   --nudge   the device's copy of every case has one operand moved by its smallest step (twin_families.h: nudge),
//             the host keeps the originals: every family must then report dev_vs_host > 0
//   --div N   every case count divided by N
// One JSON line per family: family, cases, positives, dev_vs_host, dev_vs_ref.  The first 10 mismatches go to
// stderr in %a.  Exit 0: no mismatch, 1: a mismatch, 2: a HIP error (nothing is launched after the first).
#include "twin_judge.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#define HIP_OK(call)                                                                                      \
    do {                                                                                                  \
        const hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                           \
            std::fprintf(stderr, "HIP error: %s at %s:%d: %s\n", hipGetErrorString(e_), __FILE__, __LINE__, #call); \
            std::exit(2);                                                                                 \
        }                                                                                                 \
    } while (0)

// one case per thread; `out` holds W words per case
template <class F>
__global__ void k_eval(const typename F::Case* cases, uint32_t* out, long n, typename F::Ctx x) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        uint32_t r[F::W];
        F::eval(cases[i], x, r);
#pragma unroll
        for (int w = 0; w < F::W; w++) out[i * F::W + w] = r[w];
    }
}

namespace {

bool g_nudge = false;
long g_bad = 0;

// the device's words of `cases` (nudged first with --nudge)
template <class F>
std::vector<uint32_t> device_eval(const std::vector<typename F::Case>& cases, const typename F::Ctx& dev_ctx) {
    using Case = typename F::Case;
    const long n = (long)cases.size();
    std::vector<uint32_t> out((size_t)n * F::W);
    if (n == 0) return out;
    std::vector<Case> up(cases);
    if (g_nudge)
        for (Case& c : up) F::nudge(c);
    Case* d_cases = nullptr;
    uint32_t* d_out = nullptr;
    HIP_OK(hipMalloc(&d_cases, sizeof(Case) * (size_t)n));
    HIP_OK(hipMalloc(&d_out, sizeof(uint32_t) * (size_t)n * F::W));
    HIP_OK(hipMemcpy(d_cases, up.data(), sizeof(Case) * (size_t)n, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0xee, sizeof(uint32_t) * (size_t)n * F::W));
    const int block = 256;
    const unsigned grid = (unsigned)((n + block - 1) / block);
    hipLaunchKernelGGL(k_eval<F>, dim3(grid), dim3(block), 0, 0, d_cases, d_out, n, dev_ctx);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), d_out, sizeof(uint32_t) * (size_t)n * F::W, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_cases));
    HIP_OK(hipFree(d_out));
    return out;
}

void print(const twj::Stats& S) {
    std::printf("{\"family\": \"%s\", \"cases\": %ld, \"positives\": %ld, \"dev_vs_host\": %ld, \"dev_vs_ref\": %ld, \"has_ref\": %s, \"nudge\": %s}\n",
                S.family.c_str(), S.cases, S.positives, S.vs_host, S.vs_ref, S.has_ref ? "true" : "false", g_nudge ? "true" : "false");
    std::fflush(stdout);
    g_bad += S.vs_host + S.vs_ref;
}

template <class F>
void family(const std::vector<typename F::Case>& cases) {
    const typename F::Ctx x{};
    twj::Stats S = twj::stats_of<F>();
    const std::vector<uint32_t> dev = device_eval<F>(cases, x);
    const std::vector<uint32_t> host = twj::host_eval<F>(cases, x);
    twj::judge<F>(cases, x, dev.data(), host.data(), S);
    print(S);
}

}  // namespace

int main(int argc, char** argv) {
    long div = 1;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--nudge")) g_nudge = true;
        else if (!std::strcmp(argv[i], "--div") && i + 1 < argc) div = std::atol(argv[++i]);
        else { std::fprintf(stderr, "usage: device_twin [--nudge] [--div N]\n"); return 2; }
    }
    const auto t0 = std::chrono::steady_clock::now();
    twf::Cases C;
    twf::generate(C, div < 1 ? 1 : div);
    if (C.dropped) { std::fprintf(stderr, "%ld cases outside their generator's domain\n", C.dropped); return 1; }
    int n_dev = 0;
    HIP_OK(hipGetDeviceCount(&n_dev));

    family<twf::Slab>(C.slab);
    family<twf::SlabWild>(C.slab_wild);
    family<twf::Cull>(C.cull);
    {   // the sweep: one launch per table, the table in device memory and the same for every ray, as in the kernel
        twj::Stats S = twj::stats_of<twf::Sweep>();
        for (int w = 0; w < twc::kSweepTables; w++) {
            const twc::SweepTable& T = C.sweep[w];
            ptp::Quad* d_table = nullptr;
            HIP_OK(hipMalloc(&d_table, sizeof(ptp::Quad) * T.quads.size()));
            HIP_OK(hipMemcpy(d_table, T.quads.data(), sizeof(ptp::Quad) * T.quads.size(), hipMemcpyHostToDevice));
            const std::vector<uint32_t> dev = device_eval<twf::Sweep>(T.rays, twf::sweep_ctx(T, d_table, g_nudge));
            HIP_OK(hipFree(d_table));
            const twf::SweepCtx hx = twf::sweep_ctx(T, T.quads.data(), false);
            const std::vector<uint32_t> host = twj::host_eval<twf::Sweep>(T.rays, hx);
            twj::judge<twf::Sweep>(T.rays, hx, dev.data(), host.data(), S);
        }
        print(S);
    }
    family<twf::Tri>(C.tri);
    family<twf::Aces>(C.aces);
    family<twf::Accum>(C.accum);
    family<twf::Quant>(C.quant);
    family<twf::Target>(C.target);
    family<twf::Retire>(C.retire);
    family<twf::Fold>(C.fold);
    family<twf::WideHits>(C.wide_hits);
    family<twf::WideNext>(C.wide_next);
    family<twf::Rng>(C.rng);
    family<twf::Vec>(C.vec);
    family<twf::Guard>(C.guard);
    family<twf::Sphere>(C.sphere);
    family<twf::LeafChoice>(C.leaf_choice);
    family<twf::Pinhole>(C.pinhole);
    family<twf::SkyDepth>(C.sky_depth);
    family<twf::Bounce>(C.bounce);

    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("{\"done\": true, \"mismatches\": %ld, \"seconds\": %.2f}\n", g_bad, s);
    return g_bad ? 1 : 0;
}
