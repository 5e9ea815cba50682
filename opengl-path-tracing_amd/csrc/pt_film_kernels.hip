// pt_film_kernels.hip -- the device half of the film (include/pt_api.h: pt_film_*) and its entry points.
// A film holds the running image, the luminance moments and the first-hit guides of one pt_camera on one context;
// k_film_expose writes all three in one pass over the paths.  A lane holds one pixel and runs, per frame,
// ptcam::make_ray, then ptq::cast and ptt::shade for the first segment and for every later one -- ptt::segment with
// the hit at hand -- the per-pixel code the host twin (pt_film.cpp) runs too.  A translation unit of its own: the
// render kernels', the query's, the traced rays', the camera models' and the denoiser's code objects stay as they are.
//
// k_film_expose<MREG>: k_trace_camera<-1>'s refill scheme (pt_camera_kernels.hip) with two additions.  In a guide
// frame the first segment's hit is folded into the two guide quads by read-modify-write in global memory: G of
// possibly hundreds of frames, so nothing of it lives in registers across the walk.  At a path's end the colour's
// luminance is folded into the moments: MREG = true keeps (S1, S2) in registers beside the running mean and stores
// them with the pixel, MREG = false reads and writes the pixel's 8 bytes at each path end (DESIGN.md §15.4 has the
// measurement that chose).  What only those places read -- the three plane pointers, the guide range, the guides-only
// flag -- is read back from the argument segment there, like the camera.
// TWIN: k_trace_camera<-1> (pt_camera_kernels.hip), the refill loop (one shared loop moved the
// registers of all three kernels).
// Shared with the other ray-batch units: the scene accessor, rank_in, the argument-segment read, the
// compute-unit count and the persistent grid's size come from pt_batch_device.h, the error return and the checks of the
// entry points from pt_entry.h.
#include "pt_film_launch.h"

#include "pt_batch_device.h"
#include "pt_denoise_launch.h"
#include "pt_entry.h"
#include "pt_scene_pack.h"

#include <climits>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>

namespace ptfilm {
namespace {

using ptb::kThreads;
using ptb::kWaves;
using ptb::rank_in;

// What the guide fold and the path end read, and nothing else does.
struct Rare {
    float2* moments;
    float4* g0;
    float4* g1;
    int g_lo, g_hi;
    int guides_only, pad;
};

struct FilmArgs {
    const float4* nodes;
    const float4* tris;
    const float4* spheres;
    const float4* leaf_tris;
    const float4* mats;
    float4* rgba;
    long long n;                           // W * H
    int n_nodes, n_spheres, scene_fast;
    ptt::Frames fr;
    Rare rare;
    ptcam::Prepared cam;
};

// The camera and the rare words, read back from the argument segment where they are used (ptb::load_arg has the why).
__device__ __forceinline__ ptcam::Prepared load_camera() { return ptb::load_arg<ptcam::Prepared, offsetof(FilmArgs, cam)>(); }
__device__ __forceinline__ Rare load_rare() { return ptb::load_arg<Rare, offsetof(FilmArgs, rare)>(); }

// amdgpu_num_sgpr(96): left alone the compiler keeps literal constants of the walk in scalar registers for as long as
// there are any, 98 in all, and beyond 96 a SIMD holds 6 of this kernel's waves although the occupancy query says 7, so
// that the last seventh of the persistent grid runs as a tail -- what §14.4 found at 106.  Measured here at 98: the
// exposure was 32-37% slower than the plain camera trace on both scenes, and 1-3% with the cap.
template <bool MREG>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_num_sgpr(96))) void k_film_expose(FilmArgs a) {
    const ptb::DevScene<FilmArgs> sc = {a};
    const ptt::Frames fr = a.fr;
    // the wave's share: cursor position c is pixel (c / 64) * 64 * Wn + 64 * w + c % 64
    const long long w = (long long)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long Wn = (long long)gridDim.x * kWaves;
    const long long n_blocks = (a.n + 63) >> 6;
    const long long c_end = w < n_blocks ? 64 * ((n_blocks - w + Wn - 1) / Wn) : 0;
    long long c = 0;          // wave-uniform
    bool live = false;
    int x = 0, y = 0;         // the lane's pixel: index (unsigned)y * W + x
    f3 o = mk(0, 0, 0), d = o, inc = o, col = o;
    uint32_t state = 0u;
    int bounce = 0, kf = 0;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float2 mom = make_float2(0.0f, 0.0f);      // MREG only
    for (;;) {
        const unsigned long long want = __ballot(!live);
        if (want != 0ull && c < c_end) {
            if (!live) {
                const long long cc = c + rank_in(want);
                const long long idx = (cc >> 6) * 64 * Wn + 64 * w + (cc & 63);
                if (cc < c_end && idx < a.n) {           // the share's last block may be the image's ragged tail
                    y = (int)((unsigned)idx / (unsigned)a.cam.W), x = (int)((unsigned)idx - (unsigned)y * (unsigned)a.cam.W);   // idx < W * H < 2^31
                    kf = 0;
                    state = pt::seed(x, y, fr.frame_first);
                    ptcam::make_ray<-1>(load_camera(), x, y, state, o, d);
                    ptt::start_path(inc, col, bounce);
                    if (fr.acc_first == 1) {             // (a guides-only launch never accumulates)
                        acc = a.rgba[idx];
                        if (MREG) mom = load_rare().moments[idx];
                    } else if (MREG) {
                        mom = make_float2(0.0f, 0.0f);
                    }
                    live = true;
                }
            }
            c += __popcll(want);
        }
        if (__ballot(live) == 0ull) {
            if (c >= c_end) break;
            continue;
        }
        if (live) {
            f3 rgb;
            const ptq::Hit h = ptq::cast<float4>(sc, o, d, __builtin_huge_valf(), fr.flags, false);
            bool only = false;                           // a guides-only launch: the path ends here
            if (bounce == 0) {                           // the first segment of a path
                const Rare r = load_rare();
                const int f = fr.frame_first + kf;
                if (f >= r.g_lo && f <= r.g_hi) {
                    const size_t idx = (size_t)((unsigned)y * (unsigned)a.cam.W + (unsigned)x);
                    float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = q0;
                    if (f > 1) q0 = r.g0[idx], q1 = r.g1[idx];
                    fold_guides(q0, q1, guide_sample<float4>(sc, h, o, d, fr.flags), f);
                    r.g0[idx] = q0;
                    r.g1[idx] = q1;
                }
                only = r.guides_only != 0;
            }
            bool ended = true;
            if (!only) ended = ptt::shade<float4>(sc, h, o, d, inc, col, state, bounce, fr.max_bounce, fr.mode, fr.flags, rgb);
            if (ended) {
                if (!only) {
                    const bool accf = kf > 0 || fr.acc_first == 1;
                    acc = pti::accumulate(acc, rgb, fr.frame_first + kf, accf);
                    const float lum = ptn::luminance(rgb.x, rgb.y, rgb.z);
                    if (MREG) {
                        ptn::add_sample(mom.x, mom.y, lum);
                    } else {
                        float2* const mp = load_rare().moments + (size_t)((unsigned)y * (unsigned)a.cam.W + (unsigned)x);
                        float2 m = make_float2(0.0f, 0.0f);
                        if (accf) m = *mp;
                        ptn::add_sample(m.x, m.y, lum);
                        *mp = m;
                    }
                }
                kf++;
                if (kf == fr.n_frames) {
                    if (!only) {
                        const size_t idx = (size_t)((unsigned)y * (unsigned)a.cam.W + (unsigned)x);
                        a.rgba[idx] = acc;
                        if (MREG) load_rare().moments[idx] = mom;
                    }
                    live = false;
                } else {                                 // the next frame of the same pixel: its ray anew
                    state = pt::seed(x, y, fr.frame_first + kf);
                    ptcam::make_ray<-1>(load_camera(), x, y, state, o, d);
                    ptt::start_path(inc, col, bounce);
                }
            }
        }
    }
}

// ptb::load_arg's premise: the kernel's one parameter is FilmArgs, at offset 0 of the argument segment.
static_assert(std::is_same<decltype(&k_film_expose<false>), void (*)(FilmArgs)>::value, "FilmArgs is the only kernel parameter");
static_assert(std::is_same<decltype(&k_film_expose<true>), void (*)(FilmArgs)>::value, "FilmArgs is the only kernel parameter");

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// The noise summary of n pixels (pt_film_noise): k_noise's shape (pt_post_kernels.h) without a footprint -- a
// grid-stride loop, per-lane integer partials, one 64-lane reduction per wave (no lane leaves early), the four waves'
// results added through LDS, then one set of integer atomics per block into the block the stream zeroed before.
// Every field is an integer: exact in any order.
__global__ __launch_bounds__(kThreads) void k_film_noise(const float2* __restrict__ moments, unsigned long long n, int frames,
                                                         unsigned target_q, pt_noise_stats* out) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kThreads;
    unsigned long long sum_q = 0;
    unsigned pixels = 0, above = 0, max_q = 0;      // n < 2^31 (pt_film_create): 32 bits hold the counts
    for (unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const float2 m = moments[i];
        const unsigned q = ptn::quantise(m.x, m.y, frames);
        pixels++;
        sum_q += q;
        above += q > target_q;
        max_q = q > max_q ? q : max_q;
    }
    for (int off = 32; off > 0; off >>= 1) {
        pixels += __shfl_xor(pixels, off, 64);
        above += __shfl_xor(above, off, 64);
        const unsigned o = __shfl_xor(max_q, off, 64);
        max_q = o > max_q ? o : max_q;
    }
    sum_q = wave_sum64(sum_q);
    __shared__ unsigned long long s_sum[kWaves];
    __shared__ unsigned s_pixels[kWaves], s_above[kWaves], s_max[kWaves];
    const unsigned wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        s_sum[wave] = sum_q;
        s_pixels[wave] = pixels;
        s_above[wave] = above;
        s_max[wave] = max_q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned k = 1; k < (unsigned)kWaves; k++) {
            sum_q += s_sum[k];
            pixels += s_pixels[k];
            above += s_above[k];
            max_q = s_max[k] > max_q ? s_max[k] : max_q;
        }
        if (pixels) {
            atomicAdd(&out->pixels, (unsigned long long)pixels);
            atomicAdd(&out->sum_q, sum_q);
            atomicAdd(&out->above, (unsigned long long)above);
            atomicMax(&out->max_q, max_q);
        }
    }
}

// One thread per pixel over pti::aces_px (the render unit's k_aces is its own).
__global__ __launch_bounds__(kThreads) void k_film_aces(const float4* __restrict__ src, uchar4* __restrict__ dst, long long n) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) dst[i] = pti::aces_px<uchar4>(src[i]);
}

}  // namespace

hipError_t launch_expose(hipStream_t s, const ptt::CtxView& v, const Launch& l) {
    const long long n = (long long)l.cam.W * l.cam.H;
    if (n <= 0 || l.n_frames <= 0) return hipSuccess;
    const ptt::Frames fr = {v.q.flags, v.max_bounce, v.mode, l.frame_first, l.n_frames, l.guides_only ? 0 : l.acc_first};
    const Rare rare = {l.moments, l.g0, l.g1, l.guides.lo, l.guides.hi, l.guides_only ? 1 : 0, 0};
    const FilmArgs a = {v.q.nodes, v.q.tris, v.q.spheres, v.q.leaf_tris, v.mats, l.rgba, n,
                        v.q.n_nodes, v.q.n_spheres, v.q.scene_fast, fr, rare, l.cam};
    void (*fn)(FilmArgs) = l.moments_in_regs ? k_film_expose<true> : k_film_expose<false>;
    static ptb::Resident resident[2];
    const unsigned blocks = ptb::persistent_grid((const void*)fn, resident[l.moments_in_regs ? 1 : 0], v.q.device, n,
                                                 l.grid_cap);
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_noise(hipStream_t s, int device, const float2* moments, long long n, int frames, unsigned target_q,
                        pt_noise_stats* out) {
    if (n <= 0) return hipSuccess;
    long long blocks = (n + kThreads - 1) / kThreads;
    const long long cap = 2LL * ptb::compute_units(device);      // k_noise's grid: two blocks per compute unit
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_film_noise, dim3((unsigned)blocks), dim3(kThreads), 0, s, moments, (unsigned long long)n, frames,
                       target_q, out);
    return hipGetLastError();
}

hipError_t launch_aces(hipStream_t s, const float4* src, uchar4* dst, long long n) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_film_aces, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, src, dst, n);
    return hipGetLastError();
}

}  // namespace ptfilm

// ===================================================================== the film and its entry points
// Every plane is allocated by pt_film_create and freed by pt_film_destroy; nothing between them allocates device
// memory.  Everything is enqueued on the context's stream.  The film reaches its context only through pt__trace_view
// and pt__scene_serial: it is invisible to rendering.
struct pt_film {
    pt_ctx* ctx = nullptr;
    pt_camera cam{};
    long long px = 0;                       // width * height
    int guide_frames = 1, guides_held = 0;
    int frames = 0;                         // n of the moments
    unsigned long long serial = 0;          // the context's scene serial as last seen
    float4* image = nullptr;
    float2* moments = nullptr;
    float4* guide = nullptr;                // two planes: (N.rgb, Z) of every pixel, then (A.rgb, 0) of every pixel
    float4* state[2] = {nullptr, nullptr};  // the filter's ping-pong planes
    float4* denoised = nullptr;
    uchar4* rgba8 = nullptr;
    pt_noise_stats* d_noise = nullptr;
    pt_noise_stats* h_noise = nullptr;      // pinned
    bool dn_done = false;
};

namespace {

int g_grid_cap = 0, g_moments = 0;         // pt__film_debug (measurements and tests only)
constexpr bool kMomentsInRegs = false;     // what ships

void free_film(pt_film* f) {
    (void)hipFree(f->image), (void)hipFree(f->moments), (void)hipFree(f->guide), (void)hipFree(f->state[0]);
    (void)hipFree(f->state[1]), (void)hipFree(f->denoised), (void)hipFree(f->rgba8), (void)hipFree(f->d_noise);
    if (f->h_noise) (void)hipHostFree(f->h_noise);
    delete f;
}

// The view of the film's context, the device made current, and the guides dropped when the context's scene has changed.
int enter(pt_film* f, ptt::CtxView& v) {
    if (!f) return PT_E_ARG;
    int rc = pt__trace_view(f->ctx, &v);
    if (rc) return rc;
    unsigned long long serial = 0;
    if ((rc = pt__scene_serial(f->ctx, &serial)) != PT_OK) return rc;
    if (serial != f->serial) f->serial = serial, f->guides_held = 0;
    PTCHK(f->ctx, hipSetDevice(v.q.device));
    return PT_OK;
}

ptfilm::Launch launch_of(const pt_film* f) {
    ptfilm::Launch l;
    l.cam = ptcam::prepare(f->cam);
    l.rgba = f->image, l.moments = f->moments, l.g0 = f->guide, l.g1 = f->guide + f->px;
    l.frame_first = 1, l.n_frames = 0, l.acc_first = 0;
    l.guides = {1, 0};
    l.guides_only = false;
    l.moments_in_regs = g_moments == 0 ? kMomentsInRegs : g_moments == 1;
    l.grid_cap = g_grid_cap;
    return l;
}

int expose(pt_film* f, const ptt::CtxView& v, int frame_first, int n_frames, int accumulate_first) {
    ptfilm::Launch l = launch_of(f);
    l.frame_first = frame_first, l.n_frames = n_frames, l.acc_first = accumulate_first;
    l.guides = ptfilm::guide_range(frame_first, n_frames, f->guides_held, f->guide_frames);
    PTCHK(f->ctx, ptfilm::launch_expose(v.q.stream, v, l));
    f->guides_held = ptfilm::held_after(l.guides, f->guides_held);
    // (a count past INT_MAX stays there: the noise estimate's n is an int)
    f->frames = accumulate_first ? (f->frames > INT_MAX - n_frames ? INT_MAX : f->frames + n_frames) : n_frames;
    return PT_OK;
}

int noise(pt_film* f, const ptt::CtxView& v, float target, pt_noise_stats* out) {
    PTCHK(f->ctx, hipMemsetAsync(f->d_noise, 0, sizeof(pt_noise_stats), v.q.stream));
    PTCHK(f->ctx, ptfilm::launch_noise(v.q.stream, v.q.device, f->moments, f->px, f->frames, ptn::target_q(target), f->d_noise));
    PTCHK(f->ctx, hipMemcpyAsync(f->h_noise, f->d_noise, sizeof(pt_noise_stats), hipMemcpyDeviceToHost, v.q.stream));
    PTCHK(f->ctx, hipStreamSynchronize(v.q.stream));
    *out = *f->h_noise;
    out->frames = f->frames;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_film_create(pt_ctx* c, const pt_camera* cam, int guide_frames, pt_film** out) {
    if (!c || !out) return PT_E_ARG;
    *out = nullptr;
    ptt::CtxView v;
    int rc = pt__trace_view(c, &v);
    if (rc) return rc;
    if ((rc = pte::check_camera(c, cam)) != PT_OK) return rc;
    if (guide_frames < 1) return pt__query_fail(c, PT_E_ARG, "pt_film_create: guide_frames must be >= 1");
    const long long px = (long long)cam->width * cam->height;
    if (px >= (1LL << 31)) return pt__query_fail(c, PT_E_ARG, "pt_film_create: width * height must be below 2^31");
    PTCHK(c, hipSetDevice(v.q.device));
    pt_film* f = new pt_film;
    f->ctx = c, f->cam = *cam, f->px = px, f->guide_frames = guide_frames;
    (void)pt__scene_serial(c, &f->serial);
    const size_t quad = (size_t)px * sizeof(float4);
    hipError_t e = hipMalloc(&f->image, quad);
    if (e == hipSuccess) e = hipMalloc(&f->moments, (size_t)px * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&f->guide, 2 * quad);
    if (e == hipSuccess) e = hipMalloc(&f->state[0], quad);
    if (e == hipSuccess) e = hipMalloc(&f->state[1], quad);
    if (e == hipSuccess) e = hipMalloc(&f->denoised, quad);
    if (e == hipSuccess) e = hipMalloc(&f->rgba8, (size_t)px * sizeof(uchar4));
    if (e == hipSuccess) e = hipMalloc(&f->d_noise, sizeof(pt_noise_stats));
    if (e == hipSuccess) e = hipHostMalloc((void**)&f->h_noise, sizeof(pt_noise_stats), hipHostMallocDefault);
    // a film starts black, with no moments and no guides
    if (e == hipSuccess) e = hipMemsetAsync(f->image, 0, quad, v.q.stream);
    if (e == hipSuccess) e = hipMemsetAsync(f->moments, 0, (size_t)px * sizeof(float2), v.q.stream);
    if (e == hipSuccess) e = hipMemsetAsync(f->guide, 0, 2 * quad, v.q.stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(v.q.stream);
        free_film(f);
        return pte::hip_fail(c, "pt_film_create", e);
    }
    *out = f;
    return PT_OK;
}

void pt_film_destroy(pt_film* f) {
    if (!f) return;
    ptt::CtxView v;
    if (pt__trace_view(f->ctx, &v) == PT_OK && hipSetDevice(v.q.device) == hipSuccess)
        (void)hipStreamSynchronize(v.q.stream);      // nothing in flight may still use the planes
    free_film(f);
}

int pt_film_set_camera(pt_film* f, const pt_camera* cam) {
    if (!f) return PT_E_ARG;
    const int rc = pte::check_camera(f->ctx, cam);
    if (rc) return rc;
    if (cam->width != f->cam.width || cam->height != f->cam.height)
        return pt__query_fail(f->ctx, PT_E_ARG, "pt_film_set_camera: the film keeps its size");
    f->cam = *cam;
    f->guides_held = 0;
    return PT_OK;
}

int pt_film_expose(pt_film* f, int frame_first, int n_frames, int accumulate_first) {
    ptt::CtxView v;
    int rc = enter(f, v);
    if (rc) return rc;
    if ((rc = pte::check_scene(f->ctx, v.q, "pt_film_expose")) != PT_OK) return rc;
    if ((rc = pte::check_frames(f->ctx, frame_first, n_frames, accumulate_first)) != PT_OK) return rc;
    return expose(f, v, frame_first, n_frames, accumulate_first);
}

int pt_film_noise(pt_film* f, float target, pt_noise_stats* out) {
    if (!out) return PT_E_ARG;
    ptt::CtxView v;
    const int rc = enter(f, v);
    if (rc) return rc;
    if (f->frames < 2) return pt__query_fail(f->ctx, PT_E_STATE, "the noise estimate needs at least 2 frames");
    return noise(f, v, target, out);
}

int pt_film_expose_until(pt_film* f, int frame_first, int accumulate_first, int batch, int max_frames, float target,
                         int* frames_done, pt_noise_stats* last) {
    if (!f || !frames_done) return PT_E_ARG;
    *frames_done = 0;
    ptt::CtxView v;
    int rc = enter(f, v);
    if (rc) return rc;
    if (batch < 2 || max_frames < batch || !(target > 0.0f))
        return pt__query_fail(f->ctx, PT_E_ARG, "pt_film_expose_until: batch >= 2, max_frames >= batch, target > 0");
    if ((rc = pte::check_scene(f->ctx, v.q, "pt_film_expose_until")) != PT_OK) return rc;
    if ((rc = pte::check_frames(f->ctx, frame_first, max_frames, accumulate_first)) != PT_OK) return rc;
    // TWIN: pt_render_until (pt_ctx_noise.h), the stop rule.
    const unsigned long long tq = ptn::target_q(target);
    pt_noise_stats s = {0, 0, 0, 0, 0};
    int done = 0;
    while (done < max_frames) {
        const int n = batch < max_frames - done ? batch : max_frames - done;
        if ((rc = expose(f, v, frame_first + done, n, done ? 1 : accumulate_first)) != PT_OK) return rc;
        done += n;
        *frames_done = done;
        if ((rc = noise(f, v, target, &s)) != PT_OK) return rc;
        if (s.sum_q <= tq * s.pixels) break;      // mean relative error at or below the target
    }
    if (last) *last = s;
    return PT_OK;
}

int pt_film_denoise(pt_film* f, const pt_denoise_params* params, pt_denoise_info* info) {
    ptt::CtxView v;
    int rc = enter(f, v);
    if (rc) return rc;
    pt_ctx* c = f->ctx;
    pt_denoise_params dp;
    pt_denoise_defaults(&dp);
    if (params) dp = *params;
    if (dp.iterations < 1 || dp.iterations > ptd::kMaxIterations) return pt__query_fail(c, PT_E_ARG, "pt_film_denoise: iterations must be 1..8");
    if (dp.guide_frames < 1) return pt__query_fail(c, PT_E_ARG, "pt_film_denoise: guide_frames must be >= 1");
    if ((rc = pte::check_scene(c, v.q, "pt_film_denoise")) != PT_OK) return rc;
    if (dp.guide_frames != f->guide_frames) f->guide_frames = dp.guide_frames, f->guides_held = 0;
    const bool gather = f->guides_held < f->guide_frames;
    if (gather) {                                  // the missing guide frames: first segments only
        ptfilm::Launch l = launch_of(f);
        l.frame_first = f->guides_held + 1, l.n_frames = f->guide_frames - f->guides_held;
        l.guides = {l.frame_first, f->guide_frames};
        l.guides_only = true;
        PTCHK(c, ptfilm::launch_expose(v.q.stream, v, l));
        f->guides_held = f->guide_frames;
    }
    const bool guided = f->frames >= 2;
    const ptd::Image im = {f->cam.width, f->cam.height, f->cam.width, f->cam.height};
    ptd::launch_prep(v.q.stream, im, f->image, guided ? f->moments : nullptr, f->frames, nullptr, 0, 0, 1, f->state[0]);
    const ptd::K k = {ptd::inv_sq(dp.sigma_lum), ptd::inv_sq(dp.sigma_normal), ptd::inv_sq(dp.sigma_albedo),
                      ptd::inv_sq(dp.sigma_depth)};
    for (int i = 0; i < dp.iterations; i++) {
        const bool last = i + 1 == dp.iterations;
        ptd::launch_iter(v.q.stream, im, f->state[i & 1], last ? f->denoised : f->state[(i + 1) & 1], f->guide,
                         f->guide + f->px, last ? f->image : nullptr, 1 << i, guided, k, ptd::kAuto);
    }
    PTCHK(c, hipGetLastError());
    f->dn_done = true;
    if (info) *info = {guided ? 1 : 0, gather ? 1 : 0, dp.iterations, f->frames};
    return PT_OK;
}

int pt_film_info(pt_film* f, int* frames, int* guides_held) {
    ptt::CtxView v;
    const int rc = enter(f, v);
    if (rc) return rc;
    if (frames) *frames = f->frames;
    if (guides_held) *guides_held = f->guides_held;
    return PT_OK;
}

int pt_film_device(pt_film* f, int what, void** dev_ptr, size_t* bytes) {
    if (!f || !dev_ptr || !bytes) return PT_E_ARG;
    const size_t px = (size_t)f->px;
    if (what == PT_FILM_IMAGE) *dev_ptr = f->image, *bytes = px * sizeof(float4);
    else if (what == PT_FILM_MOMENTS) *dev_ptr = f->moments, *bytes = px * sizeof(float2);
    else if (what == PT_FILM_GUIDES) *dev_ptr = f->guide, *bytes = 2 * px * sizeof(float4);
    else if (what == PT_FILM_DENOISED) {
        if (!f->dn_done) return pt__query_fail(f->ctx, PT_E_STATE, "no denoised image (pt_film_denoise first)");
        *dev_ptr = f->denoised, *bytes = px * sizeof(float4);
    } else return pt__query_fail(f->ctx, PT_E_ARG, "pt_film_device: planes 0..3");
    return PT_OK;
}

int pt_film_read(pt_film* f, int what, void* dst, size_t bytes) {
    if (!dst) return PT_E_ARG;
    ptt::CtxView v;
    const int rc = enter(f, v);
    if (rc) return rc;
    pt_ctx* c = f->ctx;
    if (what < PT_FILM_IMAGE || what > PT_FILM_DENOISED_ACES8) return pt__query_fail(c, PT_E_ARG, "pt_film_read: unknown plane");
    const size_t px = (size_t)f->px;
    const size_t per_px[6] = {16, 8, 32, 16, 4, 4};
    if (bytes != px * per_px[what]) return pt__query_fail(c, PT_E_ARG, "pt_film_read: bytes is not the plane's size");
    if ((what == PT_FILM_DENOISED || what == PT_FILM_DENOISED_ACES8) && !f->dn_done)
        return pt__query_fail(c, PT_E_STATE, "no denoised image (pt_film_denoise first)");
    const void* src = what == PT_FILM_IMAGE ? (const void*)f->image : what == PT_FILM_MOMENTS ? (const void*)f->moments
                    : what == PT_FILM_DENOISED ? (const void*)f->denoised : (const void*)f->rgba8;
    if (what == PT_FILM_IMAGE_ACES8 || what == PT_FILM_DENOISED_ACES8)
        PTCHK(c, ptfilm::launch_aces(v.q.stream, what == PT_FILM_IMAGE_ACES8 ? f->image : f->denoised, f->rgba8, f->px));
    PTCHK(c, hipStreamSynchronize(v.q.stream));
    if (what != PT_FILM_GUIDES) {
        PTCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return PT_OK;
    }
    // the two planes interleaved per pixel: pt_read_guides' order
    std::vector<float> g(px * 4);
    float* out = (float*)dst;
    for (int h = 0; h < 2; h++) {
        PTCHK(c, hipMemcpy(g.data(), f->guide + (size_t)h * px, px * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < px; i++) std::memcpy(out + 8 * i + 4 * h, g.data() + 4 * i, 4 * sizeof(float));
    }
    return PT_OK;
}

// Measurements and tests only (tools/film_measure.py, tests/test_gpu_film.py), not part of the public ABI: a
// ptfilm::Debug setting for every later exposure of the process.
int pt__film_debug(int what, int value) {
    if (what == ptfilm::kDebugGridCap && value >= 0) g_grid_cap = value;
    else if (what == ptfilm::kDebugMoments && value >= 0 && value <= 2) g_moments = value;
    else return PT_E_ARG;
    return PT_OK;
}

}  // extern "C"
