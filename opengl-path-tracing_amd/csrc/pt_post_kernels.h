// pt_post_kernels.h -- a section of the pt_render.hip translation unit, not a general-purpose
// header: pt_render.hip includes it once, after pt_kparams.h.
// The small kernels around the render kernel: the progressive graph's frame counter, the
// adaptive tile order, the frame-split mode's running mean, the tonemap and the noise summary.
namespace {

using pti::accumulate;

// Progressive mode: the device frame counter of resolve_frames moves on after a replay.
__global__ void k_advance_frames(int* frame_dev, int n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *frame_dev += n;
}

// Adaptive tile order, on the device after every launch that recorded tile
// costs: longest-processing-time-first order of the 8x8 tiles for the next launches -- a
// counting sort of the recorded segment counts into 1024 buckets, most expensive first --
// then the counts are cleared.  Stream-ordered, so the next launch reads the new order with
// no host round trip (the host form cost ~0.2 ms per pt_render: three synchronous copies).
// The order inside a bucket is whatever the LDS atomics give: tile order changes only the
// launch tail, never the image.  One 1024-thread workgroup.
__global__ __launch_bounds__(1024) void k_tile_order(unsigned* __restrict__ cost, unsigned* __restrict__ perm,
                                                     int n_tiles, int tiles_x) {
    constexpr int nb = 1024;
    __shared__ unsigned hist[nb], base[nb], wmax[16];
    const int tid = threadIdx.x;
    unsigned mx = 1u;
    for (int t = tid; t < n_tiles; t += 1024) mx = max(mx, cost[t]);
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    hist[tid] = 0u;
    __syncthreads();
    mx = wmax[0];
    for (int w = 1; w < 16; w++) mx = max(mx, wmax[w]);
    auto bucket = [&](unsigned v) { return nb - 1 - (int)((unsigned long long)v * (nb - 1) / mx); };
    for (int t = tid; t < n_tiles; t += 1024) atomicAdd(&hist[bucket(cost[t])], 1u);
    __syncthreads();
    const unsigned own = hist[tid];
    for (int off = 1; off < nb; off <<= 1) {      // inclusive scan of the bucket sizes
        const unsigned add = tid >= off ? hist[tid - off] : 0u;
        __syncthreads();
        hist[tid] += add;
        __syncthreads();
    }
    base[tid] = hist[tid] - own;
    __syncthreads();
    for (int t = tid; t < n_tiles; t += 1024) {
        const unsigned pos = atomicAdd(&base[bucket(cost[t])], 1u);
        perm[pos] = ((unsigned)(t / tiles_x) << 16) | (unsigned)(t % tiles_x);
    }
    __syncthreads();
    for (int t = tid; t < n_tiles; t += 1024) cost[t] = 0u;
}

// Running mean of the frame-split mode (:548-551): per local pixel, the launch's frames in
// order from the per-frame colours the render kernel stored -- the same accumulate() the
// lane applies in registers otherwise.  Pixels outside the dispatch footprint are skipped.
// Each thread takes kAccumPix pixels a block-width apart (coalesced), their loads issued
// together: beside a running render this pass gets a few block slots per CU, and with one
// pixel per thread it was latency-bound (about 100 us for a 1080p frame against 15 us alone).
// Long launches (more than kShortLaunch frames): 2 pixels per thread and 8 frames per load
// group (same-process A/B, a 1080p/8 share's 1024-frame launch: +1.6% for the whole render
// against one frame per group, +1.1% with 4 x 4; the full 1080p image unchanged).  Short
// launches keep 4 pixels and one frame per group (the pass beside the next one-frame render).
constexpr int kAccumFramesLong = 8;   // (pixels per thread: ptl::kAccumPix, kAccumPixLong)
// MOMENTS: the per-frame luminance moments of the noise estimate (pt_noise.h) are kept beside
// the image -- loaded with it (or zero where it restarts), updated after each frame's
// accumulate() in the same frame order, stored with it.  The colours are already in registers
// here, in frame order, in a pass that streams: 8 B more read and written per pixel per launch.
template <int kAccumPix, int kAccumFrames, bool MOMENTS = false>
__global__ __launch_bounds__(256) void k_accum_frames(KParams p) {
    resolve_frames(p);
    // the render that used these queue heads has ended (this pass runs after it): ready them
    // for the slot's next render, which waits for this pass (no fill dispatch per launch)
    if (p.reset_work && blockIdx.x == 0 && threadIdx.x == 0) *p.reset_work = 0u;
    // rows_local * W < 2^31 (pt_create), and the grid covers n rounded up to a block's pixels:
    // 32-bit pixel indices
    const unsigned n = (unsigned)p.rows_local * (unsigned)p.W;
    const unsigned base = blockIdx.x * blockDim.x * kAccumPix + threadIdx.x;
    unsigned idx[kAccumPix];
    bool on[kAccumPix];
    float4 acc[kAccumPix];
    float2 mom[MOMENTS ? kAccumPix : 1];
#pragma unroll
    for (int j = 0; j < kAccumPix; j++) {
        idx[j] = base + (unsigned)j * blockDim.x;
        on[j] = idx[j] < n;
        if (on[j]) {
            const int crow = (int)(idx[j] / (unsigned)p.W), cx = (int)(idx[j] - (unsigned)crow * (unsigned)p.W);
            on[j] = cx < p.x_limit && p.row0 + crow * p.row_stride < p.y_limit;
        }
        acc[j] = (on[j] && p.acc_first) ? p.accum[idx[j]] : make_float4(0, 0, 0, 0);
        if constexpr (MOMENTS) mom[j] = (on[j] && p.acc_first) ? p.moments[idx[j]] : make_float2(0, 0);
    }
    // frames in groups of kAccumFrames whose loads are issued together, then applied in frame
    // order: one load group in flight per thread made a long launch's pass latency-bound when
    // few pixels give few threads (a 1080p/8 share's 1024 frames: 0.96 ms for 3.2 GB)
    int k = 0;
    for (; k + kAccumFrames <= p.n_frames; k += kAccumFrames) {
        f3 v[kAccumFrames][kAccumPix];
#pragma unroll
        for (int u = 0; u < kAccumFrames; u++)
#pragma unroll
            for (int j = 0; j < kAccumPix; j++)
                v[u][j] = on[j] ? nt_load3(p.rgb + 3 * ((size_t)(k + u) * (size_t)n + (size_t)idx[j])) : mk(0, 0, 0);
#pragma unroll
        for (int u = 0; u < kAccumFrames; u++)
#pragma unroll
            for (int j = 0; j < kAccumPix; j++) {
                acc[j] = accumulate(acc[j], v[u][j], p.frame_first + k + u, k + u > 0 || p.acc_first == 1);
                if constexpr (MOMENTS) ptn::add_sample(mom[j].x, mom[j].y, ptn::luminance(v[u][j].x, v[u][j].y, v[u][j].z));
            }
    }
    for (; k < p.n_frames; k++) {
        f3 v[kAccumPix];
#pragma unroll
        for (int j = 0; j < kAccumPix; j++)
            v[j] = on[j] ? nt_load3(p.rgb + 3 * ((size_t)k * (size_t)n + (size_t)idx[j])) : mk(0, 0, 0);
#pragma unroll
        for (int j = 0; j < kAccumPix; j++) {
            acc[j] = accumulate(acc[j], v[j], p.frame_first + k, k > 0 || p.acc_first == 1);
            if constexpr (MOMENTS) ptn::add_sample(mom[j].x, mom[j].y, ptn::luminance(v[j].x, v[j].y, v[j].z));
        }
    }
#pragma unroll
    for (int j = 0; j < kAccumPix; j++)
        if (on[j]) {
            p.accum[idx[j]] = acc[j];
            if constexpr (MOMENTS) p.moments[idx[j]] = mom[j];
        }
    // the ACES view of the new image for pt_present_begin (pixels outside the dispatch
    // footprint keep their old value): the same aces_px of the same values as k_aces
    if (p.aces_out) {
#pragma unroll
        for (int j = 0; j < kAccumPix; j++)
            if (idx[j] < n) p.aces_out[idx[j]] = pti::aces_px<uchar4>(on[j] ? acc[j] : p.accum[idx[j]]);
    }
}

// ACES film tonemap epilogue (aces_px) of n pixels.  Each thread
// takes kAcesPix pixels a block-width apart (coalesced), their loads issued together: the pass
// runs beside the next render with few free slots per CU, latency-bound (as k_accum_frames).
#ifndef PT_ACES_PIX
#define PT_ACES_PIX 4
#endif
constexpr int kAcesPix = PT_ACES_PIX;
__global__ __launch_bounds__(256) void k_aces(const float4* __restrict__ src, uchar4* __restrict__ dst,
                                              long long n) {
    const long long base = (long long)blockIdx.x * blockDim.x * kAcesPix + threadIdx.x;
    float4 v[kAcesPix];
#pragma unroll
    for (int j = 0; j < kAcesPix; j++) {
        const long long i = base + (long long)j * blockDim.x;
        v[j] = i < n ? src[i] : make_float4(0, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < kAcesPix; j++) {
        const long long i = base + (long long)j * blockDim.x;
        if (i < n) dst[i] = pti::aces_px<uchar4>(v[j]);
    }
}

// The noise summary of the local rows (pt_noise): every footprint pixel's moments through
// ptn::quantise, summed as integers -- exact in any order, so neither the grid nor the arrival
// order of the atomics can change a field.  A grid-stride loop with the footprint predicate of
// k_accum_frames, per-thread partials, one 64-lane shuffle reduction per wave (every lane of
// the block's four full waves takes part: no lane leaves early), the four waves' results added
// through LDS, and then one set of four device-scope integer atomics per block into the stats
// block the stream zeroed before.  The atomics all land on one 32-byte block and are the
// kernel's cost, about 12 ns each: with one set per wave a 1080p summary took 104 us at 2 blocks
// per CU and 407 us (host round trip) at 8, the time following the number of waves.
#ifndef PT_NOISE_BPC
#define PT_NOISE_BPC 2
#endif
constexpr int kNoiseBlocksPerCu = PT_NOISE_BPC;   // pt_noise's grid: at most this many blocks per CU
__global__ __launch_bounds__(256) void k_noise(KParams p, int frames, unsigned target_q, pt_noise_stats* out) {
    const unsigned n = (unsigned)p.rows_local * (unsigned)p.W;      // < 2^31 (pt_create)
    const unsigned stride = gridDim.x * blockDim.x;                 // a few blocks per CU: i + stride < 2^32
    unsigned long long sum_q = 0;
    unsigned pixels = 0, above = 0, max_q = 0;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int crow = (int)(i / (unsigned)p.W), cx = (int)(i - (unsigned)crow * (unsigned)p.W);
        if (!(cx < p.x_limit && p.row0 + crow * p.row_stride < p.y_limit)) continue;
        const float2 m = p.moments[i];
        const unsigned q = ptn::quantise(m.x, m.y, frames);
        pixels++;
        sum_q += q;
        above += q > target_q;
        max_q = q > max_q ? q : max_q;
    }
    // pixels and above: a wave's counts stay below the image's 2^31 pixels -- 32 bits hold them
    for (int off = 32; off > 0; off >>= 1) {
        pixels += __shfl_xor(pixels, off, 64);
        above += __shfl_xor(above, off, 64);
        const unsigned o = __shfl_xor(max_q, off, 64);
        max_q = o > max_q ? o : max_q;
    }
    sum_q = wave_sum(sum_q);
    __shared__ unsigned long long s_sum[4];
    __shared__ unsigned s_pixels[4], s_above[4], s_max[4];
    const unsigned wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        s_sum[wave] = sum_q;
        s_pixels[wave] = pixels;
        s_above[wave] = above;
        s_max[wave] = max_q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned w = 1; w < 4; w++) {      // a block's counts stay below 2^31 as well
            sum_q += s_sum[w];
            pixels += s_pixels[w];
            above += s_above[w];
            max_q = s_max[w] > max_q ? s_max[w] : max_q;
        }
        if (pixels) {
            atomicAdd(&out->pixels, (unsigned long long)pixels);
            atomicAdd(&out->sum_q, sum_q);
            atomicAdd(&out->above, (unsigned long long)above);
            atomicMax(&out->max_q, max_q);
        }
    }
}

}  // namespace
