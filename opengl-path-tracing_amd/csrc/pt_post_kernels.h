// pt_post_kernels.h -- a section of the pt_render.hip translation unit, not a general-purpose
// header: pt_render.hip includes it once, after pt_kparams.h.
// The small kernels around the render kernel: the progressive graph's frame counter, the
// adaptive tile order, the frame-split mode's running mean, the tonemap, the noise summary and
// adaptive sampling's accumulate-and-retire pass.
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

// Adaptive sampling (pt_render_adaptive): the accumulate pass and the stop rule
// of one batch, over the launch's list of active tiles only.  The call's summary block: the
// tiles retired so far (sums that only grow over the call) and the tiles that stay active after
// this batch (zeroed by the stream before each batch, with the next list's length).
struct AdaptSum {
    unsigned long long ret_pixels, ret_sum_q, ret_above, ret_tiles, pixel_frames;
    unsigned ret_max_q, pad;
    unsigned long long act_pixels, act_sum_q, act_above;    // from here on: per batch
    unsigned act_max_q, n_next;
};
struct AdaptArgs {
    unsigned n_list;            // tiles in the launch's list (KParams::tile_perm, KParams::queue_tiles)
    unsigned per_wave;          // tiles a wave takes in turn, 1..kAdaptTilesPerWave (adapt_tiles_per_wave)
    int n_tiles;                // the tile grid (tile_frames' length)
    int n_after;                // n0 + the frames done after this pass: the stop rule's n (0: a batch's earlier launch, no verdict)
    unsigned frames_after;      // the frames this call has given the list's tiles after this pass
    unsigned target_q;
    unsigned* tile_frames;      // per tile of the grid: frames received in this call
    unsigned* next;             // the tiles that stay active (any order)
    AdaptSum* sum;
};
constexpr int kAdaptTilesPerWave = 8;
// Tiles per wave for a list of n tiles: 8 for long lists (a set of summary atomics per 32 tiles), fewer for short
// ones, whose pass is a chain of dependent loads per wave and not a stream (a list of 736 tiles took 139 us at 8 per
// wave, the time of one wave's 8 tiles x 8 load groups): about 1,000 blocks at most either way.
inline unsigned adapt_tiles_per_wave(unsigned n) { return std::min(8u, std::max(1u, n / 4096u)); }
constexpr int kAdaptFrames = 8;   // frames per load group (as k_accum_frames' long shape), then one at a time
// One wave per tile and turn; lane w owns the pixel the render kernel's queue id w of that tile
// maps to (the same tw / th / tile_shift arithmetic and the same bounds), folds the batch's
// colours from the scratch planes in frame order (pti::accumulate, ptn::add_sample: what
// k_accum_frames<.., true> does for the pixel), stores image and moments, and quantises its own
// pixel; the wave reduces.  A wave takes a.per_wave tiles in turn, four list entries apart, keeps
// its sums in registers and its surviving tiles in LDS; at the end the block adds its four
// waves' integers into the summary block and reserves its stretch of the next list -- one set
// of atomics per block (32 tiles of a long list), not per tile (the lesson of k_noise).  Every field is an
// integer: exact in any order.  A list entry outside the tile grid is skipped.
__global__ __launch_bounds__(256) void k_accum_retire(KParams p, AdaptArgs a) {
    const unsigned wave = threadIdx.x >> 6, w = threadIdx.x & 63u;
    const int tsh = p.tile_shift, tw = 8 << tsh, th = 8 >> tsh;
    const int tiles_x = (p.W + tw - 1) >> (3 + tsh);
    const size_t n = (size_t)p.rows_local * (size_t)p.W;
    unsigned long long r_sum = 0, a_sum = 0, pf = 0;
    unsigned r_px = 0, r_ab = 0, r_mx = 0, r_tiles = 0, a_px = 0, a_ab = 0, a_mx = 0, n_surv = 0;
    __shared__ unsigned s_surv[4][kAdaptTilesPerWave];
    for (unsigned j = 0; j < a.per_wave && j < (unsigned)kAdaptTilesPerWave; j++) {    // (s_surv holds kAdaptTilesPerWave)
        const unsigned li = (blockIdx.x * a.per_wave + j) * 4u + wave;
        if (li >= a.n_list) break;              // wave-uniform
        const unsigned pk = p.tile_perm[li];
        const int tx = (int)(pk & 0xffffu), ty = (int)(pk >> 16);
        const long long tile = (long long)ty * tiles_x + tx;
        if (tx >= tiles_x || tile >= (long long)a.n_tiles) continue;     // wave-uniform: not a tile of this grid
        const int cx = tx * tw + (int)(w & (unsigned)(tw - 1));
        const int crow = ty * th + (int)(w >> (3 + tsh));
        const bool on = cx < p.W && crow < p.rows_local && cx < p.x_limit && p.row0 + crow * p.row_stride < p.y_limit;
        const size_t idx = on ? (size_t)crow * (size_t)p.W + (size_t)cx : 0;
        float4 acc = (on && p.acc_first) ? p.accum[idx] : make_float4(0, 0, 0, 0);
        float2 mom = (on && p.acc_first) ? p.moments[idx] : make_float2(0, 0);
        int k = 0;
        for (; k + kAdaptFrames <= p.n_frames; k += kAdaptFrames) {
            f3 v[kAdaptFrames];
#pragma unroll
            for (int u = 0; u < kAdaptFrames; u++)
                v[u] = on ? nt_load3(p.rgb + 3 * ((size_t)(k + u) * n + idx)) : mk(0, 0, 0);
#pragma unroll
            for (int u = 0; u < kAdaptFrames; u++) {
                acc = accumulate(acc, v[u], p.frame_first + k + u, k + u > 0 || p.acc_first == 1);
                ptn::add_sample(mom.x, mom.y, ptn::luminance(v[u].x, v[u].y, v[u].z));
            }
        }
        for (; k < p.n_frames; k++) {
            const f3 v = on ? nt_load3(p.rgb + 3 * ((size_t)k * n + idx)) : mk(0, 0, 0);
            acc = accumulate(acc, v, p.frame_first + k, k > 0 || p.acc_first == 1);
            ptn::add_sample(mom.x, mom.y, ptn::luminance(v.x, v.y, v.z));
        }
        if (on) {
            p.accum[idx] = acc;
            p.moments[idx] = mom;
        }
        unsigned px = on ? 1u : 0u;
        for (int off = 32; off > 0; off >>= 1) px += __shfl_xor(px, off, 64);
        pf += (unsigned long long)px * (unsigned long long)p.n_frames;
        if (!a.n_after || !px) continue;        // wave-uniform: no verdict yet, or a tile without a footprint pixel
        const unsigned q = on ? ptn::quantise(mom.x, mom.y, a.n_after) : 0u;
        unsigned sq = q, ab = (on && q > a.target_q) ? 1u : 0u, mx = q;    // a tile's sum: at most 64 * 2^22
        for (int off = 32; off > 0; off >>= 1) {
            sq += __shfl_xor(sq, off, 64);
            ab += __shfl_xor(ab, off, 64);
            const unsigned o = __shfl_xor(mx, off, 64);
            mx = o > mx ? o : mx;
        }
        if (w == 0) a.tile_frames[tile] = a.frames_after;
        if (ptn::tile_retires(sq, px, a.target_q)) {
            r_sum += sq, r_px += px, r_ab += ab, r_mx = mx > r_mx ? mx : r_mx, r_tiles++;
        } else {
            a_sum += sq, a_px += px, a_ab += ab, a_mx = mx > a_mx ? mx : a_mx;
            if (w == 0) s_surv[wave][n_surv] = pk;
            n_surv++;
        }
    }
    // the block's four waves: their sums (every lane of a wave holds the wave's) through LDS
    __shared__ unsigned long long s_u64[4][3];
    __shared__ unsigned s_u32[4][8], s_base;
    if (w == 0) {
        s_u64[wave][0] = r_sum, s_u64[wave][1] = a_sum, s_u64[wave][2] = pf;
        s_u32[wave][0] = r_px, s_u32[wave][1] = r_ab, s_u32[wave][2] = r_mx, s_u32[wave][3] = r_tiles;
        s_u32[wave][4] = a_px, s_u32[wave][5] = a_ab, s_u32[wave][6] = a_mx, s_u32[wave][7] = n_surv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = n_surv;
        for (unsigned o = 1; o < 4; o++) {
            r_sum += s_u64[o][0], a_sum += s_u64[o][1], pf += s_u64[o][2];
            r_px += s_u32[o][0], r_ab += s_u32[o][1], r_tiles += s_u32[o][3], a_px += s_u32[o][4], a_ab += s_u32[o][5];
            r_mx = s_u32[o][2] > r_mx ? s_u32[o][2] : r_mx;
            a_mx = s_u32[o][6] > a_mx ? s_u32[o][6] : a_mx;
            total += s_u32[o][7];
        }
        if (pf) atomicAdd(&a.sum->pixel_frames, pf);
        if (r_tiles) {
            atomicAdd(&a.sum->ret_pixels, (unsigned long long)r_px);
            atomicAdd(&a.sum->ret_sum_q, r_sum);
            atomicAdd(&a.sum->ret_above, (unsigned long long)r_ab);
            atomicAdd(&a.sum->ret_tiles, (unsigned long long)r_tiles);
            atomicMax(&a.sum->ret_max_q, r_mx);
        }
        if (total) {
            atomicAdd(&a.sum->act_pixels, (unsigned long long)a_px);
            atomicAdd(&a.sum->act_sum_q, a_sum);
            atomicAdd(&a.sum->act_above, (unsigned long long)a_ab);
            atomicMax(&a.sum->act_max_q, a_mx);
            s_base = atomicAdd(&a.sum->n_next, total);     // the block's stretch of the next list
        }
    }
    __syncthreads();
    if (w == 0 && n_surv) {         // (n_surv > 0 in any wave means total > 0: s_base was written)
        unsigned at = s_base;
        for (unsigned o = 0; o < wave; o++) at += s_u32[o][7];
        // at + n_surv <= the sum of all blocks' survivors <= n_list <= the list buffers' n_tiles entries
        for (unsigned i = 0; i < n_surv; i++) a.next[at + i] = s_surv[wave][i];
    }
}

}  // namespace
