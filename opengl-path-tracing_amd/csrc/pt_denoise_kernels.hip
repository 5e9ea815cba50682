// pt_denoise_kernels.hip -- the device half of the denoised view (include/pt_api.h: pt_denoise): the
// guide pack, the state prep and the a-trous iteration, a 5 x 5 stencil over ping-pong float4 (r, g, b, v) planes (by
// its traffic a memory-bound pass; as measured, bound by the vector arithmetic of its 25 weights -- DESIGN.md §11.4).
// One thread per pixel runs ptd::filter_px (pt_denoise.h), so a pixel's taps keep the order the host twin and the
// numpy model take them in.  A translation unit of its own: the render kernels' code object stays as it is.
//
// An iteration at step s reads 25 taps of 48 B (state + two guide quads) per pixel.  Two ways to get them:
//   direct  every tap a global load.  For a fixed tap a row of 64 lanes reads 64 consecutive pixels at any step, so the
//           loads coalesce; the reuse between neighbouring pixels is left to L1 / L2.
//   LDS     a workgroup of 64 x 4 threads takes 64 consecutive columns of 4 rows that lie s apart (a residue class of
//           the rows, so the vertical taps of its pixels are each other's rows), and stages 64 + 4s columns x 8 rows in
//           LDS: 2.1 (s = 1) to 4 (s = 16) loads per pixel instead of 25.  The columns stay consecutive, so staging
//           coalesces and a wave's 64 lanes read 64 consecutive 16-B LDS words per tap.  At s = 16 the tile is 48 KiB;
//           beyond, the halo outgrows the tile and the taps mostly fall outside the image anyway: direct loads.
// The variance prefilter's 3 x 3 unit offsets are not in a residue-class tile for s > 1: it reads global memory (16 B
// per tap, the state plane only) in both variants.
#include "pt_denoise_launch.h"

namespace ptd {
namespace {

constexpr int kTX = 64, kTY = 4;      // a workgroup's pixels: one wave per row

PTD_HD Px px_of(const float4& v) { return {v.x, v.y, v.z, v.w}; }
PTD_HD Gd gd_of(const float4& a, const float4& b) { return {a.x, a.y, a.z, a.w, b.x, b.y, b.z}; }

struct IterArgs {
    const float4* in;
    float4* out;
    const float4* g0;
    const float4* g1;
    const float4* alpha_from;
    int W, H, xl, yl, step, lum_on;
    K k;
};

struct DirectSrc {
    const float4* st;
    const float4* g0;
    const float4* g1;
    int W, xl, yl, x, y, step;
    __device__ bool inside(int qx, int qy) const { return (unsigned)qx < (unsigned)xl && (unsigned)qy < (unsigned)yl; }
    __device__ Px state(int qx, int qy) const { return px_of(st[(size_t)qy * (size_t)W + (size_t)qx]); }
    __device__ Px tap_state(int dx, int dy) const { return state(x + step * dx, y + step * dy); }
    __device__ Gd tap_guide(int dx, int dy) const {
        const size_t i = (size_t)(y + step * dy) * (size_t)W + (size_t)(x + step * dx);
        return gd_of(g0[i], g1[i]);
    }
};

// the tile: three planes of `cells` quads; a tap of the thread at (tx, ty) is at row ty + 2 + dy, column
// tx + 2 * step + step * dx -- rows 0 .. kTY + 3 and columns 0 .. kTX + 4 * step - 1 for dx, dy in -2 .. 2
struct LdsSrc {
    const float4* st;       // global: the variance prefilter's unit offsets
    const float4* tile;
    int W, xl, yl, x, y, step, cols, cells, at;
    __device__ bool inside(int qx, int qy) const { return (unsigned)qx < (unsigned)xl && (unsigned)qy < (unsigned)yl; }
    __device__ Px state(int qx, int qy) const { return px_of(st[(size_t)qy * (size_t)W + (size_t)qx]); }
    __device__ Px tap_state(int dx, int dy) const { return px_of(tile[at + dy * cols + step * dx]); }
    __device__ Gd tap_guide(int dx, int dy) const {
        const int c = at + dy * cols + step * dx;
        return gd_of(tile[cells + c], tile[2 * cells + c]);
    }
};

__device__ __forceinline__ void store_px(const IterArgs& a, size_t i, const Px& o) {
    a.out[i] = make_float4(o.r, o.g, o.b, a.alpha_from ? a.alpha_from[i].w : o.v);
}

__global__ __launch_bounds__(kTX * kTY) void k_denoise_direct(IterArgs a) {
    const int x = (int)blockIdx.x * kTX + (int)(threadIdx.x & 63u), y = (int)blockIdx.y * kTY + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t i = (size_t)y * (size_t)a.W + (size_t)x;
    const DirectSrc s = {a.in, a.g0, a.g1, a.W, a.xl, a.yl, x, y, a.step};
    store_px(a, i, s.inside(x, y) ? filter_px(s, x, y, a.step, a.lum_on != 0, a.k) : px_of(a.in[i]));
}

__global__ __launch_bounds__(kTX * kTY) void k_denoise_lds(IterArgs a) {
    extern __shared__ float4 tile[];
    const int step = a.step, cols = kTX + 4 * step, cells = cols * (kTY + 4);
    // block row b: the rows of residue b % step in the band of kTY * step rows number b / step
    const int band = (int)blockIdx.y / step, ybase = band * step * kTY + ((int)blockIdx.y - band * step);
    const int x0 = (int)blockIdx.x * kTX;
    for (int c = (int)threadIdx.x; c < cells; c += kTX * kTY) {
        const int row = c / cols, col = c - row * cols;
        const int gx = x0 - 2 * step + col, gy = ybase + step * (row - 2);
        float4 s = make_float4(0, 0, 0, 0), u = s, v = s;
        if ((unsigned)gx < (unsigned)a.xl && (unsigned)gy < (unsigned)a.yl) {   // inside the footprint, so inside the image
            const size_t i = (size_t)gy * (size_t)a.W + (size_t)gx;
            s = a.in[i], u = a.g0[i], v = a.g1[i];
        }
        tile[c] = s, tile[cells + c] = u, tile[2 * cells + c] = v;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & 63u), ty = (int)(threadIdx.x >> 6);
    const int x = x0 + tx, y = ybase + step * ty;
    if (x >= a.W || y >= a.H) return;
    const size_t i = (size_t)y * (size_t)a.W + (size_t)x;
    const LdsSrc s = {a.in, tile, a.W, a.xl, a.yl, x, y, step, cols, cells, (ty + 2) * cols + tx + 2 * step};
    store_px(a, i, s.inside(x, y) ? filter_px(s, x, y, step, a.lum_on != 0, a.k) : px_of(a.in[i]));
}

__global__ __launch_bounds__(256) void k_denoise_pack(const float4* __restrict__ n, const float4* __restrict__ al,
                                                      const float4* __restrict__ z, float4* __restrict__ g0,
                                                      float4* __restrict__ g1, long long px) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= px) return;
    const float4 nn = n[i], aa = al[i];
    g0[i] = make_float4(nn.x, nn.y, nn.z, z[i].x);
    g1[i] = make_float4(aa.x, aa.y, aa.z, 0.0f);
}

struct PrepArgs {
    const float4* accum;
    const float2* moments;
    const unsigned* tile_frames;
    float4* state;
    int W, H, n, extra, tile_shift, tiles_x;
};
__global__ __launch_bounds__(256) void k_denoise_prep(PrepArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.W * a.H) return;
    const float4 c = a.accum[i];
    float v = 0.0f;
    if (a.moments) {
        int n = a.n;
        if (a.tile_frames) {    // per-tile counts after an adaptive run
            const int y = (int)(i / a.W), x = (int)(i - (long long)y * a.W);
            n = (int)a.tile_frames[(y >> (3 - a.tile_shift)) * a.tiles_x + (x >> (3 + a.tile_shift))] + a.extra;
        }
        const float2 m = a.moments[i];
        v = n >= 2 ? variance(m.x, m.y, n) : 0.0f;
    }
    a.state[i] = make_float4(c.x, c.y, c.z, v);
}

}  // namespace

void launch_pack(hipStream_t s, const float4* n, const float4* a, const float4* z, float4* g0, float4* g1, long long px) {
    if (px <= 0) return;
    hipLaunchKernelGGL(k_denoise_pack, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, n, a, z, g0, g1, px);
}

void launch_prep(hipStream_t s, const Image& im, const float4* accum, const float2* moments, int n,
                 const unsigned* tile_frames, int extra, int tile_shift, int tiles_x, float4* state) {
    const long long px = (long long)im.W * im.H;
    if (px <= 0) return;
    const PrepArgs a = {accum, moments, tile_frames, state, im.W, im.H, n, extra, tile_shift, tiles_x};
    hipLaunchKernelGGL(k_denoise_prep, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, a);
}

void launch_iter(hipStream_t s, const Image& im, const float4* in, float4* out, const float4* g0, const float4* g1,
                 const float4* alpha_from, int step, bool lum_on, const K& k, int variant) {
    if (im.W <= 0 || im.H <= 0) return;
    const IterArgs a = {in, out, g0, g1, alpha_from, im.W, im.H, im.x_limit, im.y_limit, step, lum_on ? 1 : 0, k};
    const unsigned bx = (unsigned)((im.W + kTX - 1) / kTX);
    if (variant != kDirect && step <= kLdsMaxStep) {
        const unsigned bands = (unsigned)((im.H + kTY * step - 1) / (kTY * step));
        const size_t bytes = (size_t)(kTX + 4 * step) * (kTY + 4) * 3 * sizeof(float4);
        hipLaunchKernelGGL(k_denoise_lds, dim3(bx, bands * (unsigned)step), dim3(kTX * kTY), bytes, s, a);
    } else {
        hipLaunchKernelGGL(k_denoise_direct, dim3(bx, (unsigned)((im.H + kTY - 1) / kTY)), dim3(kTX * kTY), 0, s, a);
    }
}

}  // namespace ptd
