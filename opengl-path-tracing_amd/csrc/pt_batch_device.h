// pt_batch_device.h -- what the ray-batch units (pt_query_kernels.hip, pt_trace_kernels.hip, pt_camera_kernels.hip,
// pt_film_kernels.hip) share on the device side and in their launchers: the workgroup shape, the scene
// accessor ptq::cast and ptt::shade are templated on, the rank of a lane in a ballot, the argument-segment read, and
// the sizing of a persistent grid.  For HIP units only.  Every unit keeps its own kernel, its own argument struct and,
// where it has them, the LDS staging prologue and the refill loop: §16.2 has the compiler output that says why.
// Everything here is inlined or has internal linkage: the library's symbols do not change with it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ptb {

constexpr int kThreads = 256;              // a workgroup: 4 waves
constexpr int kWaves = kThreads / 64;
constexpr int kMaxDevices = 64;

// The scene as a kernel reads it from its argument struct `a`.  STAGED: the first a.n_top node records come from the
// LDS copy the kernel made (lo plane at top[i], hi plane at top[a.n_top + i]); only then is a.n_top named.  mat() is
// instantiated only where a path is shaded, so the query's arguments need no `mats`.
template <class Args, bool STAGED = false>
struct DevScene {
    const Args& a;
    const float4* top = nullptr;
    __device__ __forceinline__ int n_nodes() const { return a.n_nodes; }
    __device__ __forceinline__ int n_spheres() const { return a.n_spheres; }
    __device__ __forceinline__ bool scene_fast() const { return a.scene_fast != 0; }
    __device__ __forceinline__ void node(int i, float4& lo, float4& hi) const {
        if constexpr (STAGED) {
            if (i < a.n_top) {
                lo = top[i];
                hi = top[a.n_top + i];
                return;
            }
        }
        lo = a.nodes[2 * (size_t)i];
        hi = a.nodes[2 * (size_t)i + 1];
    }
    __device__ __forceinline__ float4 tri(int slot, int k) const { return a.tris[4 * (size_t)slot + k]; }
    __device__ __forceinline__ float4 sphere(int i, int k) const { return a.spheres[2 * (size_t)i + k]; }
    __device__ __forceinline__ float4 leaf_tris(int pair) const { return a.leaf_tris[pair]; }
    __device__ __forceinline__ float4 mat(int i, int k) const { return a.mats[3 * (size_t)i + k]; }
};

// Number of set bits of m below this lane.
__device__ __forceinline__ int rank_in(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// The T at byte OFFSET of the kernel's argument struct, read from the argument segment where it is used, by vector
// loads (every lane the same words): nothing of it is live during the walk.  Read as a by-value argument the camera
// stayed in SGPRs across the whole refill loop, k_trace_camera needed 106 SGPRs (112 allocated) against k_trace's 96,
// and a SIMD then held 6 of its waves, not the 7 the runtime's occupancy query reports: the last seventh of the
// persistent grid ran as a tail, 28% slower on both scenes measured (one session's measurement, with
// the grid-cap comparison that located it).  Scalar loads at this place still peaked at 98 to 106.  The empty asm
// makes the address opaque and per-lane, so the loads are neither hoisted out of the loop nor turned back into scalar
// ones.
// Relies on the argument struct being the kernel's first and only parameter, so that it starts the argument segment
// (each kernel asserts it below its definition) -- and on nothing else: should the compiler one day see through the
// asm, the result is the same words from the same place, only with more SGPRs again (the resource tables of
// tools/camera_measure.py and tools/film_measure.py show it).  A word the kernel needs at every take and store
// (cam.W) it reads directly beside this copy, so that it stays a scalar.
template <class T, size_t OFFSET>
__device__ __forceinline__ T load_arg() {
    typedef const __attribute__((address_space(4))) uint32_t* kernarg_words;
    static_assert(OFFSET % 4 == 0 && sizeof(T) % 4 == 0, "whole words");
    kernarg_words w = (kernarg_words)__builtin_amdgcn_kernarg_segment_ptr() + OFFSET / 4;
    asm volatile("" : "+v"(w));
    union { T t; uint32_t u[sizeof(T) / 4]; } c;
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); k++) c.u[k] = w[k];
    return c.t;
}

// ---------------------------------------------------------------------- launchers (host)
// Compute units of a device; asked of the runtime once per device.
static inline int compute_units(int device) {
    static int cache[kMaxDevices];
    if (device < 0 || device >= kMaxDevices) return 256;
    if (cache[device] == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
        cache[device] = cus;
    }
    return cache[device];
}

// One kernel's row of its unit's cache, zero until asked: a unit keeps `static ptb::Resident cache[its kernels]`.
typedef int Resident[kMaxDevices];

// Workgroups of kernel `fn` that a device holds at once: compute units x workgroups per unit at its occupancy.
// Asked of the runtime once per kernel and device.
static inline int resident_blocks(const void* fn, Resident& row, int device) {
    if (device < 0 || device >= kMaxDevices) return 1024;
    if (row[device] == 0) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kThreads, 0) != hipSuccess || per_cu < 1) per_cu = 1;
        row[device] = per_cu * compute_units(device);
    }
    return row[device];
}

// The workgroups of a persistent grid over n items: what is resident, at most one item per thread, at most grid_cap
// where that is set (the debug hooks' cap; 0 = none).
static inline unsigned persistent_grid(const void* fn, Resident& row, int device, long long n, int grid_cap) {
    long long blocks = resident_blocks(fn, row, device);
    const long long want = (n + kThreads - 1) / kThreads;
    if (want < blocks) blocks = want;
    if (grid_cap > 0 && grid_cap < blocks) blocks = grid_cap;
    return (unsigned)blocks;
}

}  // namespace ptb
