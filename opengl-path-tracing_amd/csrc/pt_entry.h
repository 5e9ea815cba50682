// pt_entry.h -- what the entry points of the ray-batch units (pt_query_kernels.hip, pt_trace_kernels.hip,
// pt_camera_kernels.hip, pt_film_kernels.hip) share on the host side: the HIP error return, the argument
// checks with their messages, and the device buffers of a host-staged call.  For HIP units only; errors go through
// pt__query_fail into the context's error string.  In an unnamed namespace on purpose: everything here has internal
// linkage in each unit, as its own copy had, and the library exports nothing new.
#pragma once

#include "pt_camera.h"
#include "pt_trace_launch.h"

#include <climits>
#include <string>

namespace pte {
namespace {

inline int hip_fail(pt_ctx* c, const char* what, hipError_t e) {
    return pt__query_fail(c, PT_E_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}
// (the message names the call as written: the tests read it)
#define PTCHK(ctx, call)                                            \
    do {                                                            \
        hipError_t e_ = (call);                                     \
        if (e_ != hipSuccess) return pte::hip_fail(ctx, #call, e_); \
    } while (0)

inline int check_scene(pt_ctx* c, const ptq::CtxView& q, const char* who) {
    if (!q.scene_ok) return pt__query_fail(c, PT_E_STATE, (std::string(who) + " before pt_upload_scene").c_str());
    return PT_OK;
}

inline int check_frames(pt_ctx* c, int frame_first, int n_frames, int accumulate_first) {
    if (frame_first < 1 || n_frames < 1) return pt__query_fail(c, PT_E_ARG, "frame_first and n_frames must be >= 1");
    if (frame_first > INT_MAX - n_frames) return pt__query_fail(c, PT_E_ARG, "frame_first + n_frames overflows");
    if (accumulate_first != 0 && accumulate_first != 1) return pt__query_fail(c, PT_E_ARG, "accumulate_first must be 0 or 1");
    return PT_OK;
}

inline int check_camera(pt_ctx* c, const pt_camera* cam) {
    if (ptcam::validate(cam) != PT_OK)
        return pt__query_fail(c, PT_E_ARG, "camera: null, unknown model or flag, size out of range, or a bad aperture, "
                                           "focus or ortho_width for its model");
    return PT_OK;
}

// The device buffers of a call that stages host arrays: allocate, copy in, (enqueue,) copy out.  The first HIP error
// is kept in `e` and every later step is skipped.  On scope exit, after an error the stream is synchronised first --
// nothing in flight may still read the buffers -- and then everything is freed.
struct Staged {
    hipStream_t s;
    hipError_t e = hipSuccess;
    void* p[3] = {nullptr, nullptr, nullptr};
    int n = 0;
    explicit Staged(hipStream_t stream) : s(stream) {}
    Staged(const Staged&) = delete;
    Staged& operator=(const Staged&) = delete;
    ~Staged() {
        if (e != hipSuccess) (void)hipStreamSynchronize(s);
        for (int k = 0; k < n; k++) (void)hipFree(p[k]);
    }
    bool ok() const { return e == hipSuccess; }
    void* alloc(size_t bytes) {            // at most three per call
        if (e == hipSuccess) e = hipMalloc(&p[n++], bytes);
        return e == hipSuccess ? p[n - 1] : nullptr;
    }
    void in(void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    }
    void out(void* dst, const void* src, size_t bytes) {      // ... and waits for it
        if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
};

}  // namespace
}  // namespace pte
