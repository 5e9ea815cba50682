// pt_ctx_io.h -- a section of the pt_render.hip translation unit, not a general-purpose header: pt_render.hip
// includes it once, after pt_ctx_denoise.h.  How the image leaves and enters the context: reading and writing the
// RGBA32F image, its 8-bit ACES view (rgba8, stage_ok), pt_present_*, the device pointer and row copy a group uses,
// the launch timing and the stream.
extern "C" {
// The view of the current image in rgba8, for a caller that shows it: written by the last render's accumulate pass
// when the caller read or presented after the render before it (stage_ok), else the ACES pass here.
static hipError_t view_image(pt_ctx* c, long long n) {
    if (n > 0 && !c->stage_ok) {
        launch_aces(c->stream, c->accum, c->rgba8, n);
        if (hipError_t e = hipGetLastError()) return e;
    }
    c->stage_ok = c->presented = true;     // rgba8 is the view of the current image
    return hipSuccess;
}

int pt_read_rgba32f(pt_ctx* c, float* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    size_t need = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    if (bytes < need) return fail(c, PT_E_ARG, "destination too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->accum, need, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_write_rgba32f(pt_ctx* c, const float* src, size_t bytes) {
    if (!c || !src) return PT_E_ARG;
    c->stage_ok = false;
    size_t need = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    if (bytes < need) return fail(c, PT_E_ARG, "source too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->accum, src, need, hipMemcpyHostToDevice));
    return PT_OK;
}

int pt_read_rgba8_aces(pt_ctx* c, unsigned char* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    long long n = (long long)c->rows_local * c->cfg.width;
    if (bytes < (size_t)n * 4) return fail(c, PT_E_ARG, "destination too small");
    if (n == 0) return PT_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, view_image(c, n));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->rgba8, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

// Asynchronous presentation for a viewer that shows every frame (ogl_path_trace.h:189-192
// draws each frame's texture on the GPU that rendered it; a headless caller reads it back).
// begin: the ACES epilogue of the current image on the context stream (after every render
// issued so far and its running mean), then a copy into pinned host memory on a separate
// stream, so renders issued after it run while the image crosses PCIe.  end: waits for that
// copy and hands out the pinned pixels.
int pt_present_begin(pt_ctx* c, int buf) {
    if (!c) return PT_E_ARG;
    if (buf < 0 || buf >= kPresentBufs) return fail(c, PT_E_ARG, "present buffer must be 0..3");
    const long long n = (long long)c->rows_local * c->cfg.width;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!c->present_host[buf]) {
        HIPCHK(c, hipHostMalloc((void**)&c->present_host[buf], std::max<long long>(n, 1) * sizeof(uchar4),
                                hipHostMallocDefault));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_copied[buf], hipEventDisableTiming));
    }
    // a buffer begun again before its end: its previous copy must land first
    if (c->present_pending[buf]) HIPCHK(c, hipEventSynchronize(c->ev_copied[buf]));
    c->present_pending[buf] = false;
    HIPCHK(c, view_image(c, n));
    // the copy on the context stream itself: a copy stream waiting on an event started each
    // copy about 150 us after the view was ready (one-frame loop with lag 2: 0.578 -> 0.537
    // ms per frame); the next render's accumulate pass, which rewrites the view, follows it
    if (n > 0)
        HIPCHK(c, hipMemcpyAsync(c->present_host[buf], c->rgba8, (size_t)n * sizeof(uchar4), hipMemcpyDeviceToHost,
                                 c->stream));
    HIPCHK(c, hipEventRecord(c->ev_copied[buf], c->stream));
    c->present_pending[buf] = true;
    return PT_OK;
}

int pt_present_end(pt_ctx* c, int buf, const unsigned char** pixels) {
    if (!c || !pixels) return PT_E_ARG;
    if (buf < 0 || buf >= kPresentBufs) return fail(c, PT_E_ARG, "present buffer must be 0..3");
    if (!c->present_pending[buf]) return fail(c, PT_E_STATE, "pt_present_end without pt_present_begin");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipEventSynchronize(c->ev_copied[buf]));
    c->present_pending[buf] = false;
    *pixels = c->present_host[buf];
    return PT_OK;
}

int pt_accum_device(pt_ctx* c, void** ptr, size_t* bytes) {
    if (!c) return PT_E_ARG;
    c->stage_ok = false;   // the caller may write the image through this pointer
    if (ptr) *ptr = c->accum;
    if (bytes) *bytes = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    return PT_OK;
}

int pt_copy_rows_device(pt_ctx* c, void* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    size_t need = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    if (bytes < need) return fail(c, PT_E_ARG, "destination too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpyAsync(dst, c->accum, need, hipMemcpyDeviceToDevice, c->stream));
    return pt_sync(c);
}

int pt_timing(pt_ctx* c, double* total_ms, int* n, int reset) {
    if (!c) return PT_E_ARG;
    if (total_ms) *total_ms = c->total_ms;
    if (n) *n = c->n_launches;
    if (reset) { c->total_ms = 0.0; c->n_launches = 0; }
    return PT_OK;
}

int pt_stream(pt_ctx* c, void** s) {
    if (!c || !s) return PT_E_ARG;
    c->stage_ok = false;   // ... or queue work on this stream that does
    *s = (void*)c->stream;
    return PT_OK;
}
}  // extern "C"
