// pt_ctx_denoise.h -- a section of the pt_render.hip translation unit, not a general-purpose header: pt_render.hip
// includes it once, after pt_ctx_noise.h.  The denoised view: the guide launch and the guide planes,
// pt_denoise*, the reads of the result and the guides, and the pt__denoise_* measurement hooks.  The filter's kernels
// are pt_denoise_kernels.hip's (pt_denoise_launch.h).
extern "C" {
// One launch of a guide render on the context stream: the render kernel in display mode `mode` over the whole tile
// grid, then the plain accumulate pass into `plane` instead of the image.  Planned like an adaptive launch -- a
// frame-split launch on the generic line of its key, on the context's own stream, never counting -- and invisible to
// the context: no tile costs, no moments, no ACES view, no timing events, and none of the launch bookkeeping
// (pt_debug_launches, pt_debug_sweep, pt_debug_pool, the sort cadence) moves.
static int enqueue_guide(pt_ctx* c, const ptl::State& st, int mode, int frame_first, int n_frames, int acc_first, float4* plane) {
    ptl::LaunchPlan pl;
    KParams p;
    int rc = plan_plain_split(c, plan_image(c), st, frame_first, n_frames, acc_first, pl, p);
    if (rc) return rc;
    p.accum = plane;
    p.mode = mode;
    p.tile_cost = nullptr;
    p.moments = nullptr;
    rc = launch_render(c, pl, p, c->stream, false, false, false);
    if (rc) return rc;
    const KParamsKernel acc = pl.accum_long ? k_accum_frames<kAccumPixLong, kAccumFramesLong> : k_accum_frames<kAccumPix, 1>;
    hipLaunchKernelGGL(acc, dim3(pl.accum_blocks), dim3(256), 0, c->stream, p);
    HIPCHK(c, hipGetLastError());
    return PT_OK;
}

// The guide planes of `frames` frames: display modes 2, 3 and 4 rendered as pt_render(1, frames, 0) would, each into a
// zeroed plane (pixels outside the dispatch footprint stay zero), then packed.
static int render_guides(pt_ctx* c, int frames) {
    const size_t bytes = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    float4* raw[3] = {c->dn_state[0], c->dn_state[1], c->dn_out};
    // not counting; split as with the moments on (the pass below keeps none); planned like an adaptive launch
    const ptl::State st = {false, true, false, true};
    for (int m = 0; m < 3; m++) {
        HIPCHK(c, hipMemsetAsync(raw[m], 0, bytes, c->stream));
        int done = 0;
        while (done < frames) {
            const int n = ptl::launch_frames(c->sf, c->tun, plan_image(c), st, frames - done);
            int rc = enqueue_guide(c, st, 2 + m, 1 + done, n, done ? 1 : 0, raw[m]);
            if (rc) return rc;
            done += n;
        }
    }
    ptd::launch_pack(c->stream, raw[0], raw[1], raw[2], c->dn_guide[0], c->dn_guide[1],
                     (long long)c->rows_local * c->cfg.width);
    HIPCHK(c, hipGetLastError());
    return PT_OK;
}

int pt_denoise_async(pt_ctx* c, const pt_denoise_params* params, pt_denoise_info* info) {
    if (!c) return PT_E_ARG;
    pt_denoise_params dp;
    pt_denoise_defaults(&dp);
    if (params) dp = *params;
    if (dp.iterations < 1 || dp.iterations > ptd::kMaxIterations) return fail(c, PT_E_ARG, "pt_denoise: iterations must be 1..8");
    if (dp.guide_frames < 1) return fail(c, PT_E_ARG, "pt_denoise: guide_frames must be >= 1");
    if (!c->scene_ok) return fail(c, PT_E_STATE, "pt_denoise before pt_upload_scene");
    if (c->cfg.world > 1)
        return fail(c, PT_E_STATE, "pt_denoise on a row-split context: its interleaved rows have no neighbours (groups are out of scope)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t px = (size_t)c->rows_local * c->cfg.width;     // world == 1: every row
    if (!c->dn_out) {
        float4** planes[5] = {&c->dn_guide[0], &c->dn_guide[1], &c->dn_state[0], &c->dn_state[1], &c->dn_out};
        for (float4** pl : planes)
            if (!*pl) HIPCHK(c, hipMalloc(pl, px * sizeof(float4)));
    }
    if (c->dn_timing)
        for (hipEvent_t& e : c->dn_ev)
            if (!e) HIPCHK(c, hipEventCreate(&e));
    int ev = 0;
    const auto mark = [&]() { if (c->dn_timing) (void)hipEventRecord(c->dn_ev[ev++], c->stream); };
    mark();
    const bool render = !c->guides_ok || c->guides_frames != dp.guide_frames;
    if (render) {
        c->guides_ok = false;
        c->dn_done = false;     // (the rendered planes pass through the result's plane)
        int rc = render_guides(c, dp.guide_frames);
        if (rc) return rc;
        c->guides_ok = true;
        c->guides_frames = dp.guide_frames;
    }
    mark();
    const bool guided = c->moments != nullptr && c->mom_frames >= 2;
    KParams ip;
    fill_image(ip, c);
    const ptd::Image im = {ip.W, ip.H, ip.x_limit, ip.y_limit};
    const bool per_tile = guided && c->mom_mixed && c->d_tile_frames;
    ptd::launch_prep(c->stream, im, c->accum, guided ? c->moments : nullptr, c->mom_frames,
                     per_tile ? c->d_tile_frames : nullptr, c->mom_frames - c->adapt_done, c->tile_shift, c->tiles_x,
                     c->dn_state[0]);
    mark();
    const ptd::K k = {ptd::inv_sq(dp.sigma_lum), ptd::inv_sq(dp.sigma_normal), ptd::inv_sq(dp.sigma_albedo),
                      ptd::inv_sq(dp.sigma_depth)};
    for (int i = 0; i < dp.iterations; i++) {
        const bool last = i + 1 == dp.iterations;
        ptd::launch_iter(c->stream, im, c->dn_state[i & 1], last ? c->dn_out : c->dn_state[(i + 1) & 1], c->dn_guide[0],
                         c->dn_guide[1], last ? c->accum : nullptr, 1 << i, guided, k, c->dn_variant);
        mark();
    }
    c->dn_ev_n = ev;
    HIPCHK(c, hipGetLastError());
    c->dn_done = true;
    if (info) *info = {guided ? 1 : 0, render ? 1 : 0, dp.iterations, c->moments ? c->mom_frames : 0};
    return PT_OK;
}

int pt_denoise(pt_ctx* c, const pt_denoise_params* params, pt_denoise_info* info) {
    int rc = pt_denoise_async(c, params, info);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_read_denoised_rgba32f(pt_ctx* c, float* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    if (!c->dn_done) return fail(c, PT_E_STATE, "no denoised image (pt_denoise first)");
    const size_t need = (size_t)c->rows_local * c->cfg.width * sizeof(float4);
    if (bytes < need) return fail(c, PT_E_ARG, "destination too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->dn_out, need, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_read_denoised_rgba8_aces(pt_ctx* c, unsigned char* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    if (!c->dn_done) return fail(c, PT_E_STATE, "no denoised image (pt_denoise first)");
    const long long n = (long long)c->rows_local * c->cfg.width;
    if (bytes < (size_t)n * 4) return fail(c, PT_E_ARG, "destination too small");
    if (n == 0) return PT_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!c->dn_rgba8) HIPCHK(c, hipMalloc(&c->dn_rgba8, (size_t)n * sizeof(uchar4)));
    // a view of its own: the image's (rgba8, stage_ok) is pt_present_*'s
    launch_aces(c->stream, c->dn_out, c->dn_rgba8, n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->dn_rgba8, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_read_guides(pt_ctx* c, float* dst, size_t bytes) {
    if (!c || !dst) return PT_E_ARG;
    if (!c->guides_ok) return fail(c, PT_E_STATE, "no guides (pt_denoise first)");
    const size_t n = (size_t)c->rows_local * c->cfg.width;
    if (bytes < n * 8 * sizeof(float)) return fail(c, PT_E_ARG, "destination too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<float> g(n * 4);
    for (int h = 0; h < 2; h++) {
        if (n) HIPCHK(c, hipMemcpy(g.data(), c->dn_guide[h], n * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) std::memcpy(dst + 8 * i + 4 * h, g.data() + 4 * i, 4 * sizeof(float));
    }
    return PT_OK;
}

// Measurements only (tools/denoise_measure.py; not part of the public ABI): how the iterations read their taps
// (ptd::Variant), and events around the guide render, the prep and each iteration of the denoises that follow.
int pt__denoise_debug(pt_ctx* c, int variant, int timing) {
    if (!c || variant < 0 || variant > 1) return PT_E_ARG;
    c->dn_variant = variant;
    c->dn_timing = timing != 0;
    c->dn_ev_n = 0;
    return PT_OK;
}
// ms of the last timed denoise: out[0] guide render, [1] prep, [2 ..] the iterations; returns the count (waits).
int pt__denoise_times(pt_ctx* c, float* out, int max_out) {
    if (!c || !out) return PT_E_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int n = 0;
    for (int i = 0; i + 1 < c->dn_ev_n && n < max_out; i++, n++) HIPCHK(c, hipEventElapsedTime(&out[n], c->dn_ev[i], c->dn_ev[i + 1]));
    return n;
}
}  // extern "C"
