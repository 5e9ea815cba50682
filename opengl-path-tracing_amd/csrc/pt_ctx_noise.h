// pt_ctx_noise.h -- a section of the pt_render.hip translation unit, not a general-purpose header: pt_render.hip
// includes it once, after its own host code.  What rests on the luminance moments: switching and
// reading them, the noise summary (pt_noise), pt_render_until, and adaptive sampling -- its per-tile buffers, the
// launch of one batch over a tile list (enqueue_adaptive) and pt_render_adaptive.
extern "C" {
// The noise estimate.  Turning the moments on or off changes which accumulate
// kernel every later launch runs and whether register-mode launches exist (split_mode), so
// the context's streams are drained and a captured graph, which bakes the pointer in, is dropped.
int pt_set_moments(pt_ctx* c, int enable) {
    if (!c) return PT_E_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t px = std::max<size_t>((size_t)c->rows_local * c->cfg.width, 1);
    c->mom_frames = 0;
    c->mom_mixed = false;
    if ((enable != 0) == (c->moments != nullptr)) {
        // already so; on again: zeroed behind the passes that may still write them
        if (c->moments) HIPCHK(c, hipMemsetAsync(c->moments, 0, px * sizeof(float2), c->stream));
        return PT_OK;
    }
    HIPCHK(c, drain_streams(c));
    drop_graph(c);
    if (!enable) {
        (void)hipFree(c->moments);
        c->moments = nullptr;
        return PT_OK;
    }
    if (!c->d_noise) HIPCHK(c, hipMalloc(&c->d_noise, sizeof(pt_noise_stats)));
    if (!c->h_noise) HIPCHK(c, hipHostMalloc((void**)&c->h_noise, sizeof(pt_noise_stats), hipHostMallocDefault));
    float2* m = nullptr;
    HIPCHK(c, hipMalloc(&m, px * sizeof(float2)));
    hipError_t e = hipMemset(m, 0, px * sizeof(float2));
    if (e != hipSuccess) {
        (void)hipFree(m);
        return fail(c, PT_E_HIP, std::string("hipMemset(moments): ") + hipGetErrorString(e));
    }
    c->moments = m;
    return PT_OK;
}

int pt_read_moments(pt_ctx* c, float* dst, size_t bytes, int* frames) {
    if (!c || !dst) return PT_E_ARG;
    if (!c->moments) return fail(c, PT_E_STATE, "moments are off (pt_set_moments)");
    const size_t need = (size_t)c->rows_local * c->cfg.width * sizeof(float2);
    if (bytes < need) return fail(c, PT_E_ARG, "destination too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, c->moments, need, hipMemcpyDeviceToHost));
    if (frames) *frames = c->mom_frames;
    return PT_OK;
}

// The summary on the context stream, behind the accumulate passes it depends on: the 32-byte
// block zeroed, k_noise, the block copied to pinned host memory; then one wait.
int pt_noise(pt_ctx* c, float target, pt_noise_stats* out) {
    if (!c || !out) return PT_E_ARG;
    if (!c->moments) return fail(c, PT_E_STATE, "moments are off (pt_set_moments)");
    if (c->mom_frames < 2) return fail(c, PT_E_STATE, "the noise estimate needs at least 2 frames");
    if (c->mom_mixed) return fail(c, PT_E_STATE, "per-tile frame counts after pt_render_adaptive: no single n until the image restarts");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemsetAsync(c->d_noise, 0, sizeof(pt_noise_stats), c->stream));
    const long long px = (long long)c->rows_local * c->cfg.width;
    if (px > 0) {
        KParams p;
        std::memset(&p, 0, sizeof(p));
        fill_image(p, c);
        p.moments = c->moments;
        const unsigned blocks = (unsigned)std::min<long long>((px + 255) / 256, (long long)kNoiseBlocksPerCu * c->n_cu);
        hipLaunchKernelGGL(k_noise, dim3(blocks), dim3(256), 0, c->stream, p, c->mom_frames, ptn::target_q(target),
                           c->d_noise);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(c->h_noise, c->d_noise, sizeof(pt_noise_stats), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = *c->h_noise;
    out->frames = c->mom_frames;
    return PT_OK;
}

int pt_render_until(pt_ctx* c, int frame_first, int acc_first, int batch, int max_frames, float target,
                    int* frames_done, pt_noise_stats* last) {
    if (!c || !frames_done) return PT_E_ARG;
    *frames_done = 0;
    if (batch < 2 || max_frames < batch || !(target > 0.0f))
        return fail(c, PT_E_ARG, "pt_render_until: batch >= 2, max_frames >= batch, target > 0");
    if (!c->scene_ok) return fail(c, PT_E_STATE, "pt_render_until before pt_upload_scene");
    if (acc_first && c->moments && c->mom_mixed)
        return fail(c, PT_E_STATE, "per-tile frame counts after pt_render_adaptive: pt_render_until must restart the image");
    if (!c->moments) {
        int rc = pt_set_moments(c, 1);
        if (rc) return rc;
    }
    const unsigned long long tq = ptn::target_q(target);
    pt_noise_stats s = {0, 0, 0, 0, 0};
    int done = 0;
    while (done < max_frames) {
        const int n = std::min(batch, max_frames - done);
        int rc = pt_render(c, frame_first + done, n, done ? 1 : acc_first);
        if (rc) return rc;
        done += n;
        *frames_done = done;
        rc = pt_noise(c, target, &s);
        if (rc) return rc;
        if (s.sum_q <= tq * s.pixels) break;      // mean relative error at or below the target
    }
    if (last) *last = s;
    return PT_OK;
}

// Adaptive sampling.  The buffers of the tile grid, on first use after set_tiles.
static int ensure_adaptive(pt_ctx* c) {
    const size_t bytes = (size_t)std::max(c->n_tiles, 1) * sizeof(unsigned);
    if (!c->d_adapt) HIPCHK(c, hipMalloc(&c->d_adapt, sizeof(AdaptSum)));
    if (!c->h_adapt) HIPCHK(c, hipHostMalloc((void**)&c->h_adapt, sizeof(AdaptSum), hipHostMallocDefault));
    if (!c->d_tile_frames) {
        HIPCHK(c, hipMalloc(&c->d_tile_frames, bytes));
        HIPCHK(c, hipMemsetAsync(c->d_tile_frames, 0, bytes, c->stream));
    }
    for (unsigned*& l : c->d_active)
        if (!l) HIPCHK(c, hipMalloc(&l, bytes));
    return PT_OK;
}

// One launch of an adaptive batch on the context stream: the render kernel over the `n_list` tiles of `list` (the
// generic line of the key the planner gives for that many tiles, no tile costs), then k_accum_retire over the same
// list.  n_after != 0: the batch's last launch, which decides.
static int enqueue_adaptive(pt_ctx* c, int frame_first, int n_frames, int acc_first, const unsigned* list, unsigned n_list,
                            unsigned* next, int n_after, unsigned frames_after, unsigned target_q) {
    ptl::Image im = plan_image(c);
    im.n_tiles = (int)n_list;
    ptl::State st = plan_state(c);
    st.adaptive = true;
    ptl::LaunchPlan pl;
    KParams p;
    int rc = plan_plain_split(c, im, st, frame_first, n_frames, acc_first, pl, p);
    if (rc) return rc;
    p.tile_perm = list;
    p.queue_tiles = n_list;
    p.tile_cost = nullptr;
    p.moments = c->moments;
    rc = launch_render(c, pl, p, c->stream, false, false, true);
    if (rc) return rc;
    const unsigned per_wave = adapt_tiles_per_wave(n_list), per_block = 4u * per_wave;
    AdaptArgs a = {n_list, per_wave, c->n_tiles, n_after, frames_after, target_q, c->d_tile_frames, next, c->d_adapt};
    hipLaunchKernelGGL(k_accum_retire, dim3((n_list + per_block - 1) / per_block), dim3(256), 0, c->stream, p, a);
    HIPCHK(c, hipGetLastError());
    return PT_OK;
}

int pt_render_adaptive(pt_ctx* c, int frame_first, int acc_first, int batch, int max_frames, float target,
                       int* frames_done, pt_adaptive_stats* last) {
    if (!c || !frames_done) return PT_E_ARG;
    *frames_done = 0;
    if (batch < 2 || max_frames < batch || !(target > 0.0f))
        return fail(c, PT_E_ARG, "pt_render_adaptive: batch >= 2, max_frames >= batch, target > 0");
    if (!c->scene_ok) return fail(c, PT_E_STATE, "pt_render_adaptive before pt_upload_scene");
    if (acc_first && c->moments && c->mom_mixed)
        return fail(c, PT_E_STATE, "per-tile frame counts after pt_render_adaptive: the next adaptive call must restart the image");
    if (!c->moments) {
        int rc = pt_set_moments(c, 1);
        if (rc) return rc;
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = ensure_tiles(c);
    if (rc) return rc;
    rc = ensure_adaptive(c);
    if (rc) return rc;
    const int n0 = acc_first ? c->mom_frames : 0;
    const unsigned tq = ptn::target_q(target);
    const size_t tile_bytes = (size_t)std::max(c->n_tiles, 1) * sizeof(unsigned);
    HIPCHK(c, reset_counters(c));
    c->stage_ok = false;
    c->aces_fuse = false;       // no ACES view from these passes: pt_present_begin runs its own
    c->presented = false;
    // the first list: every tile, in the learned order (behind the sorts on this stream; overlapped renders of
    // earlier calls have been waited for by the accumulate passes on it)
    HIPCHK(c, hipMemcpyAsync(c->d_active[0], c->d_tile_perm, tile_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_tile_frames, 0, tile_bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_adapt, 0, sizeof(AdaptSum), c->stream));
    std::memset(c->h_adapt, 0, sizeof(AdaptSum));
    unsigned n_list = c->rows_local > 0 ? (unsigned)c->n_tiles : 0u;
    int done = 0, cur = 0;
    while (done < max_frames && n_list > 0) {
        const int n = std::min(batch, max_frames - done);
        // the batch's share of the summary block: the tiles that stay active, and the next list's length
        HIPCHK(c, hipMemsetAsync(&c->d_adapt->act_pixels, 0, sizeof(AdaptSum) - offsetof(AdaptSum, act_pixels), c->stream));
        // a batch too large for the scratch budget or the 32-bit queue ids runs as several launches; the last decides
        const int step = launch_frames(c, n);
        for (int off = 0; off < n; off += step) {
            const int m = std::min(step, n - off);
            const bool decides = off + m >= n;
            rc = enqueue_adaptive(c, frame_first + done + off, m, (done + off) ? 1 : acc_first, c->d_active[cur], n_list,
                                  c->d_active[cur ^ 1], decides ? n0 + done + n : 0, (unsigned)(done + n), tq);
            if (rc) return rc;
        }
        HIPCHK(c, hipMemcpyAsync(c->h_adapt, c->d_adapt, sizeof(AdaptSum), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        done += n;
        c->mom_frames = n0 + done;      // the largest count; per tile from here on
        c->mom_mixed = true;
        c->adapt_done = done;
        if (c->h_adapt->n_next > n_list) return fail(c, PT_E_STATE, "internal: the active list grew");
        n_list = c->h_adapt->n_next;
        cur ^= 1;
    }
    // a context without rows: nothing rendered, the (empty) state restarts like the image
    if (done == 0 && !acc_first) c->mom_frames = 0, c->mom_mixed = false;
    c->count_pending = c->counting;
    *frames_done = done;
    if (last) {
        const AdaptSum& s = *c->h_adapt;
        last->noise.pixels = s.ret_pixels + s.act_pixels;
        last->noise.sum_q = s.ret_sum_q + s.act_sum_q;
        last->noise.above = s.ret_above + s.act_above;
        last->noise.max_q = std::max(s.ret_max_q, s.act_max_q);
        last->noise.frames = n0 + done;
        last->tiles = s.ret_tiles + s.n_next;
        last->tiles_active = s.n_next;
        last->pixel_frames = s.pixel_frames;
    }
    return pt_sync(c);
}

int pt_read_tile_frames(pt_ctx* c, unsigned* dst, int max_tiles, int* n_tiles, int* tiles_x) {
    if (!c) return PT_E_ARG;
    if (dst && max_tiles < c->n_tiles) return fail(c, PT_E_ARG, "tile frame buffer too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_tiles) *n_tiles = c->n_tiles;
    if (tiles_x) *tiles_x = c->tiles_x;
    if (dst && c->n_tiles > 0) {
        if (c->d_tile_frames)
            HIPCHK(c, hipMemcpy(dst, c->d_tile_frames, (size_t)c->n_tiles * sizeof(unsigned), hipMemcpyDeviceToHost));
        else
            std::memset(dst, 0, (size_t)c->n_tiles * sizeof(unsigned));
    }
    return PT_OK;
}
}  // extern "C"
