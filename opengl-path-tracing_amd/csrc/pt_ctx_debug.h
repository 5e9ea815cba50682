// pt_ctx_debug.h -- a section of the pt_render.hip translation unit, not a general-purpose header: pt_render.hip
// includes it last.  What tests and tools read back: the counters of the last counting render (pt_stats, pt_stats_ex),
// the pt_debug_* views of the launch bookkeeping, and the readers of the PT_WAVE_TRACE and PT_PHASE_CLOCK builds.
extern "C" {
#ifdef PT_WAVE_TRACE
extern "C" int pt_debug_wave_trace(unsigned long long* out, int max_waves, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    const int n = max_waves < kWaveTraceMax ? max_waves : kWaveTraceMax;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_trace), sizeof(unsigned long long) * 4 * n) != hipSuccess) return -1;
    if (reset) {
        std::vector<unsigned long long> z(4 * (size_t)kWaveTraceMax, 0ull);
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_wave_trace), z.data(), z.size() * 8) != hipSuccess) return -1;
    }
    return n;
}
#endif

#ifdef PT_PHASE_CLOCK
extern "C" int pt_debug_phase_clock(unsigned long long out[8], int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_clk), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_clk), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

int pt_stats_ex(pt_ctx* c, unsigned long long out[16]) {
    if (!c || !out) return PT_E_ARG;
    std::memcpy(out, c->last_counts, sizeof(c->last_counts));
    out[13] = c->sf.lds_bytes;
    out[14] = c->sf.walk_nested ? c->sf.lds_bytes_sk : 0;
    out[15] = ptl::cons_walk_on(c->sf, c->tun, c->counting);               // the scene's LDS walk culls (slab_oct_cons)
    return PT_OK;
}

int pt_debug_window_cull(pt_ctx* c, int* active, float* slack) {
    if (!c) return PT_E_ARG;
    if (active) *active = ptl::window_cull_on(c->sf, c->tun, c->cfg.flags, c->counting) ? 1 : 0;
    if (slack) *slack = std::max(c->sf.win_slack[0], std::max(c->sf.win_slack[1], c->sf.win_slack[2]));
    return PT_OK;
}

int pt_debug_sweep(pt_ctx* c, int* swept, int* qualifies, int* n_leaves) {
    if (!c) return PT_E_ARG;
    if (swept) *swept = c->last_swept ? 1 : 0;
    if (qualifies) *qualifies = c->sf.sweep_ok ? 1 : 0;
    if (n_leaves) *n_leaves = c->sf.n_leaves;
    return PT_OK;
}

int pt_debug_pool(pt_ctx* c, int* pooled) {
    if (!c) return PT_E_ARG;
    if (pooled) *pooled = c->last_pooled ? 1 : 0;
    return PT_OK;
}

int pt_debug_launches(pt_ctx* c, unsigned long long out[2]) {
    if (!c || !out) return PT_E_ARG;
    out[0] = c->n_line_launches[0];
    out[1] = c->n_line_launches[1];
    return PT_OK;
}

int pt_debug_tile_order(pt_ctx* c, unsigned long long* sorts, unsigned* perm_out, int max_tiles, int* n_tiles,
                        int* tiles_x) {
    if (!c) return PT_E_ARG;
    if (perm_out && max_tiles < c->n_tiles) return fail(c, PT_E_ARG, "tile order buffer too small");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // the sorts run on the context stream, which waits for every render before them
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sorts) *sorts = c->n_sorts;
    if (n_tiles) *n_tiles = c->n_tiles;
    if (tiles_x) *tiles_x = c->tiles_x;
    if (perm_out && c->n_tiles > 0)
        HIPCHK(c, hipMemcpy(perm_out, c->d_tile_perm, (size_t)c->n_tiles * sizeof(unsigned), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_stats(pt_ctx* c, double* ms, unsigned long long out[5]) {
    if (!c) return PT_E_ARG;
    if (ms) *ms = c->last_ms;
    if (out) std::memcpy(out, c->last_counts, 5 * sizeof(unsigned long long));
    return PT_OK;
}
}  // extern "C"
