// pt_render_pool.h -- a section of the pt_render.hip translation unit, included after pt_render_sm.h.
// k_render_pool: the specialised swept line (LaunchPlan::common && sweep) with the path state in a wave-private LDS
// pool instead of registers (pt_pool.h).  A wave owns P paths and two ready lists; every pass it pops
// up to 64 paths of the longer list, one per lane, loads the fields the phase reads, runs the phase of k_render_sm on
// them -- the same per-ray functions on the same values -- stores what changed and pushes each path to the list of
// its new state.  The order in which paths are served cannot show in the image: every frame's colour goes to the
// frame-split scratch, and k_accum_frames applies the running mean in frame order.
// No cross-wave communication: the only barrier follows the scene staging; list heads and counts are wave-uniform.
// The arithmetic of the two phases is pt_render_phase.h's, the functions k_render_sm calls, with LaunchFacts<true, true>:
// the finished segment, the queue reservation, the camera ray, the guard, the sphere's distance, the sweep candidates,
// the leaf choice and the chain-order staging exist once.  What stays restated here, because it is bound to where the
// path state lives: the decode of a queue id to a pixel (TWIN: k_render_sm's decode, pt_render_sm.h; this one packs
// the pixel and the cost sample into the path record and has no tile shapes, raster order or clipped footprint), the
// sphere's acceptance (one sphere, no loop or counter) and the skeleton of the swept LEAF body.
// tests/test_gpu_path_pool.py compares the two kernels word for word.
// The leaf sweep of the set-up pass keeps bounds in flight ("Round 16"): at four waves per SIMD the
// plain loop's scalar load and full wait per box stood exposed 18 times per set-up pass on Cornell.  Two build
// switches, so that each form can be compared against the plain one in one process (tools/ab_inproc.py):
//   PT_POOL_SWEEP_DEPTH  boxes per chunk of the pipelined sweep (ptc::sweep_mask_piped: one chunk's bounds are
//                        requested while the other chunk is tested); 0: ptc::sweep_mask, as k_render_sm runs it
//   PT_POOL_SWEEP_LDS    1: the bounds come from the workgroup's LDS copy of the table (the one staged for the exact
//                        re-test) by broadcast reads, which return in order and are awaited by count; 0: from the
//                        scalar cache, whose loads return out of order and are awaited all together
// Same-process A/B on C2's 1024-frame launch against the plain loop, whose copy measured ±0.1-0.5% in those visits
// (profiles/ab/r16_pool_waits/):
//   LDS, depth 1 / 2 / 3 / 4:  +4.6% / +4.8..5.6% / +5.0% / +4.7%
//   scalar cache, depth 2:     -0.3%  (the second set of bounds costs 24 SGPRs in a kernel that is out of them: 46
//                                      lane writes and 61 lane reads of spilled SGPRs in the code, against 19 and 32)
// Depth 2 ships: 87 VGPRs (81 with the plain loop; 128 keep four waves per SIMD); depth 3 is within the floor of it.
#ifndef PT_POOL_SWEEP_DEPTH
#define PT_POOL_SWEEP_DEPTH 2
#endif
#ifndef PT_POOL_SWEEP_LDS
#define PT_POOL_SWEEP_LDS 1
#endif
// Round 17: the sweep reads each box's bounds near-first by the ray's signs from a signed table the
// workgroup builds in LDS (pt_cull.h, "the signed sweep table"): 6 fmas per box instead of 12 and three 8-byte reads
// instead of two broadcast 16-byte ones.  The signed table takes the place of the {lo, hi} copy, 3 quads per leaf
// instead of 2: the exact leaf re-test assembles its operands from the table's positive variants, the same floats
// (both tables side by side would cost a 24-leaf scene of 13 materials, one of the pinned fuzz soups, a workgroup per CU).
//   PT_POOL_SWEEP_SIGNED 1: ptc::sweep_mask_signed_piped at PT_POOL_SWEEP_DEPTH boxes per chunk (needs the LDS form and
//                        a depth above 0); 0: the round-16 loop on the {lo, hi} copy, for the same-process A/B
//                        (profiles/ab/r17_signed_sweep/); the planner's LDS account is the signed table's either way
// Same-process A/B against the parent (a copy of it: -0.05..+0.5%): +4.3% and +4.9% on C2's 1024-frame launch, +4.3% on the
// 1080p/8 share; depth 3 / 4 gain 3.6 / 2.7%, so depth 2 stays.  Per trip of four boxes the loop is 24 v_fma_f32, six
// ds_read2_b64 with immediate offsets, no v_cndmask and 4 address adds; 93 VGPRs.  Wave-VALU per segment 22.93 -> 21.69;
// the LDS array is busier than with the broadcast reads (60.6% -> 70.7% of the launch), not idler.
#ifndef PT_POOL_SWEEP_SIGNED
#define PT_POOL_SWEEP_SIGNED 1
#endif
#define PT_POOL_SIGNED_ON (PT_POOL_SWEEP_SIGNED && PT_POOL_SWEEP_LDS && PT_POOL_SWEEP_DEPTH > 0)
// Round 20: a bounce ray starts on the triangle it left, so its own pair's plane distance is near
// zero and, unless the pair is not coplanar, outside both hit windows for the whole segment.  Such a visit changes
// nothing but `bi &= bi - 1` and still costs the path a LEAF pass slot.  The thin wall boxes fall to the sweep's window
// clause; the fat boxes of the rotated blocks and non-coplanar pairs do not.  The set-up pass runs the LEAF pass's own
// plane tests on that one pair (pti::pair_in_window, pt_isect.h: the quads are staged already) and clears its bit
// where both distances are outside their windows at t0: the same (t, triangle) bit for bit, since the windows only
// shrink.  Camera rays and sphere hits have no own pair.  k_render_sm keeps its code: tests/test_gpu_path_pool.py and
// tests/test_gpu_plane_filter.py compare the two kernels word for word, which is the check of this filter.
// CPU model on Cornell's 1080p paths (tests/pool/plane_window_sim.cpp): 1.43 candidate visits per segment, 0.30 of
// them the own pair outside its windows, 20.9% of the LEAF path-visits.
//   PT_POOL_PLANE_FILTER 1: the filter; 0: every candidate bit is visited, for the same-process A/B
//                        (profiles/ab/r20_plane_window/)
// Same-process A/B against the parent (a copy of it: -0.58% and -0.03%): +2.76% on C2's 1024-frame launch, +2.64% on
// the 1080p/8 share; with both plane distances computed and selected by the coplanar flag +2.33%, so the second
// triangle's read and division sit under a wave-uniform branch.  36 VALU, two LDS reads and one division per set-up
// pass on Cornell; 94 VGPRs (93).  LDS instructions per segment 1.202 -> 1.122, wave-VALU 21.69 -> 21.27.
#ifndef PT_POOL_PLANE_FILTER
#define PT_POOL_PLANE_FILTER 1
#endif
namespace {

// The reference walk and leaf tests for a ray outside the exact-reciprocal guard (a few thousand of C2's segments),
// from global memory inside the set-up pass: the IEEE-division slab on the reference's node records and each lane's
// own triangle tests, as the generic global-memory line runs them.  The triangles are read from the LDS copy, whose
// slots are in chain order (pair q at chain position sweep_tab[2 q + 1].w), so hprim is an index of that copy.
__device__ __forceinline__ void pool_cold_walk(const KParams& p, const SceneView& S, f3 o, f3 d, float& t, int& hprim) {
    int w = 0;
    while (w >= 0) {
        const float4 lo = p.sc.nodes[2 * w], hi = p.sc.nodes[2 * w + 1];
        const int a = __float_as_int(hi.z), b = __float_as_int(hi.w);
        if (!slab(lo, hi, o, d, t)) { w = b; continue; }
        if (a >= 0) { w = a; continue; }
        const int q = (~a) >> 2;                                        // the leaf's pair
        const int s0 = 2 * __float_as_int(p.sweep_tab[2 * q + 1].w);    // its slots in the chain-order copy
        const bool cop = __float_as_int(tri_quad<true>(S, s0 + 1, 1).w) != 0;
        const float4 nda = tri_quad<true>(S, s0, 0);
        const float4 ndb = cop ? nda : tri_quad<true>(S, s0 + 1, 0);
        const float ta = tri_plane(nda, o, d);
        const float tb = cop ? ta : tri_plane(ndb, o, d);
        bool oka = false, okb = false, ca = false, cb = false;
        if (win_open(ta, t)) oka = tri_edges_at<true, false>(S, s0, mk(nda.x, nda.y, nda.z), o + d * ta, false, 0.0f, ca);
        if (win_closed(tb, t)) okb = tri_edges_at<true, false>(S, s0 + 1, mk(ndb.x, ndb.y, ndb.z), o + d * tb, false, 0.0f, cb);
        const float h1 = oka ? ta : -1.0f, h2 = okb ? tb : -1.0f;
        const LeafChoice lc = leaf_choice(h1, h2, t);
        if (lc.c1 | lc.c2) {
            t = lc.c1 ? h1 : h2;
            hprim = s0 + (lc.c1 ? 0 : 1);
        }
        w = b;
    }
}

// Orders a pass's LDS stores before the next pass's loads for the compiler (one wave: the hardware keeps LDS
// operations of a wave in order).
__device__ __forceinline__ void pool_pass_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NT, int P, int MINW>
__global__ __launch_bounds__(NT, MINW) void k_render_pool(KParams p) {
    static_assert(P >= 64 && P <= ptpool::kMaxPaths && P % 4 == 0, "one-byte list entries in a 16-byte padded array");
    using namespace ptpool;
    const LaunchFacts<true, true> F{p};   // the shared pieces (pt_render_phase.h) see the COMMON && SWEEP line's constants
    const const_v4f* const sweep_tab = (const const_v4f*)(size_t)p.sweep_tab;
    (void)sweep_tab;    // (the LDS form of the sweep reads the staged copy)
    resolve_frames(p);
    extern __shared__ float4 lds[];
    // staged: what swept rays read -- the triangle slots in chain order (planes), materials, the sphere, and the
    // leaf boxes in chain order: the signed table (ptc::kSignedQuads per leaf: the sweep's reads and, by its positive
    // variants, the exact re-test's), or without it the sweep table's own axis-paired records
    const int T = p.n_slots, nt = 4 * T, nm = 3 * p.n_mats, ns = 2, nb = ptc::kSignedQuads * p.n_sweep;
    stage_tris_chain_order(lds, p, T, NT);
    for (int i = threadIdx.x; i < nm; i += NT) lds[nt + i] = p.sc.mats[i];
    for (int i = threadIdx.x; i < ns; i += NT) lds[nt + nm + i] = p.sc.spheres[i];
#if PT_POOL_SIGNED_ON
    for (int leaf = threadIdx.x; leaf < p.n_sweep; leaf += NT) {    // (a thread per leaf: at most 32 of them, once)
        const float4 a = p.sweep_tab[2 * leaf], b = p.sweep_tab[2 * leaf + 1];
        for (int axis = 0; axis < ptc::kSignedQuads; axis++) {
            float q[4];
            ptc::sweep_signed_quad(a, b, axis, q);
            lds[nt + nm + ns + ptc::kSignedQuads * leaf + axis] = make_float4(q[0], q[1], q[2], q[3]);
        }
    }
#else
    for (int i = threadIdx.x; i < 2 * p.n_sweep; i += NT) lds[nt + nm + ns + i] = p.sweep_tab[i];
#endif
    const int scene_q = nt + nm + ns + nb;
    const int lane = (int)(threadIdx.x & 63u);
    float4* const pool = lds + scene_q + (int)(threadIdx.x >> 6) * (wave_bytes(P) / 16);
    unsigned char* const list = (unsigned char*)(pool + kChunks * P);
    for (int i = lane; i < P; i += kLanes) {    // every path starts fresh (t < 0) and without a work item
        pool[quad_of(kChunkO, i, P)] = make_float4(0, 0, 0, -1.0f);
        pool[quad_of(kChunkD, i, P)] = make_float4(0, 0, 1, 0);
        pool[quad_of(kChunkInc, i, P)] = make_float4(0, 0, 0, __uint_as_float(pack_hit(-1, -1)));
        pool[quad_of(kChunkCol, i, P)] = make_float4(1, 1, 1, 0);
        pool[quad_of(kChunkItem, i, P)] = make_float4(__uint_as_float(kNoItem), 0, 0, 0);
        list[i] = (unsigned char)i;
    }
    __syncthreads();
    SceneView S;
    S.nodes = nullptr;
    S.tris = lds;
    S.mats = lds + nt;
    S.spheres = lds + nt + nm;
    const float4* const boxes = lds + nt + nm + ns;
    const float2* const signed_pairs = (const float2*)boxes;
    (void)signed_pairs;
    S.np = 0;
    S.tp = T;
    S.cm[0] = p.cons_m[0], S.cm[1] = p.cons_m[1], S.cm[2] = p.cons_m[2];
    S.ws[0] = p.win_slack[0], S.ws[1] = p.win_slack[1], S.ws[2] = p.win_slack[2];
    S.clo = ptc::kWindowLo;
    const f3 cpos = mk(p.cam[0], p.cam[1], p.cam[2]), cfwd = mk(p.cam[3], p.cam[4], p.cam[5]);
    const f3 cright = mk(p.cam[6], p.cam[7], p.cam[8]), cup = mk(p.cam[9], p.cam[10], p.cam[11]);
    const int tiles_x = (p.W + 7) >> 3;
    const unsigned n_groups = (unsigned)((p.n_frames + p.group - 1) / p.group);
    const unsigned total_ids = p.queue_tiles * n_groups * 64u;
    unsigned qnext = 0, qend = 0;     // the wave's reserved queue ids
    Lists L = {P, 0};
    while (L.nS + L.nL > 0) {
        const int phase = choose(L), n = take(L, phase);
        const bool on = lane < n;
        int idx = 0;
        if (on) idx = list[pop_index(L, phase, n, lane, P)];
        drop(L, phase, n);
        bool to_shade = false, to_leaf = false;
        if (phase == kShade) {
            // ---------------- SHADE: finish segment, regenerate, set up the next segment (k_render_sm's, COMMON)
            const float4 c0 = pool[quad_of(kChunkO, idx, P)], c1 = pool[quad_of(kChunkD, idx, P)];
            const float4 c2 = pool[quad_of(kChunkInc, idx, P)], c3 = pool[quad_of(kChunkCol, idx, P)];
            const float4 c4 = pool[quad_of(kChunkItem, idx, P)];
            f3 o = mk(c0.x, c0.y, c0.z), d = mk(c1.x, c1.y, c1.z), inc = mk(c2.x, c2.y, c2.z), col = mk(c3.x, c3.y, c3.z);
            float t = c0.w;
            unsigned bi = __float_as_uint(c1.w);
            int hprim = hit_hprim(__float_as_uint(c2.w)), bounce = hit_bounce(__float_as_uint(c2.w));
            uint32_t state = __float_as_uint(c3.w);
            unsigned xy = __float_as_uint(c4.x);
            int aidx = __float_as_int(c4.y);
            int k = k_k(__float_as_uint(c4.z)), kend = k_kend(__float_as_uint(c4.z));
            unsigned pcost = cost_of(__float_as_uint(c4.w));
            bool report = cost_report(__float_as_uint(c4.w));
            bool retired = false;
#if PT_POOL_PLANE_FILTER
            int own = -1;              // the pair of the triangle a continuing path's ray leaves (round 20)
#endif
            if (on && !(t < 0.0f)) {   // a finished segment (t < 0: fresh)
                const bool hit = hprim != -1;
                pcost++;
                f3 rgb;
                const bool finished = shade_segment<true>(F, p, S, hit, hprim, t, o, d, inc, col, state, bounce, rgb);
#if PT_POOL_PLANE_FILTER
                if (!finished & (hprim >= 0)) own = hprim >> 1;
#endif
                if (finished) {
                    bounce = -1;
                    const f3 px = (mk(0, 0, 0) + rgb) / 1.0f;
                    nt_store3(p.rgb + 3 * ((size_t)k * (size_t)(p.rows_local * p.W) + (size_t)aidx), px);
                    k++;
                }
                t = -1.0f;
            }
            if (on & (bounce < 0) & (xy != kNoItem) & (k >= kend)) {
                if (report) atomicAdd(&p.tile_cost[(xy_crow(xy) >> 3) * tiles_x + (xy_lx(xy) >> 3)], pcost);
                xy = kNoItem;
            }
            // wave-aggregated pull from the work queue (k_render_sm's protocol)
            const bool want = on && xy == kNoItem;
            const unsigned long long m = __ballot(want);
            if (m) {
                const QueueIds qi = queue_ids<true>(p, want, m, qnext, qend);
                const unsigned id = qi.id;
                qnext = qi.qnext, qend = qi.qend;
                if (want) {
                    if (id >= total_ids) {
                        retired = true;      // the queue is empty: the path retires
                    } else {
                        const unsigned item = id >> 6, w = id & 63u;
                        const unsigned tile = p.grp_magic ? __umulhi(item, p.grp_magic) : item;
                        const int g = (int)(item - tile * n_groups);
                        const unsigned pk = p.tile_perm[tile];
                        const int tx = (int)(pk & 0xffffu), ty = (int)(pk >> 16);
                        const int cx = tx * 8 + (int)(w & 7u);
                        const int crow = ty * 8 + (int)(w >> 3);
                        if ((cx < p.W) & (crow < p.rows_local)) {
                            xy = pack_xy(cx, crow);
                            aidx = crow * p.W + cx;
                            report = (w & 0x1bu) == 0u;
                            pcost = 0;
                            k = g * p.group;
                            kend = min(k + p.group, p.n_frames);
                            bounce = -1;
                        }
                    }
                }
            }
            if (on && xy != kNoItem) {
                const int lx = xy_lx(xy), y = p.row0 + xy_crow(xy) * p.row_stride;
                if (bounce < 0) camera_ray(F, p, cpos, cfwd, cright, cup, lx, y, k, 0, state, o, d, inc, col, bounce);
                const bool fast_seg = seg_in_guard(F, o, d);
                const f3 rd = fast_seg ? mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z)) : mk(0, 0, 0);
                t = __builtin_huge_valf();
                hprim = -1;
                {
                    const float ht = sphere_t(S, 0, o, d);
                    if (win_open(ht, t)) {
                        t = ht;
                        hprim = -2;
                    }
                }
                const bool walk = !ray_has_nan(o, d);     // (a sweeping launch has nodes and triangles)
#if PT_POOL_SIGNED_ON
                unsigned cand = sweep_candidates_signed<PT_POOL_SWEEP_DEPTH>(p, S, signed_pairs, walk & fast_seg, o, rd, t);
#elif PT_POOL_SWEEP_DEPTH > 0 && PT_POOL_SWEEP_LDS
                unsigned cand = sweep_candidates<PT_POOL_SWEEP_DEPTH>(p, S, boxes, walk & fast_seg, o, rd, t);
#else
                unsigned cand = sweep_candidates<PT_POOL_SWEEP_DEPTH>(p, S, sweep_tab, walk & fast_seg, o, rd, t);
#endif
                // rays outside the guard: cold code, the whole reference walk here (wave-uniform branch)
                const bool cold = walk & !fast_seg;
                if (__any(cold)) {
                    if (cold) pool_cold_walk(p, S, o, d, t, hprim);
                }
#if PT_POOL_PLANE_FILTER
                // the own pair's plane tests at t0, as its LEAF visit would run them (a ray outside the guard has no bit)
                if ((own >= 0) & (((cand >> (own & 31)) & 1u) != 0u)) {
                    const int s0 = 2 * own;
                    const bool cop = __float_as_int(tri_quad<true>(S, s0 + 1, 1).w) != 0;
                    const float4 nda = tri_quad<true>(S, s0, 0);
                    // the second triangle's read and division only where some lane's pair is not coplanar
                    // (wave-uniform, as leaf_pair_tests has it: Cornell has no such pair)
                    bool keep;
                    if (__any(!cop)) {
                        const float4 ndb = cop ? nda : tri_quad<true>(S, s0 + 1, 0);
                        keep = pti::pair_in_window(nda, ndb, cop, o, d, t);
                    } else {
                        keep = pti::pair_in_window(nda, nda, true, o, d, t);
                    }
                    if (!keep) cand &= ~(1u << own);
                }
#endif
                bi = cand;
                to_leaf = cand != 0u;
            }
            to_shade = on & !retired & !to_leaf;
            if (on) {
                pool[quad_of(kChunkO, idx, P)] = make_float4(o.x, o.y, o.z, t);
                pool[quad_of(kChunkD, idx, P)] = make_float4(d.x, d.y, d.z, __uint_as_float(bi));
                pool[quad_of(kChunkInc, idx, P)] = make_float4(inc.x, inc.y, inc.z, __uint_as_float(pack_hit(hprim, bounce)));
                pool[quad_of(kChunkCol, idx, P)] = make_float4(col.x, col.y, col.z, __uint_as_float(state));
                pool[quad_of(kChunkItem, idx, P)] = make_float4(__uint_as_float(xy), __int_as_float(aidx),
                                                                __uint_as_float(pack_k(k, kend)),
                                                                __uint_as_float(pack_cost(pcost, report)));
            }
        } else {
            // ---------------- LEAF: the lowest candidate's pair tests, the 2-way choice, the exact re-test
            const float4 c0 = pool[quad_of(kChunkO, idx, P)], c1 = pool[quad_of(kChunkD, idx, P)];
            float* const hw = (float*)&pool[quad_of(kChunkInc, idx, P)] + 3;
            const unsigned hb = __float_as_uint(*hw);
            const f3 o = mk(c0.x, c0.y, c0.z), d = mk(c1.x, c1.y, c1.z);
            float t = c0.w;
            unsigned bi = __float_as_uint(c1.w);
            const bool at = on;
            int s0 = 0, lp = 0;
            bool cop = false;
            float4 nd0 = make_float4(0, 0, 0, 0);
            if (at) {
                lp = __ffs((int)bi) - 1;
                s0 = 2 * lp;
                cop = __float_as_int(tri_quad<true>(S, s0 + 1, 1).w) != 0;
                nd0 = tri_quad<true>(S, s0, 0);
            }
            float h1 = -1.0f, h2 = -1.0f;
            bool ca = false, cb = false;
            leaf_pair_tests<true, false>(S, at, s0, nd0, cop, o, d, t, p.compact_max, h1, h2, false, ca, cb);
            bool c1h = false, c2h = false;
            if (at) {
                const LeafChoice lc = leaf_choice(h1, h2, t);
                c1h = lc.c1, c2h = lc.c2;
            }
            // the sweep's test is conservative: the leaf's box passes the exact test at this t, or no triangle moves t
            const bool chk = at & (c1h | c2h);
            if (__any(chk)) {
                if (chk) {
                    const f3 rd = mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z));
#if PT_POOL_SIGNED_ON
                    // (lo, hi) per axis: the first pair of each of the leaf's three signed quads
                    const float2 bx = signed_pairs[ptc::kSignedPairs * lp], by = signed_pairs[ptc::kSignedPairs * lp + 2];
                    const float2 bz = signed_pairs[ptc::kSignedPairs * lp + 4];
                    if (!slab_fast(make_float4(bx.x, bx.y, by.x, by.y), make_float4(bz.x, bz.y, 0, 0), o, d, rd, t)) c1h = c2h = false;
#else
                    if (!slab_fast(boxes[2 * lp], boxes[2 * lp + 1], o, d, rd, t)) c1h = c2h = false;
#endif
                }
            }
            if (at) {
                int hprim = hit_hprim(hb);
                if (c1h | c2h) {
                    t = c1h ? h1 : h2;
                    hprim = s0 + (c1h ? 0 : 1);
                }
                bi &= bi - 1u;
                to_leaf = bi != 0u;
                to_shade = bi == 0u;
                ((float*)&pool[quad_of(kChunkO, idx, P)])[3] = t;
                ((float*)&pool[quad_of(kChunkD, idx, P)])[3] = __uint_as_float(bi);
                *hw = __uint_as_float(with_hprim(hb, hprim));
            }
        }
        // push: each path to the list of its new state
        const unsigned long long mS = __ballot(to_shade), mL = __ballot(to_leaf);
        if (to_shade) list[push_index(L, kShade, rank_in(mS), P)] = (unsigned char)idx;
        if (to_leaf) list[push_index(L, kLeaf, rank_in(mL), P)] = (unsigned char)idx;
        grow(L, kShade, __popcll(mS));
        grow(L, kLeaf, __popcll(mL));
        pool_pass_fence();
    }
}

}  // namespace
