// pt_render_sm.h -- a section of the pt_render.hip translation unit, not a general-purpose header:
// pt_render.hip includes it once, after pt_render_phase.h.
// The render kernel k_render_sm and what only it uses: the LDS / global access of the scene
// (node_at, wrec_at), the lane utilities, the leaf phase's pair tests and the three walks.  The
// per-ray arithmetic it calls is pt_isect.h; the launch-uniform facts, tri_quad and the pieces of
// SHADE and LEAF it shares with k_render_pool are pt_render_phase.h.
namespace {

using pti::slab;
using pti::slab_fast;
using pti::slab_oct;
using pti::slab_oct_cons;
using pti::oct_base;
using pti::ray_has_nan;
using pti::tri_plane;
using pti::tri_mt;
using pti::accumulate;

// Records one wave iteration of a phase: the first active lane adds 1 and popcount(exec).
__device__ __forceinline__ void diag_tick(uint32_t& waves, uint32_t& lanes) {
    unsigned long long e = __builtin_amdgcn_read_exec();
    if ((int)(threadIdx.x & 63) == __ffsll((long long)e) - 1) {
        waves++;
        lanes += (uint32_t)__popcll(e);
    }
}

template <bool COUNT>
__device__ __forceinline__ void flush_counters(const KParams& p, const Cnt& c) {
    if (!COUNT) return;
    unsigned long long v[kNumCounters] = {c.seg, c.nodes, c.tri, c.sph, c.hits, c.tw, c.tl, c.lw, c.ll, c.sw, c.sl,
                                          c.slow, c.nan};
    for (int i = 0; i < kNumCounters; i++) {
        unsigned long long s = wave_sum(v[i]);
        if ((threadIdx.x & 63) == 0) atomicAdd(&p.counters[i], s);
    }
}

// =====================================================================================
// The render kernel: a persistent state-machine kernel with path regeneration.
//
// * Work items are (pixel, group of consecutive frames); lanes pull them from a device queue
//   with wave-aggregated atomics, 8x8-pixel tiles in queue order so a wave starts on a
//   coherent tile.  A lane whose path ended regenerates the next camera ray instead of
//   idling until the wave's longest path ends.  A pixel's frames stay in order, so the
//   running mean is bit-identical.
// * Slab test in exact-reciprocal form: q = RN((b-o)/d) computed as q0 = (b-o)*rd,
//   q = fma(fma(-q0, d, b-o), rd, q0) with rd = RN(1/d) per ray (Markstein's theorem:
//   correctly rounded when no under/overflow).  The guard that makes that hold is checked
//   per ray (|d_i| in [2^-20, 2], origin components 0 or in [2^-40, 2^60]) and per scene
//   (box coordinates likewise, at upload); lanes outside it use the IEEE division chain.
//   With all quotients finite the swap/compare chain of :309-365 equals min/max form.
// * Small scenes are staged in LDS once per workgroup (ds_read instead of vector-memory
//   gathers on the dependent node->node chain).
// =====================================================================================

// Node / triangle-record access of the state-machine kernel.  Global memory holds AoS
// records (node = 2 float4, triangle slot = 4 float4).  Its LDS copy is split into
// planes -- node half h of node i at [h*np + i], triangle quad k of slot s at [k*tp + s] --
// so random per-lane gathers of one half/quad hit 16-B bank groups spread over all 64
// banks instead of every 2nd (nodes, 32-B stride) or 4th (triangles, 64-B stride) group.
//
// WalkLinks: in the LDS image a node's (hi.z, hi.w) are the walk's next position after a
// box hit and after a miss, as byte offsets of the node (16 * index, its lo-plane entry) or
// -1 (chain ends):
//   internal node: (first child, next-right)
//   leaf node:     (-2 - code, next-right), code = k << 2 | coplanar << 1 | single: a hit
//                  stops the walk
// so one select is the whole link step.  The leaf's continuation (its next-right) rides in
// the spare .w of its first triangle's quad 1 (beside v0).
// The LDS walk holds 8 such images, one per octant of ray directions (image k at byte
// 32 * N * k, links absolute inside their image): image k stores the bounds of each axis
// whose direction sign bit is set in k swapped, near bound first (slab_oct); image 0 is the
// reference order.  A leaf's continuation is stored as its image-0 offset.
// The global-memory walk keeps the reference links (node indices, a = ~code at a leaf):
// there the loads, not the selects, set the pace, and the reference form measured faster.
extern __shared__ float4 g_lds[];   // the state-machine kernel's scene copy (nodes first)
// (scenes of at most kPadNodes nodes: images padded to that count, pt_launch_plan.h)
template <bool LDS, bool PADN = false>
__device__ __forceinline__ void node_at(const SceneView& S, int i, float4& lo, float4& hi) {
    if (LDS) {      // i = byte offset from the LDS base, which is 0 (checked at kernel entry)
        const v4f x = *(lds_v4f*)(size_t)(unsigned)i;
        const v4f y = PADN ? *(lds_v4f*)(size_t)((unsigned)i + 16u * kPadNodes)
                           : *(lds_v4f*)(size_t)(unsigned)(i + (S.np << 4));
        lo = make_float4(x.x, x.y, x.z, x.w);
        hi = make_float4(y.x, y.y, y.z, y.w);
    } else if (i < S.np) {   // global-memory scene: a top node, staged in LDS
        const v4f x = *(lds_v4f*)(size_t)(unsigned)(i << 4);
        const v4f y = *(lds_v4f*)(size_t)(unsigned)((i + S.np) << 4);
        lo = make_float4(x.x, x.y, x.z, x.w);
        hi = make_float4(y.x, y.y, y.z, y.w);
    } else {
        lo = S.nodes[2 * i];
        hi = S.nodes[2 * i + 1];
    }
}

// The three edge tests (:299-306) of triangle `slot` at p with normal n: the caller has n
// from the plane test (quad 0), so only the vertices (quads 1-3) are read.
// (tests/isect/isect_check.cpp restates the three expressions: moving them into pt_isect.h
// changes the scratch of five wide-walk instantiations and 13,676 lines of assembly)
// With `cert_on` (wave-uniform) it also evaluates the leaf re-test certificate of this
// triangle at p (ptw::leaf_certificate, pt_wide.h): its vertices are at hand here.
template <bool LDS, bool CERT>
__device__ __forceinline__ bool tri_edges_at(const SceneView& S, int slot, f3 n, f3 p, bool cert_on, float omax,
                                             bool& cert) {
    const float4 q1 = tri_quad<LDS>(S, slot, 1), q2 = tri_quad<LDS>(S, slot, 2), q3 = tri_quad<LDS>(S, slot, 3);
    const f3 v0 = mk(q1.x, q1.y, q1.z), v1 = mk(q2.x, q2.y, q2.z), v2 = mk(q3.x, q3.y, q3.z);
    const float e0 = pt::dot(n, pt::cross(v1 - v0, p - v0));
    const float e1 = pt::dot(n, pt::cross(v2 - v1, p - v1));
    const float e2 = pt::dot(n, pt::cross(v0 - v2, p - v2));
    if (CERT && cert_on) cert = ptw::leaf_certificate(p, n, v0, v1, v2, omax);
    return (e0 > 0.0f) & (e1 > 0.0f) & (e2 > 0.0f);
}
// The lane's index in its wave, recomputed where it is used (two VALU): a value held across
// the state-machine loop is spilled to scratch at 7 waves per SIMD, and its reload sat in
// the leaf and queue paths.  Volatile, so the compiler neither hoists nor merges it.
__device__ __forceinline__ int lane_id() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
__device__ __forceinline__ float fperm_f(int dst_bytes, float v) {
    return __int_as_float(__builtin_amdgcn_ds_permute(dst_bytes, __float_as_int(v)));
}

// The leaf phase of calculateRayCollision (:406-429) for the lanes at a leaf (`at`), with the
// edge tests compacted over the wave.  A leaf's 2-way choice
//   c1 = h1 > 1e-4 && h1 < t && (h1 < h2 || h2 < 1e-4),  c2 = !c1 && h2 > 1e-4 && h2 < t
// only depends on a triangle's edge verdict when its plane distance lies in (1e-4, t) for the
// first triangle and in [1e-4, t) for the second (outside those ranges both verdicts give the
// same c1 / c2: h1 <= 1e-4 fails c1 either way; h2 < 1e-4 or a miss (-1) both satisfy
// `h2 < 1e-4` and fail c2).  About 47% of the triangle tests of a Cornell frame need them
// (81% with the plain t >= 0 cull: a bounce ray starts ON the surface it left, at a plane
// distance near 0).  The wave's needed (lane, triangle) pairs are packed onto its first lanes
// -- forward permutes hand each worker lane its pair's hit point o + d*t and slot -- so one
// pass of edge tests serves both triangles of every lane; a ballot returns the verdicts.  More than 63 pairs: each lane tests its own.  Every edge
// test runs the same operations on the same values as at its source lane: the same bits.
// Returns (through h1 / h2) the hit_triangle results up to that equivalence.
// nda: quad 0 {n, d0} of slot s0; cop: the leaf code's coplanar bit.
// cert_on (wave-uniform): also return each triangle's leaf re-test certificate (ca / cb, for
// a triangle whose edge tests pass; omax = max_i |o_i|), computed by the lane that tests it.
template <bool LDS, bool CERT>
__device__ __forceinline__ void leaf_pair_tests(const SceneView& S, bool at, int s0, float4 nda, bool cop,
                                                f3 o, f3 d, float t, int max_pairs, float& h1, float& h2,
                                                bool cert_on, bool& cta, bool& ctb) {
    float ta = 0.0f, tb = 0.0f;
    if (at) ta = tri_plane(nda, o, d);
    // a coplanar pair (n and d0 equal up to the sign of zero components, flagged at upload)
    // has the same plane distance wherever it can pass the acceptance tests, so the second
    // one is only computed when some lane's leaf is not such a pair.  Its edge tests may use
    // the first triangle's n: a zero factor of either sign cannot change a `> 0` verdict.
    float4 ndb = nda;
    if (__any(at & !cop)) {
        if (at & !cop) {
            ndb = tri_quad<LDS>(S, s0 + 1, 0);
            tb = tri_plane(ndb, o, d);
        }
    }
    tb = cop ? ta : tb;
    const f3 na3 = mk(nda.x, nda.y, nda.z), nb3 = mk(ndb.x, ndb.y, ndb.z);
    const bool na = at & win_open(ta, t);
    const bool nb = at & win_closed(tb, t);
    const unsigned long long ma = __ballot(na), mb = __ballot(nb);
    const int ca = __popcll(ma), n = ca + __popcll(mb);
    bool oka = false, okb = false;
    const float omax = ptw::abs_max3(o);
    if (n <= max_pairs) {      // max_pairs <= 63 (tuning key 7; 0 = every lane tests its own)
        const int lane = lane_id();
        const int ja = rank_in(ma), jb = ca + rank_in(mb);
        // forward permutes hand worker j its pair's hit point o + d*t and slot; lanes
        // without a pair send to lane 63, never a worker (n <= 63)
        const int da = (na ? ja : 63) << 2, db = (nb ? jb : 63) << 2;
        const f3 pa = o + d * ta, pb = o + d * tb;
        const bool first = lane < ca;
        // (all eight permutes run on the full wave: a permute only moves data between
        // active lanes, so none of them may sit under the `first` select)
        const float ax = fperm_f(da, pa.x), ay = fperm_f(da, pa.y), az = fperm_f(da, pa.z);
        const float bx = fperm_f(db, pb.x), by = fperm_f(db, pb.y), bz = fperm_f(db, pb.z);
        const int as = __builtin_amdgcn_ds_permute(da, s0), bs = __builtin_amdgcn_ds_permute(db, s0 + 1);
        const f3 wp = first ? mk(ax, ay, az) : mk(bx, by, bz);
        const int ws = first ? as : bs;
        // the worker's normal: re-read from LDS, or for a global-memory scene (where the
        // loads, not the permutes, set the pace) handed over with the hit point
        f3 wn;
        if (LDS) {
            const float4 q0 = tri_quad<LDS>(S, ws, 0);
            wn = mk(q0.x, q0.y, q0.z);
        } else {
            const float nax = fperm_f(da, na3.x), nay = fperm_f(da, na3.y), naz = fperm_f(da, na3.z);
            const float nbx = fperm_f(db, nb3.x), nby = fperm_f(db, nb3.y), nbz = fperm_f(db, nb3.z);
            wn = first ? mk(nax, nay, naz) : mk(nbx, nby, nbz);
        }
        bool pass = false, cert = false;
        float wom = 0.0f;
        if (CERT && cert_on) {
            const float oa = fperm_f(da, omax), ob = fperm_f(db, omax);
            wom = first ? oa : ob;
        }
        if (lane < n) pass = tri_edges_at<LDS, CERT>(S, ws, wn, wp, cert_on, wom, cert);
        const unsigned long long r = __ballot(pass);
        oka = na & (((r >> ja) & 1ull) != 0ull);
        okb = nb & (((r >> jb) & 1ull) != 0ull);
        if (CERT && cert_on) {
            const unsigned long long rc = __ballot(pass & cert);
            cta = oka & (((rc >> ja) & 1ull) != 0ull);
            ctb = okb & (((rc >> jb) & 1ull) != 0ull);
        }
    } else {
        if (na) oka = tri_edges_at<LDS, CERT>(S, s0, na3, o + d * ta, cert_on, omax, cta);
        if (nb) okb = tri_edges_at<LDS, CERT>(S, s0 + 1, nb3, o + d * tb, cert_on, omax, ctb);
        cta = cta & oka;
        ctb = ctb & okb;
    }
    h1 = oka ? ta : -1.0f;
    h2 = okb ? tb : -1.0f;
}

// =====================================================================================
// The state machine (variants 0 and 3).  Every lane carries one path through three
// states -- TRAV (walking the link chain), LEAF (stopped at a leaf whose box it hit), SHADE
// (segment finished: shade / regenerate / set up the next segment) -- and each wave
// iteration runs ONE phase for the lanes in that state, picked by ballot counts:
//   SHADE when >= shade_thresh lanes wait to shade (or nothing else is runnable),
//   LEAF  when >= leaf_thresh lanes wait at leaves (or no lane is walking),
//   TRAV  otherwise (an inner walk loop that yields when either threshold is reached).
// A lane's own operation sequence is exactly the reference's (node, leaf tests before the
// next node, same t), so results are bit-identical; only lane interleaving changes.
// With the leaf sweep (scenes of a few leaves, pt_cull.h) a ray inside the guard never enters
// TRAV: its segment set-up leaves the candidate leaves as a bit mask in bi, and the lane stays
// in LEAF until the mask is empty.
// The pieces of SHADE and LEAF that do not depend on where the path state lives are pt_render_phase.h's, shared with
// k_render_pool (pt_render_pool.h), which runs the COMMON && SWEEP line on path state held in LDS.
// TWIN: the decode of a queue id to a pixel below is restated there in the pool record's packing.
// =====================================================================================
enum : int { ST_DONE = 0, ST_TRAV = 1, ST_LEAF = 2, ST_SHADE = 3 };
#ifndef PT_WALK_UNROLL
#define PT_WALK_UNROLL 4
#endif
#ifndef PT_SINK_UNROLL
#define PT_SINK_UNROLL 6    // its node steps per yield check (measured: 4 -2.2%, 8 -1.4% against 6)
#endif
constexpr int kWalkUnroll = PT_WALK_UNROLL;   // node steps per yield check of the walk (measured: 1 -> 2 +3.6%, 4 +5.7%, 6/8 slower)

// The TRAV phase: each TRAV lane advances one node per iteration (bvh_intersect + the link
// choice of calculateRayCollision :389-431) until it stops at a leaf whose box it hit
// (-> LEAF) or its walk ends (-> SHADE).  The wave yields once leaf_thresh lanes wait at
// leaves or shade_thresh lanes wait to shade; lanes only ever leave TRAV here, so the two
// separate counts are needed only once the waiting total reaches the smaller threshold.
// ALL_FAST: every walking lane is inside the exact-reciprocal guard (wave-uniform).
// No step counter: the reference's `steps < numNodes` bound (:393) can never bind on an
// accepted scene -- pt_upload_scene rejects link graphs with a cycle, and a walk in an
// acyclic graph visits each node at most once.  The transition is select-only; `leaf`
// keeps the raw link (~code), decoded in LEAF.
// CONS (LDS scenes, never counting): the culling walk -- lanes inside the guard test every
// node with slab_oct_cons; a leaf they stop at is re-tested exactly in the leaf phase.
template <bool ALL_FAST, bool COUNT, bool LDS, bool PADN, bool CONS = false>
__device__ __forceinline__ void trav_walk(const SceneView& S, f3 o, f3 d, f3 rd, bool fast, float t,
                                          unsigned long long live, unsigned long long m_trav,
                                          unsigned long long m_leaf, unsigned long long m_shade,
                                          int leaf_thresh, int shade_thresh,
                                          int trav_floor, int& st, int& bi, int& leaf, Cnt& c,
                                          bool eligible = true) {
    const int min_thresh = leaf_thresh < shade_thresh ? leaf_thresh : shade_thresh;
    f3 ol = mk(0, 0, 0), oh = mk(0, 0, 0);
    if (CONS) ptc::cull_addends(o, rd, S.cm, S.ws, ol, oh);   // S.cm[i] = 2^-19 M_i
    // Inside the walk one register carries the lane's state (WalkLinks): w >= 0 the next
    // node, w == -1 the chain ended (-> SHADE), w <= -2 stopped at the hit leaf with code
    // -2 - w (-> LEAF, bi = w).  st / bi are written back once at the end.
    // The culling walk's images end in sinks instead (pt_upload_scene): w < sink0 walks,
    // w == sink0 ended, w == sink0 + 16 (1 + k) stopped at leaf pair k; a stopped lane steps
    // in place, so the step runs unmasked.
    const int sink0 = (PADN ? kPadNodes : S.np) << 8;
    // LDS walks take the lane masks of the three states from the phase choice (uniform values:
    // no per-lane booleans copied into the walk loop, +1.2..1.5% on C2); the global-memory walk
    // measured 0.8-1% slower that way and keeps its own ballots
    // (eligible: the wide walk's scenes send only the lanes outside the exact-reciprocal guard
    // here, and the walking lanes inside it wait)
    const bool walking = (st == ST_TRAV) & eligible;
    const unsigned long long mw = LDS ? m_trav : __ballot(walking);
    const unsigned long long pre_leaf = LDS ? m_leaf : __ballot(st == ST_LEAF);
    const unsigned long long pre_shade = LDS ? m_shade : __ballot(st == ST_SHADE);
    int w = walking ? bi : (CONS ? sink0 : -1);
    // the yield test in counts: the walkers (ballot of w < sink0, or w >= 0) are live lanes, so
    // the lanes waiting elsewhere number popc(live) - walkers, and "waiting >= min_thresh" is
    // walkers <= popc(live) - min_thresh; floor1 >= 1 also covers "no walker left" (fewer
    // scalar instructions per yield check than the mask form)
    const int floor1 = trav_floor > 1 ? trav_floor : 1;
    const int wait_lim = __popcll(live) - min_thresh;
    if (CONS) {
        auto sstep = [&]() {
            float4 lo, hi;
            node_at<LDS, PADN>(S, w, lo, hi);
            const int a = __float_as_int(hi.z), b = __float_as_int(hi.w);
            const bool hb = (ALL_FAST || fast) ? slab_oct_cons(lo, hi, rd, ol, oh, t, S.clo) : slab(lo, hi, o, d, t);
#ifdef PT_PHASE_CLOCK
            if (w < sink0) diag_tick(c.tw, c.tl);
#endif
            w = hb ? a : b;
        };
        for (;;) {
#pragma unroll
            for (int u = 0; u < PT_SINK_UNROLL; u++) sstep();
            const int nw = __popcll(__ballot(w < sink0));
            if (nw < floor1) break;
            if (nw <= wait_lim) {
                if (__popcll(pre_leaf | __ballot(w > sink0)) >= leaf_thresh) break;
                if (__popcll(pre_shade | (__ballot(w == sink0) & mw)) >= shade_thresh) break;
            }
        }
        if (walking) {
            st = w < sink0 ? ST_TRAV : (w == sink0 ? ST_SHADE : ST_LEAF);
            bi = w;
            leaf = ((w - sink0) >> 4) - 1;   // the leaf pair
        }
        return;
    }
    auto step = [&]() {
        if (!LDS && !COUNT && ALL_FAST) {
            // global-memory walk without the per-step exec-mask branch: a lane whose walk has
            // stopped (w < 0) steps on the root, an LDS top node (S.np >= 1 for any tree), and
            // keeps its w and leaf
            const bool on = w >= 0;
            float4 lo, hi;
            node_at<LDS, PADN>(S, on ? w : 0, lo, hi);
            const int a = __float_as_int(hi.z), b = __float_as_int(hi.w);
            const bool hb = slab_fast(lo, hi, o, d, rd, t);
            leaf = on ? a : leaf;
            w = on ? (hb ? (a >= 0 ? a : -3 - b) : b) : w;
            return;
        }
        if (w >= 0) {
            float4 lo, hi;
            node_at<LDS, PADN>(S, w, lo, hi);
            int a = __float_as_int(hi.z), b = __float_as_int(hi.w);
            bool hb = (ALL_FAST || fast) ? (LDS ? (CONS ? slab_oct_cons(lo, hi, rd, ol, oh, t, S.clo)
                                                        : slab_oct(lo, hi, o, d, rd, t))
                                                 : slab_fast(lo, hi, o, d, rd, t))
                                         : slab(lo, hi, o, d, t);
            if (COUNT) { c.nodes++; diag_tick(c.tw, c.tl); }
#ifdef PT_PHASE_CLOCK
            if (!COUNT) diag_tick(c.tw, c.tl);
#endif
            if (LDS) {
                w = hb ? a : b;                       // WalkLinks: one select
            } else {                                  // reference links: a = ~code at a leaf
                leaf = a;
                w = hb ? (a >= 0 ? a : -3 - b) : b;
            }
        }
    };
    for (;;) {
#pragma unroll
        for (int u = 0; u < kWalkUnroll; u++) step();
        const int nw = __popcll(__ballot(w >= 0));
        if (nw < floor1) break;                   // too few walkers (or none): run a waiting phase
        if (nw <= wait_lim) {
            if (__popcll(pre_leaf | __ballot(w <= -2)) >= leaf_thresh) break;
            if (__popcll(pre_shade | (__ballot(w == -1) & mw)) >= shade_thresh) break;
        }
    }
    if (walking) {
        st = w >= 0 ? ST_TRAV : (w == -1 ? ST_SHADE : ST_LEAF);
        if (LDS) {
            bi = w;
            leaf = -2 - w;                // the leaf's code
        } else {
            bi = w >= -1 ? w : -3 - w;    // the leaf's continuation; leaf = ~code
        }
    }
}

// ------------------------------------------------------------------ the wide walk
// Global-memory scenes whose tree is nested (pt_bvh_culling_ok) walk the 4-wide quantised tree
// of pt_wide.h: one 48-B record per step tests up to four descendants
// conservatively, and the lane keeps a two-entry stack of pending children plus a resume
// position.  Lanes inside the exact-reciprocal guard only; their leaf boxes are re-tested
// exactly in the leaf phase before a triangle may move t.  The first `wtop` records sit in
// LDS as three planes (q0 at [i], q1 at [wtop + i], q2 at [2 wtop + i]).
// (measured, same-process A/B on the C3 / C4 stand-ins: stack depth 3 and three record visits
// per yield check with packed 48-B records +3.5% / +3.9% over depth 2, two visits, 64-B
// stride; each alone +0.5 / +2.6% (depth), +1.3 / -0.2% (unroll), +0.5 / +0.3% (stride))
constexpr int kWideStack = ptw::kStack;   // pt_wide.h (PT_WIDE_STACK)
// float4 per device record: the three quads of pt_wide.h packed (48 B) or on a 64-B stride
using ptp::kWideStride;                   // pt_scene_pack.h (PT_WIDE_STRIDE)
#ifndef PT_WIDE_UNROLL
#define PT_WIDE_UNROLL 3
#endif
__device__ __forceinline__ void wrec_at(const SceneView& S, int n, float4& q0, float4& q1, float4& q2) {
    if (n < S.wtop) {
        const unsigned b = (unsigned)n << 4, k = (unsigned)S.wtop << 4;
        const v4f x = *(lds_v4f*)(size_t)b;
        const v4f y = *(lds_v4f*)(size_t)(b + k);
        const v4f z = *(lds_v4f*)(size_t)(b + 2u * k);
        q0 = make_float4(x.x, x.y, x.z, x.w);
        q1 = make_float4(y.x, y.y, y.z, y.w);
        q2 = make_float4(z.x, z.y, z.z, z.w);
    } else {
        const float4* r = S.wrec + kWideStride * n;
        q0 = r[0];
        q1 = r[1];
        q2 = r[2];
    }
}

// The TRAV phase of the wide walk (every walking lane inside the guard): each lane visits one
// record per step (ptw::wide_hits + wide_visit, the functions the CPU model in
// tests/wide/wide_sim.cpp checks against the reference walk) until it stops at a leaf (-> LEAF)
// or its walk ends (-> SHADE).  Stopped lanes step on record 0 (in LDS) without changing their
// state.  The yield rule is trav_walk's.
__device__ __forceinline__ void trav_wide(const SceneView& S, f3 o, f3 rd, float t, unsigned long long live,
                                          int leaf_thresh, int shade_thresh, int trav_floor, int& st, int& bi,
                                          uint32_t (&e)[kWideStack], int& R) {
    const int min_thresh = leaf_thresh < shade_thresh ? leaf_thresh : shade_thresh;
    const ptw::WRay wr = ptw::make_wray(o, rd, S.cw, rd.x < 0.0f, rd.y < 0.0f, rd.z < 0.0f);
    const bool walking = st == ST_TRAV;
    const unsigned long long mw = __ballot(walking);
    const unsigned long long pre_leaf = __ballot(st == ST_LEAF), pre_shade = __ballot(st == ST_SHADE);
    int cur = walking ? bi : -1;
    const int floor1 = trav_floor > 1 ? trav_floor : 1;
    const int wait_lim = __popcll(live) - min_thresh;
    for (;;) {
#pragma unroll
        for (int u = 0; u < PT_WIDE_UNROLL; u++) {
            const bool on = cur >= 0;
            float4 q0, q1, q2;
            wrec_at(S, on ? cur >> 3 : 0, q0, q1, q2);
            const uint32_t pend = ptw::wide_hits(q0.x, q0.y, q0.z, __float_as_uint(q0.w), __float_as_uint(q1.x),
                                                 __float_as_uint(q1.y), __float_as_uint(q1.z), __float_as_uint(q1.w),
                                                 __float_as_uint(q2.x), __float_as_uint(q2.y), wr, t, cur & 7);
            if (on) cur = ptw::wide_visit<kWideStack>(cur, pend, __float_as_int(q2.z), __float_as_int(q2.w), e, R);
        }
        const int nw = __popcll(__ballot(cur >= 0));
        if (nw < floor1) break;
        if (nw <= wait_lim) {
            if (__popcll(pre_leaf | __ballot(cur <= -2)) >= leaf_thresh) break;
            if (__popcll(pre_shade | (__ballot(cur == -1) & mw)) >= shade_thresh) break;
        }
    }
    if (walking) {
        st = cur >= 0 ? ST_TRAV : (cur == -1 ? ST_SHADE : ST_LEAF);
        bi = cur;
    }
}

#ifdef PT_PHASE_CLOCK
// experiment builds only (tools/ab_build.sh with PT_EXTRA=-DPT_PHASE_CLOCK): per-phase
// wave-clock accounting of the state machine, read back by pt_debug_phase_clock
__device__ unsigned long long g_phase_clk[8];
#endif

#ifdef PT_WAVE_TRACE
// experiment builds only (-DPT_WAVE_TRACE): per wave of the last render launch, the wall clock
// (s_memrealtime, 100 MHz) at kernel entry, after the LDS staging and at exit, and the work
// items it took; read back by pt_debug_wave_trace
constexpr int kWaveTraceMax = 16384;
__device__ unsigned long long g_wave_trace[kWaveTraceMax * 4];
#endif

template <bool COUNT, bool LDS, int MINW, bool MULTI, bool SPLIT, bool PADN = false, int NT = 256, bool WIDE = false,
          bool COMMON = false, bool SWEEP = false>
__global__ __launch_bounds__(NT, MINW) void k_render_sm(KParams p) {
    static_assert(!WIDE || (!LDS && !COUNT), "the wide walk is the global-memory walk of a render build");
    static_assert(!COMMON || (!COUNT && LDS && !MULTI && SPLIT && PADN), "COMMON is the default path's LDS line");
    static_assert(!SWEEP || COMMON, "SWEEP is a constant of the COMMON line; generic lines read KParams::sweep");
    const LaunchFacts<COMMON, SWEEP> F{p};
    // the leaf sweep: 256-thread LDS render lines only (wave-uniform; with it on the walk culls, ptl::sweep_on)
#ifdef PT_DIAG_TRIS_GLOBAL
    const bool sweep = false;   // (the diagnostic build reads the triangles in the upload's order)
#else
    const bool sweep = LDS && !COUNT && !WIDE && NT == 256 && F.sweep();
#endif
    const const_v4f* const sweep_tab = (const const_v4f*)(size_t)p.sweep_tab;
#ifdef PT_WAVE_TRACE
    const unsigned long long wt_entry = __builtin_amdgcn_s_memrealtime();
    unsigned wt_items = 0;
#endif
    resolve_frames(p);
    extern __shared__ float4 lds[];
    SceneView S;
    if (LDS) {      // planes (see node_at / tri_quad)
        // node_at addresses LDS by raw offset: the dynamic LDS block must start at offset 0
        if ((unsigned)(size_t)(__attribute__((address_space(3))) const char*)g_lds != 0u) __builtin_trap();
        // 8 octant images (the culling walk: + its sink image)
        const int N = PADN ? kPadNodes : p.walk_np, T = p.n_slots, nt = 4 * T;
        const bool sk = !COUNT && F.cons_walk();
        const int nn = sk ? 18 * N : 16 * N;
        const float4* wsrc = sk ? p.sc.walk_sk : p.sc.walk_lds;
        const int nm = 3 * p.n_mats, ns = 2 * F.n_spheres();
        for (int i = threadIdx.x; i < nn; i += blockDim.x) lds[i] = wsrc[i];   // ready-made image
        if (sweep) {
            stage_tris_chain_order(lds + nn, p, T, blockDim.x);
        } else {
            for (int i = threadIdx.x; i < nt; i += blockDim.x) lds[nn + (i & 3) * T + (i >> 2)] = p.sc.tris[i];
        }
        for (int i = threadIdx.x; i < nm; i += blockDim.x) lds[nn + nt + i] = p.sc.mats[i];
        for (int i = threadIdx.x; i < ns; i += blockDim.x) lds[nn + nt + nm + i] = p.sc.spheres[i];
        __syncthreads();
        S.nodes = lds;
        S.tris = lds + nn;
        S.mats = lds + nn + nt;
        S.spheres = lds + nn + nt + nm;
        S.np = N;
        S.tp = T;
#ifdef PT_DIAG_TRIS_GLOBAL
        S.tris = p.sc.tris;
#endif
#ifdef PT_DIAG_SHADE_GLOBAL  // diagnostic build: materials and spheres from HBM
        S.mats = p.sc.mats;
        S.spheres = p.sc.spheres;
#endif
        S.cm[0] = p.cons_m[0];
        S.cm[1] = p.cons_m[1];
        S.cm[2] = p.cons_m[2];
        S.ws[0] = p.win_slack[0];
        S.ws[1] = p.win_slack[1];
        S.ws[2] = p.win_slack[2];
        S.clo = F.win_lo();
    } else {
        S.nodes = p.sc.nodes;     // reference layout; the walk image is for LDS only
        S.tris = p.sc.tris;
        S.mats = p.sc.mats;
        S.spheres = p.sc.spheres;
        S.wrec = p.sc.wrec;
        S.wlbox = p.sc.wlbox;
        S.cw[0] = p.wide_cw[0];
        S.cw[1] = p.wide_cw[1];
        S.cw[2] = p.wide_cw[2];
        if ((unsigned)(size_t)(__attribute__((address_space(3))) const char*)g_lds != 0u) __builtin_trap();
        // the top nodes (breadth-first numbering) in LDS planes: lo at [i], hi at [n_top + i];
        // the wide walk stages its top records instead (wrec_at), and the binary walk of its
        // lanes outside the guard reads every node from global memory
        const int K = WIDE ? p.wide_top : p.n_top;
        if (WIDE) {
            for (int i = threadIdx.x; i < 3 * K; i += blockDim.x) lds[(i % 3) * K + i / 3] = p.sc.wrec[kWideStride * (i / 3) + i % 3];
        } else {
            for (int i = threadIdx.x; i < 2 * K; i += blockDim.x) lds[(i & 1) * K + (i >> 1)] = p.sc.nodes[i];
        }
        const int KQ = WIDE ? 3 * K : 2 * K;   // float4 before the shading records
        // materials and spheres after them when small (p.shade_lds): every segment's sphere
        // test and every hit's material then read LDS, not scattered global lines (the global
        // walk is bound by its vector-memory lane-loads)
        if (p.shade_lds) {
            const int nm = 3 * p.n_mats, ns = 2 * p.sc.n_spheres;
            for (int i = threadIdx.x; i < nm; i += blockDim.x) lds[KQ + i] = p.sc.mats[i];
            for (int i = threadIdx.x; i < ns; i += blockDim.x) lds[KQ + nm + i] = p.sc.spheres[i];
            S.mats = lds + KQ;
            S.spheres = lds + KQ + nm;
        }
        __syncthreads();
        S.np = WIDE ? 0 : K;
        S.wtop = WIDE ? K : 0;
        S.tp = 0;
    }
#ifdef PT_PHASE_CLOCK
    const int lane = threadIdx.x & 63;
#endif
    const f3 cpos = mk(p.cam[0], p.cam[1], p.cam[2]), cfwd = mk(p.cam[3], p.cam[4], p.cam[5]);
    const f3 cright = mk(p.cam[6], p.cam[7], p.cam[8]), cup = mk(p.cam[9], p.cam[10], p.cam[11]);
    const int tsh = F.tile_shift(), tw = 8 << tsh, th = 8 >> tsh;   // tile: tw columns x th local rows
    const int tiles_x = (p.W + tw - 1) >> (3 + tsh);
    const unsigned n_groups = SPLIT ? (unsigned)((p.n_frames + p.group - 1) / p.group) : 1u;
    const unsigned total_ids = p.queue_tiles * n_groups * 64u;   // (the host's tile count: the grid, or an adaptive launch's list)
    // Three s_nop stand where the tile-count arithmetic was (12 bytes of scalar code): without them every loop below
    // sits 12 bytes earlier against the instruction fetch lines, and C2 measured 0.1-0.45% slower in four A/Bs on four
    // boxes; with them it is level with the kernel that computed the count.
    asm volatile("s_nop 0\n\ts_nop 0\n\ts_nop 0");
    const int n_nodes = p.sc.n_nodes;
    const bool use_tris = !(F.flags() & PT_FLAG_NO_TRIANGLES) && n_nodes > 0;
    // walk start for a ray inside the root box: its first child (the counting build walks
    // from the root, so the counts stay the reference's)
    const int root_skip = (COUNT || (!COMMON && p.root_child < 0)) ? -1 : p.root_child << (LDS ? 4 : 0);
    const bool has_skip = COMMON || root_skip >= 0;
#ifdef PT_WAVE_TRACE
    const unsigned long long wt_staged = __builtin_amdgcn_s_memrealtime();
#endif

    Cnt c = {0, 0, 0, 0, 0};
    int st = ST_SHADE;
    // "fresh" (SHADE without a segment to finish: start / after shading) is t < 0, and "a new
    // camera ray is due" is bounce < 0: no lane-mask booleans carried around the loop (their
    // merges cost scalar instructions on every iteration)
    int lx = -1, y = 0;
    int aidx = 0;             // rows_local * W < 2^31 (checked at pt_create)
    int k = 0, kend = 0, r = 0, bounce = -1;   // frames k..kend-1 of this work item
    unsigned qnext = 0, qend = 0;             // wave's reserved queue ids (frame-split mode)
    unsigned tile_id = 0, pcost = 0;    // adaptive queue order: this pixel's tile + segments
    float4 acc = make_float4(0, 0, 0, 0);
    f3 psum = mk(0, 0, 0), o = mk(0, 0, 0), d = mk(0, 0, 1), inc = mk(0, 0, 0), col = mk(1, 1, 1);
    uint32_t state = 0;
    // segment state.  Only the closest primitive and its t are carried; the hit point, the
    // normal and the material are rebuilt at shading time from them with the operations
    // the reference performs when it accepts the hit (o + d*t; the stored/recomputed
    // normal and its flip against d; matIdx), on the same final t -- the same bits.
    //   hprim >= 0: triangle slot, -1: no hit, <= -2: sphere (-2 - index)
    f3 rd = mk(0, 0, 0);
    float t = -1.0f;
    int hprim = -1, bi = -1, leaf = 0;   // bi: walk position (WalkLinks); leaf: code of a hit leaf
    // wide walk (lanes inside the guard): bi is its position (pt_wide.h), plus the stack and R
    uint32_t we[kWideStack] = {};
    int wR = -1;

#ifdef PT_PHASE_CLOCK
    unsigned long long clk[6] = {0, 0, 0, 0, 0, 0};   // cycles + wave iterations per phase
#endif
    for (;;) {
        // inside the exact-reciprocal guard (the segment's "fast" walk) <=> rd was set: |d_i| is
        // in [2^-20, 2] there, so RN(1/d_x) is nonzero; outside it rd stays 0
        const bool fast = rd.x != 0.0f;
        const unsigned long long mS = __ballot(st == ST_SHADE), mL = __ballot(st == ST_LEAF), mT = __ballot(st == ST_TRAV);
        int nS = __popcll(mS);
        int nL = __popcll(mL);
        int nT = __popcll(mT);
        if (nS + nL + nT == 0) break;
#ifdef PT_PHASE_CLOCK
        const unsigned long long clk_t0 = clock64();
        int clk_ph = 2;
        if (nS > 0 && (nS >= p.shade_thresh || (nT < p.trav_floor && nL == 0))) clk_ph = 0;
        else if (nL > 0 && (nL >= p.leaf_thresh || nT < p.trav_floor)) clk_ph = 1;
#endif
        // phase choice: SHADE / LEAF once their thresholds are reached, otherwise TRAV while
        // at least trav_floor lanes walk; below the floor the leaf phase runs if any lane
        // waits at a leaf, else shading (trav_floor 1 = walk until no lane walks)
        const bool low = nT < p.trav_floor;
        if (nS > 0 && (nS >= p.shade_thresh || (low && nL == 0))) {
            // ---------------- SHADE: finish segment, regenerate, set up next segment
            if (st == ST_SHADE && !(t < 0.0f)) {   // a finished segment (t < 0: fresh)
                const bool hit = hprim != -1;
                if (COUNT) { c.seg++; if (hit) c.hits++; diag_tick(c.sw, c.sl); }
                pcost++;
                f3 rgb;
                const bool finished = shade_segment<LDS>(F, p, S, hit, hprim, t, o, d, inc, col, state, bounce, rgb);
                if (finished) bounce = -1;
                if (finished) {
                    bool frame_done = true;
                    f3 px;
                    if (MULTI) {          // raysPerPixel > 1: pixel = 0 + sum of rays, / rpp
                        psum = psum + rgb;
                        r++;
                        frame_done = r >= p.rpp;
                        px = psum / (float)p.rpp;
                    } else {              // raysPerPixel == 1: pixel = (0 + rgb) / 1
                        px = (mk(0, 0, 0) + rgb) / 1.0f;
                    }
                    if (frame_done) {
                        if (SPLIT) {
                            // streamed once, read once by k_accum_frames: non-temporal, so the
                            // colour stream does not evict the scene from L2/MALL
                            nt_store3(p.rgb + 3 * ((size_t)k * (size_t)(p.rows_local * p.W) + (size_t)aidx), px);
                        } else {
                            int f = p.frame_first + k;
                            acc = accumulate(acc, px, f, k > 0 || p.acc_first == 1);
                        }
                        if (MULTI) {
                            psum = mk(0, 0, 0);
                            r = 0;
                        }
                        k++;
                    }
                }
                t = -1.0f;
            }
            if ((st == ST_SHADE) & (bounce < 0) & (lx >= 0) & (k >= (SPLIT ? kend : p.n_frames))) {
                if (!SPLIT) p.accum[aidx] = acc;
                if (F.tile_cost() && tile_id != ~0u) atomicAdd(&p.tile_cost[tile_id], pcost);
                lx = -1;
            }
            // wave-aggregated pull from the work queue (queue_ids, pt_render_phase.h)
            bool want = st == ST_SHADE && lx < 0;
            unsigned long long m = __ballot(want);
            if (m) {
                const QueueIds qi = queue_ids<SPLIT>(p, want, m, qnext, qend);
                const unsigned id = qi.id;
                qnext = qi.qnext, qend = qi.qend;
                if (want) {
                    if (id >= total_ids) {
                        st = ST_DONE;
                    } else {
                        const unsigned item = id >> 6, w = id & 63u;
                        // item -> (tile, frame group): by the host's exact magic reciprocal
                        // (kernel argument) when it is valid for every item
                        unsigned tile = item;
                        // (COMMON: the planner's magic is valid, or 0 for items of one group)
                        if (SPLIT) tile = p.grp_magic ? __umulhi(item, p.grp_magic) : (COMMON ? item : item / n_groups);
                        const int g = SPLIT ? (int)(item - tile * n_groups) : 0;
                        int tx, ty;
                        if (F.tile_perm()) {        // packed (ty << 16) | tx: no division
                            const unsigned pk = p.tile_perm[tile];
                            tx = (int)(pk & 0xffffu);
                            ty = (int)(pk >> 16);
                        } else {
                            tx = (int)(tile % (unsigned)tiles_x);
                            ty = (int)(tile / (unsigned)tiles_x);
                        }
                        tile = (unsigned)(ty * tiles_x + tx);
                        int cx = tx * tw + (int)(w & (unsigned)(tw - 1));
                        int crow = ty * th + (int)(w >> (3 + tsh));
                        int cy = p.row0 + crow * p.row_stride;
                        if ((cx < p.W) & (crow < p.rows_local) & F.inside(cx, cy)) {
                            lx = cx;
#ifdef PT_WAVE_TRACE
                            wt_items++;
#endif
                            y = cy;
                            aidx = crow * p.W + cx;
                            // cost sample: 4 pixels per 8x8 tile report (one 64-B memory-side
                            // atomic each), the rest keep tile_id = ~0u
                            tile_id = ((w & 0x1bu) == 0u) ? tile : ~0u;
                            pcost = 0;
                            k = g * p.group;
                            if (SPLIT) kend = min(k + p.group, p.n_frames);
                            r = 0;
                            psum = mk(0, 0, 0);
                            if (!SPLIT) acc = p.acc_first ? p.accum[aidx] : make_float4(0, 0, 0, 0);
                            bounce = -1;
                        }
                    }
                }
            }
            if (st == ST_SHADE && lx >= 0) {
                if (bounce < 0) camera_ray(F, p, cpos, cfwd, cright, cup, lx, y, k, r, state, o, d, inc, col, bounce);   // (:514-542)
                // segment set-up: exact-reciprocal guard, spheres (:372-385), walk start
                const bool fast_seg = seg_in_guard(F, o, d);
                // under the guard |d_i| is in [2^-20, 2]: rcp_fast is the exact RN(1/d_i); rd = 0
                // marks a segment outside it
                rd = fast_seg ? mk(pt::rcp_fast(d.x), pt::rcp_fast(d.y), pt::rcp_fast(d.z)) : mk(0, 0, 0);
                if (COUNT && !fast_seg) c.slow++;
                if (COUNT && ray_has_nan(o, d)) c.nan++;
                t = __builtin_huge_valf();
                hprim = -1;
                if (!(F.flags() & PT_FLAG_NO_SPHERES)) {
                    for (int si = 0; si < F.n_spheres(); si++) {
                        const float ht = sphere_t(S, si, o, d);
                        if (COUNT) c.sph++;
                        if (win_open(ht, t)) {
                            t = ht;
                            hprim = -2 - si;
                        }
                    }
                }
                const bool walk = use_tris & (COUNT || !ray_has_nan(o, d));
                // inside the root box (all three axes, inclusive) each axis has near <= 0 <=
                // far, so the exact slab says hit for any t >= 0: skip the root's test
                const bool inside = has_skip & fast_seg & (o.x >= p.root_box[0]) & (o.x <= p.root_box[1]) &
                                    (o.y >= p.root_box[2]) & (o.y <= p.root_box[3]) & (o.z >= p.root_box[4]) &
                                    (o.z <= p.root_box[5]);
                const int img = (LDS && fast_seg) ? oct_base(d, S.np << 5) : 0;   // octant image
                bi = walk ? ((WIDE && fast_seg) ? 0 : (inside ? root_skip : 0) + img) : -1;
                if (WIDE) {   // the wide walk starts at the root record with an empty stack
#pragma unroll
                    for (int k = 0; k < kWideStack; k++) we[k] = 0u;
                    wR = -1;
                }
                st = walk ? ST_TRAV : ST_SHADE;
                if (sweep) {
                    // the leaf sweep: a ray inside the guard tests every leaf box once at this t and never walks;
                    // bi carries its candidate leaves, lowest bit first (the root-inside test, the octant image and
                    // the walk start above are only for the rays outside the guard, which walk from the root)
                    const unsigned cand = sweep_candidates(p, S, sweep_tab, walk & fast_seg, o, rd, t);
                    bi = walk ? (fast_seg ? (int)cand : 0) : -1;
                    st = walk ? (fast_seg ? (cand ? ST_LEAF : ST_SHADE) : ST_TRAV) : ST_SHADE;
                }
            }
        } else if (nL > 0 && (nL >= p.leaf_thresh || low)) {
            // ---------------- LEAF: both triangle tests + the 2-way choice (:406-429)
            const bool at = st == ST_LEAF;
            // the leaf sweep: a lane inside the guard holds its candidate leaves in bi and visits the lowest
            const bool swept = sweep & fast;
            int s0 = 0, cont = -1;
            bool cop = false;
            float4 nd0 = make_float4(0, 0, 0, 0);
            if (at) {
                if (COUNT) { c.tri += 2; diag_tick(c.lw, c.ll); }
                const int code = LDS ? leaf : ~leaf;         // k << 2 | coplanar << 1 | single
                s0 = (code >> 1) & ~1;                       // slots 2k, 2k+1
                cop = (code & 2) != 0;
                if (WIDE && fast) {                          // wide walk: bi = -2 - (g << 1 | cop)
                    const int gc = -2 - bi;
                    s0 = gc & ~1;                            // slots 2g, 2g+1
                    cop = (gc & 1) != 0;
                }
                if (LDS && !COUNT && F.cons_walk()) {   // sinks carry the pair k only
                    int lp = leaf;
                    // a sweeping launch holds the slots in chain order: a candidate bit is a chain position (a swept
                    // lane at a leaf has a bit set); a ray outside the guard walked to pair `leaf`
                    // (entry 0 for a swept lane, whose `leaf` is stale: the read stays inside the table)
                    if (sweep) lp = swept ? __ffs(bi) - 1 : __float_as_int(p.sweep_tab[2 * (swept ? 0 : leaf) + 1].w);
                    s0 = 2 * lp;
                    cop = __float_as_int(tri_quad<LDS>(S, s0 + 1, 1).w) != 0;
                }
                nd0 = tri_quad<LDS>(S, s0, 0);               // {n, d0} of the first triangle
                if (!swept) {
                    cont = LDS ? __float_as_int(tri_quad<LDS>(S, s0, 1).w) : bi;   // LDS: next-right, image 0
                    if (LDS && (fast & (cont >= 0))) cont += oct_base(d, S.np << 5);
                }
            }
            float h1 = -1.0f, h2 = -1.0f;
            bool ca = false, cb = false;   // the chosen triangle certifies its leaf's box (pt_wide.h)
            if (F.flags() & PT_FLAG_MOLLER_TRUMBORE) {   // wave-uniform
                if (at) {
                    h1 = tri_mt(tri_quad<LDS>(S, s0, 1), tri_quad<LDS>(S, s0, 2), tri_quad<LDS>(S, s0, 3), o, d);
                    h2 = tri_mt(tri_quad<LDS>(S, s0 + 1, 1), tri_quad<LDS>(S, s0 + 1, 2),
                                tri_quad<LDS>(S, s0 + 1, 3), o, d);
                }
            } else {
                leaf_pair_tests<LDS, WIDE>(S, at, s0, nd0, cop, o, d, t, p.compact_max, h1, h2, WIDE && p.leaf_cert != 0, ca, cb);
            }
            bool c1 = false, c2 = false;
            if (at) {
                const LeafChoice lc = leaf_choice(h1, h2, t);
                c1 = lc.c1, c2 = lc.c2;
            }
            if (LDS && !COUNT && F.cons_walk()) {
                // the culling walk stopped here on the conservative test: the reference tests
                // this leaf's triangles only if its box passes the exact test at this t, and
                // only a triangle that moves t makes the difference (a leaf's hit and miss
                // links are the same next-right).  Its image-0 offset: slot 2k+1 quad 3 .w.
                const bool chk = at & fast & ((c1 & !ca) | (c2 & !cb));
                if (__any(chk)) {
                    if (chk) {
                        float4 lo, hi;
                        node_at<LDS, PADN>(S, __float_as_int(tri_quad<LDS>(S, s0 + 1, 3).w) + oct_base(d, S.np << 5),
                                           lo, hi);
                        if (!slab_oct(lo, hi, o, d, rd, t)) c1 = c2 = false;
                    }
                }
            }
            if (WIDE) {
                // the wide walk reached this leaf on the conservative test: as the culling walk,
                // its own box is tested exactly at this t before a triangle may move t (leaf g's
                // box at wlbox[2g], [2g + 1]) -- unless the chosen triangle certifies that test
                const bool chk = at & fast & ((c1 & !ca) | (c2 & !cb));
                if (__any(chk)) {
                    if (chk) {
                        if (!slab_fast(S.wlbox[s0], S.wlbox[s0 + 1], o, d, rd, t)) c1 = c2 = false;
                    }
                }
            }
            if (at) {
                if (c1 | c2) {
                    t = c1 ? h1 : h2;
                    hprim = s0 + (c1 ? 0 : 1);
                }
                if (WIDE && fast) {   // the next pending child, or the resume position
                    bi = ptw::wide_pop<kWideStack>(we, wR);
                    st = bi >= 0 ? ST_TRAV : (bi == -1 ? ST_SHADE : ST_LEAF);
                } else if (swept) {   // the next candidate, or the segment is finished
                    bi &= bi - 1;
                    st = bi ? ST_LEAF : ST_SHADE;
                } else {
                    bi = cont;
                    st = bi > -1 ? ST_TRAV : ST_SHADE;
                }
            }
        } else {
            // ---------------- TRAV: walk until a leaf is hit / the chain ends; yield to the
            // other phases once enough lanes wait there.  `fast` is fixed for the segment,
            // so a wave whose walking lanes are all inside the guard runs a walk without
            // the per-node IEEE-division branch.
            const unsigned long long live = LDS ? mS | mL | mT : __ballot(st != ST_DONE);
            const bool all_fast = LDS ? (__ballot(fast) & mT) == mT : __all(fast || st != ST_TRAV);
            if (LDS && !COUNT && F.cons_walk()) {    // the culling walk (kernel argument: uniform)
                // (with the leaf sweep only rays outside the guard walk, on the exact test)
                if (all_fast && !sweep)
                    trav_walk<true, COUNT, LDS, PADN, true>(S, o, d, rd, fast, t, live, mT, mL, mS, p.leaf_thresh, p.shade_thresh, p.trav_floor, st, bi, leaf, c);
                else
                    trav_walk<false, COUNT, LDS, PADN, true>(S, o, d, rd, fast, t, live, mT, mL, mS, p.leaf_thresh, p.shade_thresh, p.trav_floor, st, bi, leaf, c);
            } else if (WIDE) {
                // lanes outside the guard walk the binary tree first (rare), then the wide walk
                if (__ballot((st == ST_TRAV) & !fast))
                    trav_walk<false, COUNT, LDS, PADN>(S, o, d, rd, fast, t, live, mT, mL, mS, p.leaf_thresh, p.shade_thresh, p.trav_floor, st, bi, leaf, c, !fast);
                else
                    trav_wide(S, o, rd, t, live, p.leaf_thresh, p.shade_thresh, p.trav_floor, st, bi, we, wR);
            } else if (all_fast) {
                trav_walk<true, COUNT, LDS, PADN>(S, o, d, rd, fast, t, live, mT, mL, mS, p.leaf_thresh, p.shade_thresh, p.trav_floor, st, bi, leaf, c);
            } else {
                trav_walk<false, COUNT, LDS, PADN>(S, o, d, rd, fast, t, live, mT, mL, mS, p.leaf_thresh, p.shade_thresh, p.trav_floor, st, bi, leaf, c);
            }
        }
#ifdef PT_PHASE_CLOCK
        clk[clk_ph] += clock64() - clk_t0;
        clk[3 + clk_ph] += 1;
#endif
    }
#ifdef PT_PHASE_CLOCK
    if (lane == 0)
        for (int i = 0; i < 6; i++) atomicAdd(&g_phase_clk[i], clk[i]);
    {
        unsigned long long tw = wave_sum(c.tw), tl = wave_sum(c.tl);
        if (lane == 0) { atomicAdd(&g_phase_clk[6], tw); atomicAdd(&g_phase_clk[7], tl); }
    }
#endif
#ifdef PT_WAVE_TRACE
    {
        const unsigned long long wt_end = __builtin_amdgcn_s_memrealtime();
        unsigned items = wt_items;
        for (int off = 32; off > 0; off >>= 1) items += __shfl_xor(items, off, 64);
        const int wid = blockIdx.x * (NT / 64) + (int)(threadIdx.x >> 6);
        if ((threadIdx.x & 63) == 0 && wid < kWaveTraceMax) {
            g_wave_trace[4 * wid] = wt_entry;
            g_wave_trace[4 * wid + 1] = wt_staged;
            g_wave_trace[4 * wid + 2] = wt_end;
            g_wave_trace[4 * wid + 3] = items;
        }
    }
#endif
    flush_counters<COUNT>(p, c);
}

}  // namespace
