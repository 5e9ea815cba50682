// pt_render_phase.h -- a section of the pt_render.hip translation unit, not a general-purpose header:
// pt_render.hip includes it once, after pt_kparams.h and before the kernel sections.
// The pieces of the SHADE and LEAF phases that both render kernels run -- k_render_sm (pt_render_sm.h) on path state
// in registers, k_render_pool (pt_render_pool.h) on path state in LDS -- each once, with the launch-uniform facts they
// branch on and the few helpers they need.  Every piece takes values and references and captures no kernel locals;
// k_render_pool passes LaunchFacts<true, true>, so it runs what the COMMON && SWEEP line of k_render_sm runs.
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const v4f lds_v4f;
// launch-constant data read through a wave-uniform index (the leaf sweep's table): in the constant address space
// such reads are scalar loads, and the values arrive as scalar operands
typedef __attribute__((address_space(4))) const v4f const_v4f;

// Triangle quad k of slot s: plane k of the LDS copy, or the AoS record in global memory (pt_render_sm.h, node_at).
template <bool LDS>
__device__ __forceinline__ float4 tri_quad(const SceneView& S, int slot, int k) {
#ifdef PT_DIAG_TRIS_GLOBAL   // diagnostic build (LDS bank-conflict attribution): triangles from HBM
    return S.tris[4 * slot + k];
#else
    return LDS ? S.tris[slot + k * S.tp] : S.tris[4 * slot + k];
#endif
}

// in_guard / in_range_abs: pt_math.h (one unsigned window on the bit patterns)
using pt::in_guard;
using pt::in_range_abs;

using pt::win_open;    // the hit windows 1e-4 < x < t and 1e-4 <= x < t (pt_math.h)
using pt::win_closed;

// Number of set bits of m below this lane.
__device__ __forceinline__ int rank_in(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// The launch-uniform facts the state machine branches on.  The generic kernels read them from
// their arguments, on every trip round the loop; a COMMON instantiation holds the default
// configuration's as constants (ptl::common_launch and enqueue_render vouch for each), so the
// untaken sides -- display modes 2-4, Moller-Trumbore, the non-culling walks, the raster tile
// order, the item division -- are not in its code.  Uniform control flow and address arithmetic
// only: every lane runs the same operations on the same values either way.  Measured on C2
// (DESIGN.md §5.2): mode, flags and the culling walk give about 1.8% each, the tile facts 0.3%,
// the single sphere nothing in time (7 fewer spilled SGPRs); the thresholds and the walk floor
// are not here because as constants they cost 1.1%.
// The leaf sweep (pt_cull.h, DESIGN.md §5.6, "The leaf sweep") is such a fact too: the COMMON line is built with it on and with it
// off (SWEEP), so tuning key 23 compares the two walks of one kernel; a generic line reads the kernel argument.
template <bool COMMON, bool SWEEP = false>
struct LaunchFacts {
    const KParams& p;
    __device__ __forceinline__ bool sweep() const { return COMMON ? SWEEP : p.sweep != 0; }
    __device__ __forceinline__ int mode() const { return COMMON ? 1 : p.mode; }
    __device__ __forceinline__ int flags() const { return COMMON ? 0 : p.flags; }
    __device__ __forceinline__ bool cons_walk() const { return COMMON || p.cons_walk != 0; }
    __device__ __forceinline__ bool scene_fast() const { return COMMON || p.scene_fast != 0; }
    __device__ __forceinline__ float win_lo() const { return COMMON ? ptc::kWindowLo : p.win_lo; }
    __device__ __forceinline__ int n_spheres() const { return COMMON ? 1 : p.sc.n_spheres; }
    __device__ __forceinline__ int tile_shift() const { return COMMON ? 0 : p.tile_shift; }
    __device__ __forceinline__ bool tile_perm() const { return COMMON || p.tile_perm != nullptr; }
    __device__ __forceinline__ bool tile_cost() const { return COMMON || p.tile_cost != nullptr; }
    // COMMON: the footprint is the image (x_limit >= W; a local row's y is below y_limit)
    __device__ __forceinline__ bool inside(int cx, int cy) const { return COMMON || ((cx < p.x_limit) & (cy < p.y_limit)); }
};

// A sweeping workgroup's triangle planes at `dst` (T slots per plane): the leaf sweep numbers the leaves by their
// chain position (a candidate bit is one), so this copy holds leaf pair q's two slots at 2 c, 2 c + 1, c = the chain
// position of pair q (the table's inverse map): every slot index the kernel keeps (s0, hprim) then is one of this copy.
__device__ __forceinline__ void stage_tris_chain_order(float4* dst, const KParams& p, int T, int nthreads) {
    for (int i = threadIdx.x; i < 4 * T; i += nthreads) {
        const int slot = i >> 2, c = __float_as_int(p.sweep_tab[2 * (slot >> 1) + 1].w);
        dst[(i & 3) * T + 2 * c + (slot & 1)] = p.sc.tris[i];
    }
}

// SHADE, a finished segment (Trace :434-501): the surface bounce of the hit (hprim >= 0: triangle slot, <= -2: sphere
// -2 - index, at o + d*t) or the sky.  Returns whether the path ended, with its colour in rgb; otherwise o, d, inc,
// col, state and bounce are the next segment's.
// TWIN: pti::shade_hit (pt_isect.h) is this dispatch on the display mode with the materials read through a scene
// accessor; here they are read in place and only the arithmetic is pt_isect.h's (DESIGN.md §17 has the compiler output).
template <bool LDS, class Facts>
__device__ __forceinline__ bool shade_segment(const Facts& F, const KParams& p, const SceneView& S, bool hit, int hprim,
                                              float t, f3& o, f3& d, f3& inc, f3& col, uint32_t& state, int& bounce,
                                              f3& rgb) {
    bool finished = false;
    rgb = inc;
    if (hit && pt::length_gt_001(col)) {
        const f3 hitp = o + d * t;
        f3 normal;
        int mat;
        if (hprim >= 0) {             // triangle: stored n, flipped (:421-428)
            const float4 nq = tri_quad<LDS>(S, hprim, 0);
            normal = mk(nq.x, nq.y, nq.z);
            mat = __float_as_int(tri_quad<LDS>(S, hprim, 2).w);
        } else {                      // sphere: normalize(hit - center) (:380)
            const int si = -2 - hprim;
            float4 s0 = S.spheres[2 * si];
            normal = pt::normalize(hitp - mk(s0.x, s0.y, s0.z));
            mat = __float_as_int(S.spheres[2 * si + 1].x);
        }
        if (pt::dot(normal, d) > 0.0f) normal = normal * -1.0f;
        if (F.mode() == 2) {
            rgb = (normal + mk(1, 1, 1)) * 0.5f;
            finished = true;
        } else if (F.mode() == 4) {
            float q = pti::depth_term(hitp, o);
            rgb = mk(q, q, q);
            finished = true;
        } else {
            o = hitp;
            f3 diffuse, specular;
            pti::bounce_dirs(normal, d, state, diffuse, specular);
            float4 m0 = S.mats[3 * mat], m1 = S.mats[3 * mat + 1], m2 = S.mats[3 * mat + 2];
            if (F.mode() == 3) {
                rgb = mk(m0.x, m0.y, m0.z);
                finished = true;
            } else {
                finished = pti::bounce_mix(m0, m1, m2, diffuse, specular, p.max_bounce, d, inc, col, state, bounce, rgb);
            }
        }
    } else {
        rgb = inc + pti::sky(d, (F.flags() & PT_FLAG_NO_SKY) != 0) * col;
        finished = true;
    }
    return finished;
}

// The wave-aggregated pull from the work queue: the lanes of m (the ballot of `want`) each get the next queue id.
// Frame-split items are short, so there a wave reserves ids in batches of pull_batch in qnext..qend (one queue
// atomic per batch instead of per pull; the counter is one address for the whole chip).  (A queue sharded over 8
// heads, one per XCD, measured slower on one-frame launches with and without overlap, and cost 5% on C2 in the same
// kernel.)
struct QueueIds { unsigned id, qnext, qend; };
template <bool SPLIT>
__device__ __forceinline__ QueueIds queue_ids(const KParams& p, bool want, unsigned long long m, unsigned qnext,
                                              unsigned qend) {
    const unsigned need = (unsigned)__popcll(m);
    const unsigned rank = (unsigned)rank_in(m);
    const int leader = __ffsll((long long)m) - 1;
    unsigned id;
    if (SPLIT && qend - qnext >= need) {
        id = qnext + rank;
        qnext += need;
    } else {
        const unsigned avail = SPLIT ? qend - qnext : 0u;
        const unsigned take = SPLIT ? max(need - avail, (unsigned)p.pull_batch) : need;
        unsigned base = 0;
        if (want && rank == 0u) base = atomicAdd(p.work_counter, take);   // the leader
        base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);
        id = rank < avail ? qnext + rank : base + (rank - avail);
        if (SPLIT) {
            qnext = base + (need - avail);
            qend = base + take;
        }
    }
    const QueueIds q = {id, qnext, qend};
    return q;
}

// The camera ray of pixel (lx, y), frame k (:514-542); r: the ray's index in its pixel (the first one seeds).
template <class Facts>
__device__ __forceinline__ void camera_ray(const Facts& F, const KParams& p, f3 cpos, f3 cfwd, f3 cright, f3 cup, int lx,
                                           int y, int k, int r, uint32_t& state, f3& o, f3& d, f3& inc, f3& col,
                                           int& bounce) {
    if (r == 0) state = pt::seed(lx, y, p.frame_first + k);
    float ax = 0.0f, ay = 0.0f;
    if (!(F.flags() & PT_FLAG_NO_AA)) {
        ax = pt::random01(state);
        ay = pt::random01(state);
    }
    float u = pti::film_coord((float)lx + ax, p.fW, p.rW);
    float v = pti::film_coord((float)y + ay, p.fH, p.rH);
    d = pt::normalize(pti::pinhole_dir(cfwd, cright, cup, u, v));
    o = cpos;
    inc = mk(0, 0, 0);
    col = mk(1, 1, 1);
    bounce = 0;
}

// The segment's verdict of the exact-reciprocal guard (pti::ray_in_guard) with the launch's scene half.
template <class Facts>
__device__ __forceinline__ bool seg_in_guard(const Facts& F, f3 o, f3 d) {
    return pti::ray_in_guard(F.scene_fast(), o, d);
}

// hit_sphere of sphere si (pti::sphere_t).
__device__ __forceinline__ float sphere_t(const SceneView& S, int si, f3 o, f3 d) {
    return pti::sphere_t(S.spheres[2 * si], o, d);
}

// The leaf sweep of a new segment inside the guard (`on`): its candidate leaves at this t, lowest bit first.
// DEPTH 0: the plain loop (ptc::sweep_mask), one box's bounds requested and awaited per iteration; DEPTH > 0: the
// pipelined loop (ptc::sweep_mask_piped) with DEPTH boxes' bounds in flight.  `table` is the sweep table through a
// wave-uniform index: the constant-address-space view (scalar loads) or the workgroup's LDS copy (broadcast reads).
template <int DEPTH = 0, class Table>
__device__ __forceinline__ unsigned sweep_candidates(const KParams& p, const SceneView& S, Table table,
                                                     bool on, f3 o, f3 rd, float t) {
    unsigned cand = 0u;
    if (on) {
        f3 ol, oh;
        ptc::cull_addends(o, rd, S.cm, S.ws, ol, oh);
        const ptc::SweepRay sr = ptc::sweep_ray(rd, ol, oh);
        // a camera outside the root box (wave-uniform): many of its rays miss the scene, and a wave
        // of them skips the sweep on the root's own test
        bool in = true;
        if (p.sweep_root) in = ptc::sweep_root_hit(p.root_box, sr, t, S.clo);
        if (in) cand = DEPTH > 0 ? ptc::sweep_mask_piped<(DEPTH > 0 ? DEPTH : 1)>(sr, t, S.clo, table, p.n_sweep)
                                 : ptc::sweep_mask(sr, t, S.clo, table, p.n_sweep);
    }
    return cand;
}

// The same candidates from the workgroup's signed table in LDS (ptc::sweep_mask_signed_piped; `pairs`: the table as
// 8-byte pairs): the ray's signs choose three read addresses once per segment instead of six selects, and a box costs
// 6 fmas.  The root box's test, wave-uniform and rare, keeps the split reciprocal.
template <int DEPTH>
__device__ __forceinline__ unsigned sweep_candidates_signed(const KParams& p, const SceneView& S, const float2* pairs,
                                                            bool on, f3 o, f3 rd, float t) {
    unsigned cand = 0u;
    if (on) {
        f3 ol, oh;
        ptc::cull_addends(o, rd, S.cm, S.ws, ol, oh);
        bool in = true;
        if (p.sweep_root) in = ptc::sweep_root_hit(p.root_box, ptc::sweep_ray(rd, ol, oh), t, S.clo);
        if (in) cand = ptc::sweep_mask_signed_piped<DEPTH>(rd, ol, oh, t, S.clo, pairs + ptc::sweep_signed_pair(rd.x, 0),
                                                           pairs + ptc::sweep_signed_pair(rd.y, 1),
                                                           pairs + ptc::sweep_signed_pair(rd.z, 2), p.n_sweep);
    }
    return cand;
}

using pti::LeafChoice;   // a leaf's 2-way choice (pt_isect.h)
using pti::leaf_choice;

}  // namespace
