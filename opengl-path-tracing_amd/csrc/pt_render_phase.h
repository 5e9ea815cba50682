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
            float s = pt::length(hitp - o);
            float dist = 1.0f - pt::fsqrt(s + 1.0f) / (s + 1.0f);
            float q = dist * dist;
            rgb = mk(q, q, q);
            finished = true;
        } else {
            o = hitp;
            f3 diffuse = pt::normalize(normal + pt::random_unit_vector(state));
            float kk = 2.0f * pt::dot(normal, d);
            f3 specular = pt::normalize(d - normal * kk);
            float4 m0 = S.mats[3 * mat], m1 = S.mats[3 * mat + 1], m2 = S.mats[3 * mat + 2];
            if (F.mode() == 3) {
                rgb = mk(m0.x, m0.y, m0.z);
                finished = true;
            } else {
                float is_spec = (m1.w > pt::random01(state)) ? 1.0f : 0.0f;
                d = pt::mix(diffuse, specular, m0.w * is_spec);
                inc = inc + mk(m1.x, m1.y, m1.z) * col;
                col = col * pt::mix(mk(m0.x, m0.y, m0.z), mk(m2.x, m2.y, m2.z), is_spec);
                bounce++;
                if (bounce > p.max_bounce) {
                    rgb = inc;
                    finished = true;
                }
            }
        }
    } else {
        f3 env = mk(0, 0, 0);
        if (!(F.flags() & PT_FLAG_NO_SKY)) {
            f3 dir = pt::normalize(d);
            float tt = 0.5f * (dir.z + 1.0f);
            float omt = 1.0f - tt;
            env = mk(omt * 1.0f + tt * 0.5f, omt * 1.0f + tt * 0.7f, omt * 1.0f + tt * 1.0f);
        }
        rgb = inc + env * col;
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
    // (x + jitter) / W by the exact reciprocal RN(1/W) and a Markstein
    // correction: the numerator is 0 or in [2^-32, 2^17), W <= 2^16, so the
    // remainder is exact and the quotient correctly rounded (test_exact_div)
    float u = pt::div_mk((float)lx + ax, p.fW, p.rW) - 0.5f;
    float v = pt::div_mk((float)y + ay, p.fH, p.rH) - 0.5f;
    d = pt::normalize((cfwd + cright * u) + cup * v);
    o = cpos;
    inc = mk(0, 0, 0);
    col = mk(1, 1, 1);
    bounce = 0;
}

// The ray half of the exact-reciprocal guard, with the scene half (F.scene_fast()), evaluated without short-circuit
// branches (each && of the old form was an exec-mask branch): every origin component 0 or in [2^-40, 2^60], every
// direction component in [2^-20, 2] (NaN fails).
template <class Facts>
__device__ __forceinline__ bool seg_in_guard(const Facts& F, f3 o, f3 d) {
    return F.scene_fast() & in_guard(o.x, 0x1p-40f, 0x1p60f) & in_guard(o.y, 0x1p-40f, 0x1p60f) &
           in_guard(o.z, 0x1p-40f, 0x1p60f) & in_range_abs(d.x, 0x1p-20f, 2.0f) &
           in_range_abs(d.y, 0x1p-20f, 2.0f) & in_range_abs(d.z, 0x1p-20f, 2.0f);
}

// hit_sphere (:209-226) of sphere si: the distance along o + d*t, or -1 (the caller keeps the closest in (1e-4, t)).
__device__ __forceinline__ float sphere_t(const SceneView& S, int si, f3 o, f3 d) {
    float4 s0 = S.spheres[2 * si];
    f3 oc = o - mk(s0.x, s0.y, s0.z);
    float a = pt::dot(d, d);
    float half_b = pt::dot(oc, d);
    float cq = pt::dot(oc, oc) - s0.w;
    float disc = half_b * half_b - a * cq;
    // the IEEE division sequence, not div_g: its range guard's four compares
    // cost more than the sequence (same quotient; +0.6% on C2, round 5)
    return disc < 0.0f ? -1.0f : (-half_b - pt::sqrt_g(disc)) / a;
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

// A leaf's 2-way choice (:406-429) between its triangles' hits h1, h2 (-1: a miss) against the segment's t.
struct LeafChoice { bool c1, c2; };
__device__ __forceinline__ LeafChoice leaf_choice(float h1, float h2, float t) {
    const bool c1 = win_open(h1, t) & ((h1 < h2) | (h2 < 0.0001f));
    const bool c2 = !c1 & win_open(h2, t);
    const LeafChoice r = {c1, c2};
    return r;
}

}  // namespace
