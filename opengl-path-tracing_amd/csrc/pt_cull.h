// pt_cull.h -- the node test of the LDS culling walk, shared by the HIP kernel
// (pt_render.hip), the scene packer (pt_scene_pack.h: the scene's window slack) and the CPU walk model
// (tests/cull/window_cull_sim.cpp); and, at the end of the file, the same test in the form the leaf sweep of
// tiny scenes runs it (sweep_mask; CPU model tests/cull/leaf_sweep_sim.cpp).
//
// The test is conservative on two sides.  Inside the exact-reciprocal guard every quotient is
// finite and normal or zero.  With u = 2^-24, q = RN(RN(b - o) / d) the reference's quotient and
// rd = RN(1/d), the margins are folded into per-ray addends:
//   near = fma(b, rd, ol),  far = fma(b, rd, oh),  ord = RN(-o * rd),
//   ol = ord - E_i,  oh = ord + E_i + W_i |rd_i|,
//   E_i = 2^-19 M_i |rd_i| + 2^-17 |ord_i|   (M_i: the scene's largest |coordinate| on axis i),
//   W_i = 20u max_j |o_j| + ws_i             (ws: the scene's window slack, window_slack below).
//
// (1) The t side, as before.  |b - o| <= M_i + |o_i| and |q| <= M_i |rd_i| + 1.01 |ord_i|; the
// error of every fma quotient against q, 4.2u |q| + 2.1u |ord| + 2.1u (oh - ord) including the
// roundings of the addends, is below E_i / 3 + 2.1u W_i |rd_i|, so near <= q_near and far >=
// q_far on every axis: a node the reference's test accepts (tn <= tf and tn <= t) is accepted
// here.
//
// (2) The window side.  The reference only ever accepts a triangle distance h with h > 0.0001f
// (computeShader.c:411, :420), so a leaf whose box ends before that distance cannot move t, nor
// can any box nested inside it: the walk also requires far >= c_lo on every axis, with
// c_lo = 1e-4 (1 - 2^-10), as max(tn, c_lo) <= min(tf, t) -- t > 1e-4 > c_lo always (t starts at
// +inf and only takes accepted distances), so c_lo may share the max with tn and one compare
// remains.  One more VALU per node (v_max_f32 with a constant operand), no register across the
// walk: the per-ray safety margin sits in oh.
//
// Lemma.  Let a ray inside the guard and a leaf triangle T = (v0, v1, v2) of a scene that passed
// pt_upload_scene with the clause on be such that the reference accepts T: hit_triangle
// (:274-307) returns h with h > 0.0001f and all three edge tests true.  Then far_i >= c_lo on
// every axis for T's leaf box and every ancestor's.
//
// Proof.  All data are binary32 values read as reals, |.| of a vector is its 2-norm.  n =
// normalize(cross(v1 - v0, v2 - v0)) and d0 = -dot(n, v0) are T's stored plane as pt_upload_scene
// rounds them, N = (v1 - v0) x (v2 - v0) exactly, D = n . N, L the longest edge, X_i - m_i the
// extent of T's vertices on axis i, rho = max_k |n . v_k + d0|, M2 = |(M_x, M_y, M_z)|,
// kappa = L^2 / D.  window_slack admits T only if D > 0, kappa <= 2^14 and rho <= L (in float64;
// its own rounding, 2^-50 relative, disappears in the factor 1.25 below).
//   (a) Edge tests.  The hit point is p_i = RN(o_i + RN(d_i h)).  Edge test k evaluates
//   e_k = dot(n, cross(E_k, w)), E_k = v_{k+1} - v_k, w = p - v_k: each of its six terms
//   n_a E_b w_c passes through at most seven roundings (E, w, E w, the cross's subtraction, the
//   product with n, two sums), and sum_a |n_a| (|E_b| |w_c| + |E_c| |w_b|) <= sqrt(2) |n| |E| |w|
//   (Cauchy-Schwarz twice), |n| <= 1 + 4u: e_k > 0 gives e^_k > -eps_k for the exact e^_k =
//   n . (E_k x (p - v_k)), eps_k = 10.1u |E_k| |p - v_k| + 2^-140 (the last term: underflows).
//   Write p = sum_j l_j v_j + s n with sum_j l_j = 1 (possible as D != 0).  e^_k is linear in p,
//   vanishes on edge k's line and along n, and equals D at the opposite vertex: e^_k =
//   D l_{k+2}.  So every l_j > -eta, eta = max_k eps_k / D; at most two of them are negative, so
//   q = sum_j l_j v_j exceeds the interval [m_i, X_i] by at most 2 eta (X_i - m_i).
//   |q - v_k| <= (1 + 5 eta) L and |p - v_k| <= |q - v_k| + sigma with sigma = |s n|, so
//   eta L <= 10.1u kappa ((1 + 5 eta) L + sigma) + 2^-140 L / D, and with 50.5u kappa < 0.05:
//   eta L <= a (L + sigma) + z,  a = 10.7u kappa <= 0.0105,  z = 1.06 * 2^-140 L / D.
//   (b) The plane.  n . p + d0 = sum_j l_j (n . v_j + d0) + s |n|^2, so sigma <= 1.001 (|g| +
//   rho (1 + 6 eta)) with g = (n . p + d0) / |n|.  h = RN(-nu / Delta) with nu = RN(RN(n . o) +
//   d0) = (n . o + d0) + e_nu, Delta = RN(n . d) = n . d + e_Delta, |e_nu| <= 4.01u (|n| |o| +
//   |d0|), |e_Delta| <= 3.01u |n| |d|.  Then n . o + d0 + h (n . d) = -e_nu - nu theta -
//   h e_Delta with |theta| <= u, |nu| <= 1.02 h |n| |d|, and the two roundings of p add at most
//   1.01u |n| (h |d| + |p|).  With h |d| <= 1.01 (|p| + |o|), |o| <= sqrt(3) omax (omax =
//   max_j |o_j|) and |p| <= M2 + sqrt(3) delta, where delta bounds p's excess over T's vertex
//   intervals:  |g| <= u (16 omax + 6.2 M2 + 4.06 |d0| + 10.8 delta).
//   (c) Together.  rho eta <= (rho / L) (a (L + sigma) + z) <= a rho + a sigma + z, delta <=
//   2 eta L + sigma and L <= 2 M2; solving the linear inequalities of (a) and (b) with a <=
//   0.0105 gives
//     sigma <= 17.1u omax + sigma_T,   sigma_T = u (7.2 M2 + 4.4 |d0|) + 1.14 rho + 6.5 z,
//     p_i in [m_i - delta_i, X_i + delta_i],
//     delta_i = 2 eta (X_i - m_i) + sigma <= 17.5u omax + [21.4u kappa (X_i - m_i) + 1.021 sigma_T + 2 z].
//   The bracket is delta_T,i; ws_i = 1.25 max_T delta_T,i.
//   (d) The far quotient.  For d_i > 0 the leaf box's far plane is b = max_i >= X_i (every leaf
//   box contains its triangles' vertices: checked at upload), so b - o_i >= p_i - o_i - delta_i >=
//   d_i h (1 - u) - 1.01u |p_i| - delta_i and Q = (b - o_i) / d_i >= h (1 - u) - (1.02u (M_i +
//   delta_i) + delta_i) |rd_i| (1 + u); d_i < 0 mirrors it with b = min_i.  far = RN(b rd + oh) >=
//   Q + (oh - ord) - (u |Q| + 1.01u |ord| + u |oh| + u |far|) >= Q + 0.9 E_i + 0.99 W_i |rd_i| (the
//   bracket is below E_i / 14 + 2.1u (oh - ord), as in (1)).  0.9 E_i >= 28u M_i |rd_i| covers
//   1.03u M_i |rd_i|, and 0.99 W_i >= 0.99 (20u omax + 1.25 delta_T,i) (1 - 2u) covers
//   1.001 delta_i: far >= h (1 - u) >= 0.0001f > c_lo, with a relative margin of 2^-10.
//   (e) Ancestors.  On a nested tree (pt_bvh_culling_ok) an ancestor's far plane lies at or beyond
//   the leaf's on every axis, so b' rd >= b rd as reals, and RN of the fma is monotone.  QED.
//
//   Overflow.  The rounding model above needs finite values.  h > 1e-4 and |d_i| >= 2^-20 keep
//   d_i h above the subnormals; if d_i h overflows, p_i and every w_i are infinite, and an edge
//   test can only be +inf if for each axis a with n_a != 0 the products n_a E^k_b sign(w_c) are
//   positive for all three edges k -- impossible, since the edge vectors sum to zero (and a zero
//   E^k_b makes the term NaN): no such hit is accepted.
// A triangle whose normal is not finite (zero area) never passes hit_triangle and asks nothing.
// A scene with a triangle outside (a)'s conditions runs without the clause (c_lo = -inf, ws = 0:
// the walk of (1) alone).
// Moller-Trumbore (PT_FLAG_MOLLER_TRUMBORE) accepts through another test with another window
// (t > 1e-7): that mode runs with c_lo = -inf, as does tuning key 22 = 1 (the A/B switch).
#pragma once

#include "pt_math.h"

namespace ptc {

// c_lo: just below the reference's acceptance threshold 0.0001f (1e-4 (1 - 2^-10), rounded)
constexpr float kWindowLo = 0.0001f * 0x1.ff8p-1f;
// the per-ray part of W: 20u max_j |o_j| (the lemma needs 1.02 * 17.5u)
constexpr float kWindowRay = 0x1.4p-20f;

PT_HD float min_t(float tf, float t) {
#if defined(__HIP_DEVICE_COMPILE__)
    // min(tf, t) for non-NaN operands as one v_med3: fminf would add a canonicalising v_max on
    // the loop-carried t (both are finite or +inf inside the guard)
    return __builtin_amdgcn_fmed3f(tf, t, -__builtin_huge_valf());
#else
    return fminf(tf, t);
#endif
}

// The per-ray addends ol = ord - E, oh = ord + E + W |rd| (cm[i] = 2^-19 M_i rounded up, ws the
// scene's window slack per axis).
PT_HD void cull_addends(pt::f3 o, pt::f3 rd, const float cm[3], const float ws[3], pt::f3& ol, pt::f3& oh) {
    const pt::f3 ord = pt::mk(-(o.x * rd.x), -(o.y * rd.y), -(o.z * rd.z));
    const float ax = __builtin_fabsf(rd.x), ay = __builtin_fabsf(rd.y), az = __builtin_fabsf(rd.z);
    const pt::f3 e = pt::mk(__builtin_fmaf(cm[0], ax, 0x1p-17f * __builtin_fabsf(ord.x)),
                            __builtin_fmaf(cm[1], ay, 0x1p-17f * __builtin_fabsf(ord.y)),
                            __builtin_fmaf(cm[2], az, 0x1p-17f * __builtin_fabsf(ord.z)));
    const float omax = fmaxf(fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    const float wx = __builtin_fmaf(kWindowRay, omax, ws[0]), wy = __builtin_fmaf(kWindowRay, omax, ws[1]),
                wz = __builtin_fmaf(kWindowRay, omax, ws[2]);
    ol = ord - e;
    oh = ord + pt::mk(__builtin_fmaf(wx, ax, e.x), __builtin_fmaf(wy, ay, e.y), __builtin_fmaf(wz, az, e.z));
}

// The node test on an octant image (bounds near-first for the ray's direction signs):
// (nx, fx, ny, fy) = the node's lo quad, (nz, fz) = its hi quad's .xy.  c_lo = kWindowLo, or -inf
// for the test without the window clause.
PT_HD bool cull_hit(float nx, float fx, float ny, float fy, float nz, float fz, pt::f3 rd, pt::f3 ol, pt::f3 oh,
                    float cur_t, float c_lo) {
    const float xn = __builtin_fmaf(nx, rd.x, ol.x), xf = __builtin_fmaf(fx, rd.x, oh.x);
    const float yn = __builtin_fmaf(ny, rd.y, ol.y), yf = __builtin_fmaf(fy, rd.y, oh.y);
    const float zn = __builtin_fmaf(nz, rd.z, ol.z), zf = __builtin_fmaf(fz, rd.z, oh.z);
    const float tn = fmaxf(fmaxf(xn, yn), zn);
    const float tf = fminf(fminf(xf, yf), zf);
    return fmaxf(tn, c_lo) <= min_t(tf, cur_t);   // one compare
}

// Host only.  The scene's window slack ws_i = 1.25 max_T delta_T,i over the triangles of its leaves
// (the lemma's (c)), rounded up; false (and ws = 0) when a triangle falls outside the lemma's
// conditions or the slack is not finite: the scene's walk then runs without the clause.  bvh: the reference's node records (12 floats: min, -, max, -, t0, t1, hit, miss),
// tris: 16 floats per triangle.
inline bool window_slack(const float* bvh, int n_nodes, const float* tris, float ws[3]) {
    const double u = 0x1p-24;
    const float inf = __builtin_huge_valf();
    ws[0] = ws[1] = ws[2] = 0.0f;
    if (n_nodes <= 0) return true;
    double M2 = 0.0;
    for (int q = 0; q < 3; q++) {
        const double m = fmax(fabs((double)bvh[q]), fabs((double)bvh[4 + q]));
        M2 += m * m;
    }
    M2 = sqrt(M2);
    double worst[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < n_nodes; i++) {
        const float* nd = bvh + 12 * (size_t)i;
        if (!(nd[8] > -1.0f)) continue;
        for (int k = 0; k < 2; k++) {
            const float* t = tris + 16 * (size_t)(int)nd[8 + k];
            const pt::f3 v0 = pt::mk(t[0], t[1], t[2]), v1 = pt::mk(t[4], t[5], t[6]), v2 = pt::mk(t[8], t[9], t[10]);
            const pt::f3 n = pt::normalize(pt::cross(v1 - v0, v2 - v0));   // as put_tri
            const float d0 = -pt::dot(n, v0);
            if (!(fabs((double)n.x) + fabs((double)n.y) + fabs((double)n.z) < (double)inf)) continue;   // never hit
            const double V[3][3] = {{v0.x, v0.y, v0.z}, {v1.x, v1.y, v1.z}, {v2.x, v2.y, v2.z}};
            const double nn[3] = {n.x, n.y, n.z};
            double E1[3], E2[3], L2 = 0.0, rho = 0.0;
            for (int q = 0; q < 3; q++) { E1[q] = V[1][q] - V[0][q]; E2[q] = V[2][q] - V[0][q]; }
            const double N[3] = {E1[1] * E2[2] - E2[1] * E1[2], E1[2] * E2[0] - E2[2] * E1[0], E1[0] * E2[1] - E2[0] * E1[1]};
            const double D = nn[0] * N[0] + nn[1] * N[1] + nn[2] * N[2];
            for (int a = 0; a < 3; a++) {
                const int b = (a + 1) % 3;
                double l2 = 0.0;
                for (int q = 0; q < 3; q++) l2 += (V[b][q] - V[a][q]) * (V[b][q] - V[a][q]);
                L2 = fmax(L2, l2);
                rho = fmax(rho, fabs(nn[0] * V[a][0] + nn[1] * V[a][1] + nn[2] * V[a][2] + (double)d0));
            }
            const double L = sqrt(L2);
            if (!(D > 0.0) || !(L2 <= 0x1p14 * D) || !(rho <= L)) return false;
            const double kappa = L2 / D, z = 1.06 * 0x1p-140 * L / D;
            const double sigma_t = u * (7.2 * M2 + 4.4 * fabs((double)d0)) + 1.14 * rho + 6.5 * z;
            for (int q = 0; q < 3; q++) {
                const double ext = fmax(fmax(V[0][q], V[1][q]), V[2][q]) - fmin(fmin(V[0][q], V[1][q]), V[2][q]);
                worst[q] = fmax(worst[q], 21.4 * u * kappa * ext + 1.021 * sigma_t + 2.0 * z);
            }
        }
    }
    for (int q = 0; q < 3; q++)
        if (!(worst[q] < 0x1p60)) return false;
    for (int q = 0; q < 3; q++) ws[q] = nextafterf((float)(1.25 * worst[q] * (1.0 + 0x1p-20)), inf);
    return true;
}

// ------------------------------------------------------------------ the leaf sweep ("The leaf sweep")
// A scene of a few leaves (ptl::kSweepMaxLeaves at most) does not walk: at segment set-up a ray inside the guard tests
// every leaf's own box once, at the segment's initial t0, and keeps the passing leaves as a bit mask in chain order
// (bit k = the k-th leaf the reference walk can reach); the leaf phase then visits the set bits from the lowest up
// and re-tests each leaf's box exactly at the current t before a triangle may move t, as it does for the culling
// walk.  The (t, triangle) of every segment are the reference's:
//   (a) the reference reaches a leaf only if the exact test of the leaf and of every ancestor passes at the t
//       current at that moment;
//   (b) t never grows and the exact test is monotone in t (tn <= min(tf, t)), so a leaf that passes at its visit
//       time passes at t0;
//   (c) the sweep's test is cull_hit's (below), which accepts whatever the exact test accepts at that t (1), and
//       with the window clause rejects only a leaf none of whose triangles can be accepted (the lemma): the mask
//       holds every leaf at which the reference moves t;
//   (d) in a nested tree a leaf's box lies inside every ancestor's, so its exact pass at t implies theirs at t and,
//       by (b), at the larger t of their own visits: the exact re-test of the leaf's box at the current t says
//       whether the reference visits the leaf, and t is the reference's by induction over the visits;
//   (e) the bits are taken in chain order, so equal distances resolve as in the reference.
// The rays of a wave differ in their octant, so the near-first images are of no use here.  Instead the ray's
// reciprocal is split by sign, rp_i = rd_i where rd_i > 0 else 0 and rn_i = rd_i - rp_i, and
//   near_i = fma(lo_i, rp_i, fma(hi_i, rn_i, ol_i)),   far_i = fma(hi_i, rp_i, fma(lo_i, rn_i, oh_i)).
// One of rp_i, rn_i is zero and the bounds are finite (the scene half of the guard), so the inner fma returns its
// addend exactly and the outer one is cull_hit's fma on the octant image, bit for bit -- up to the sign of a zero,
// which only enters comparisons.  The proof above therefore holds as it stands.  The bounds are the same for every
// lane: the kernel reads them through a wave-uniform index, as scalar operands.
struct SweepRay { pt::f3 rp, rn, ol, oh; };
PT_HD SweepRay sweep_ray(pt::f3 rd, pt::f3 ol, pt::f3 oh) {
    SweepRay r;
    r.rp = pt::mk(rd.x > 0.0f ? rd.x : 0.0f, rd.y > 0.0f ? rd.y : 0.0f, rd.z > 0.0f ? rd.z : 0.0f);
    r.rn = pt::mk(rd.x > 0.0f ? 0.0f : rd.x, rd.y > 0.0f ? 0.0f : rd.y, rd.z > 0.0f ? 0.0f : rd.z);
    r.ol = ol;
    r.oh = oh;
    return r;
}
// One box in the reference order (lo, hi per axis) at t0.
PT_HD bool sweep_hit(float lx, float hx, float ly, float hy, float lz, float hz, const SweepRay& r, float t0, float c_lo) {
    const float xn = __builtin_fmaf(lx, r.rp.x, __builtin_fmaf(hx, r.rn.x, r.ol.x));
    const float xf = __builtin_fmaf(hx, r.rp.x, __builtin_fmaf(lx, r.rn.x, r.oh.x));
    const float yn = __builtin_fmaf(ly, r.rp.y, __builtin_fmaf(hy, r.rn.y, r.ol.y));
    const float yf = __builtin_fmaf(hy, r.rp.y, __builtin_fmaf(ly, r.rn.y, r.oh.y));
    const float zn = __builtin_fmaf(lz, r.rp.z, __builtin_fmaf(hz, r.rn.z, r.ol.z));
    const float zf = __builtin_fmaf(hz, r.rp.z, __builtin_fmaf(lz, r.rn.z, r.oh.z));
    const float tn = fmaxf(fmaxf(xn, yn), zn);
    const float tf = fminf(fminf(xf, yf), zf);
    return fmaxf(tn, c_lo) <= min_t(tf, t0);
}
// mask + mask + hit: the box's verdict enters as the carry of one add
PT_HD unsigned sweep_push(unsigned m, bool hit) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(PT_SWEEP_NO_ADDC)
    // (the compiler makes a select and a shift-or of the C++ form, two instructions: +1.0% on C2 for this one)
    unsigned r;
    const unsigned long long c = __builtin_amdgcn_ballot_w64(hit);   // the compare's own lane mask
    unsigned long long co;
    asm("v_addc_co_u32 %0, %1, %2, %2, %3" : "=v"(r), "=s"(co) : "v"(m), "s"(c));
    return r;
#else
    return m + m + (hit ? 1u : 0u);
#endif
}
// The candidate mask of a ray inside the guard: bit k is set when the box of sweep-table entry k passes at t0.
// table: 2 quads per entry, {lo.x, hi.x, lo.y, hi.y}, {lo.z, hi.z, pair, inverse} (ptp::kSweep), indexable by int;
// n <= 32.  Entry k is the k-th leaf of the chain: its own box, axis-paired as the reference's node records (what
// pti::slab_fast reads: k_render_pool stages these records for its exact leaf re-test), and its triangle-pair index;
// `inverse` of entry p is the chain position of pair p (both render kernels stage the triangle slots by it).
// The boxes run from the last to the first so that a set bit enters as the carry of mask + mask.
// (This plain loop requests one box's bounds and waits for all of them before the box's 18 VALU.  In k_render_sm, at
// seven waves per SIMD, the other resident waves cover that latency: requesting box k - 1's bounds before box k's
// test measured 0.5% slower on C2 there.  At the path pool's four waves per SIMD they do not: k_render_pool runs
// sweep_mask_piped below on its LDS copy of the table, +5% on C2; DESIGN.md §5.12, "Round 16" -- and since round 17
// sweep_mask_signed_piped, further below, on the signed table: 6 of the 12 fmas, +4% more.)
template <class T>
PT_HD unsigned sweep_mask(const SweepRay& r, float t0, float c_lo, T table, int n) {
    unsigned m = 0u;
    for (int k = n - 1; k >= 0; k--) {
        const auto a = table[2 * k], b = table[2 * k + 1];
        m = sweep_push(m, sweep_hit(a.x, a.y, a.z, a.w, b.x, b.y, r, t0, c_lo));
    }
    return m;
}
// The same mask with the bounds of D boxes in flight: the n mod D highest boxes go first, plainly, then whole
// chunks of D boxes, the next chunk's bounds requested before the current chunk is tested (and none past the last:
// no read below the table).  Per box the same sweep_hit and sweep_push on the same values in the same order as
// sweep_mask, so the masks are equal; only when a load is issued differs.  Two register sets take the chunks in
// turn (a single rotating set cost the device 13 register copies per two boxes), and reads that return in order
// (LDS) are awaited by count.
#if defined(__clang__)
#define PT_SWEEP_UNROLL _Pragma("unroll")
#else
#define PT_SWEEP_UNROLL
#endif
// (The compiler's scheduler works block by block: a load whose first use is in the next trip round the loop looks free
// to it and goes to the end of the block, where it is awaited at once.  The fence keeps the request where it is written.)
PT_HD void sweep_issue_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
}
template <int D> struct SweepChunk { float q[D][6]; };      // boxes k, k - 1, .. k - D + 1, box k - j in q[j]
template <int D, class T>
PT_HD void sweep_chunk_load(SweepChunk<D>& c, T table, int k) {
    PT_SWEEP_UNROLL
    for (int j = 0; j < D; j++) {
        const auto a = table[2 * (k - j)], b = table[2 * (k - j) + 1];
        c.q[j][0] = a.x, c.q[j][1] = a.y, c.q[j][2] = a.z, c.q[j][3] = a.w, c.q[j][4] = b.x, c.q[j][5] = b.y;
    }
}
template <int D>
PT_HD unsigned sweep_chunk_test(unsigned m, const SweepChunk<D>& c, const SweepRay& r, float t0, float c_lo) {
    PT_SWEEP_UNROLL
    for (int j = 0; j < D; j++)
        m = sweep_push(m, sweep_hit(c.q[j][0], c.q[j][1], c.q[j][2], c.q[j][3], c.q[j][4], c.q[j][5], r, t0, c_lo));
    return m;
}
template <int D, class T>
PT_HD unsigned sweep_mask_piped(const SweepRay& r, float t0, float c_lo, T table, int n) {
    static_assert(D >= 1 && D <= 8, "boxes in flight");
    unsigned m = 0u;
    int k = n - 1;
    for (int j = n % D; j > 0; j--, k--) {
        const auto a = table[2 * k], b = table[2 * k + 1];
        m = sweep_push(m, sweep_hit(a.x, a.y, a.z, a.w, b.x, b.y, r, t0, c_lo));
    }
    if (k < 0) return m;
    SweepChunk<D> ca, cb;       // k + 1 is a multiple of D: whole chunks from here, the one at k in ca
    sweep_chunk_load(ca, table, k);
    for (; k >= 3 * D - 1; k -= 2 * D) {    // two more chunks below
        sweep_chunk_load(cb, table, k - D);
        sweep_issue_fence();
        m = sweep_chunk_test(m, ca, r, t0, c_lo);
        sweep_chunk_load(ca, table, k - 2 * D);
        sweep_issue_fence();
        m = sweep_chunk_test(m, cb, r, t0, c_lo);
    }
    if (k >= 2 * D - 1) {                   // one more
        sweep_chunk_load(cb, table, k - D);
        m = sweep_chunk_test(m, ca, r, t0, c_lo);
        return sweep_chunk_test(m, cb, r, t0, c_lo);
    }
    return sweep_chunk_test(m, ca, r, t0, c_lo);
}
template <class T>
PT_HD unsigned sweep_mask(pt::f3 rd, pt::f3 ol, pt::f3 oh, float t0, float c_lo, T table, int n) {
    return sweep_mask(sweep_ray(rd, ol, oh), t0, c_lo, table, n);
}
// ------------------------------------------------------------------ the signed sweep table ("Round 17")
// Where a read can carry a per-lane address (k_render_pool's LDS copy of the table), the choice between a box's two
// bounds is made by the address and costs nothing: per leaf the signed table holds 3 quads = six 8-byte pairs,
//   byte 16 a     : {lo_a, hi_a}   near first for rd_a > 0
//   byte 16 a + 8 : {hi_a, lo_a}   near first otherwise
// for the axes a = x, y, z, and a lane reads axis a of box k as one pair at pair index 6 k + 2 a + s_a with
// s_a = !(rd_a > 0), sweep_ray's predicate.  Two lanes of a read either share an address (a broadcast) or differ by
// 8 bytes within one quad, which are different banks: no conflict.  The pair is cull_hit's (near, far) of the ray's
// octant image, so the test is cull_hit itself, 6 fmas where sweep_hit runs 12:
//   near_a = fma(n_a, rd_a, ol_a),   far_a = fma(f_a, rd_a, oh_a).
// It equals sweep_hit on the same box.  For rd_a > 0 sweep_hit's inner fmas are fma(hi_a, 0, ol_a) and
// fma(lo_a, 0, oh_a): a finite bound times zero is a zero, so they return ol_a and oh_a -- exactly, except that an
// addend -0 may come back as +0 -- and the outer ones are fma(lo_a, rd_a, ol_a) and fma(hi_a, rd_a, oh_a), the two
// above with (n, f) = (lo, hi).  Otherwise rp_a = 0: the inner fmas are fma(hi_a, rd_a, ol_a) and fma(lo_a, rd_a, oh_a),
// the two above with (n, f) = (hi, lo), and the outer ones add a zero to them, which again changes at most the sign
// of a zero result.  A zero of either sign orders alike in fmaxf, fminf, min_t and <=, and no NaN arises on either
// side (finite bounds and reciprocals, finite addends), so the verdicts are equal: (c) of the sweep's argument above
// stands, now with cull_hit in person.
constexpr int kSignedQuads = 3;                     // per leaf
constexpr int kSignedPairs = 2 * kSignedQuads;      // 8-byte pairs per leaf
// Quad `axis` of a leaf's signed record from its two sweep-table quads a = {lo.x, hi.x, lo.y, hi.y}, b = {lo.z, hi.z, ..}.
template <class Q>
PT_HD void sweep_signed_quad(const Q& a, const Q& b, int axis, float q[4]) {
    const float lo = axis == 0 ? a.x : (axis == 1 ? a.z : b.x), hi = axis == 0 ? a.y : (axis == 1 ? a.w : b.y);
    q[0] = lo, q[1] = hi, q[2] = hi, q[3] = lo;
}
// The pair index of a ray's read on `axis` within a leaf's record (add kSignedPairs per leaf).
PT_HD int sweep_signed_pair(float rd_axis, int axis) { return 2 * axis + (rd_axis > 0.0f ? 0 : 1); }
// One box from its three pairs (near, far per axis) at t0.
PT_HD bool sweep_hit_signed(float xn, float xf, float yn, float yf, float zn, float zf, pt::f3 rd, pt::f3 ol, pt::f3 oh,
                            float t0, float c_lo) {
    return cull_hit(xn, xf, yn, yf, zn, zf, rd, ol, oh, t0, c_lo);
}
// The candidate mask from the signed table, with the chunk structure of sweep_mask_piped: the n mod D highest boxes
// first, then whole chunks of D boxes from two register sets, the next chunk's pairs requested before the current
// chunk is tested, none below the table.  px, py, pz: the lane's three views of the table, indexable in pairs
// (.x = near, .y = far), already offset by sweep_signed_pair, so box k's pairs are px[6 k], py[6 k], pz[6 k]: on the
// device three address registers per segment and immediate offsets in the loop.
template <int D, class P>
PT_HD void sweep_signed_load(SweepChunk<D>& c, P px, P py, P pz, int k) {
    PT_SWEEP_UNROLL
    for (int j = 0; j < D; j++) {
        const auto x = px[kSignedPairs * (k - j)], y = py[kSignedPairs * (k - j)], z = pz[kSignedPairs * (k - j)];
        c.q[j][0] = x.x, c.q[j][1] = x.y, c.q[j][2] = y.x, c.q[j][3] = y.y, c.q[j][4] = z.x, c.q[j][5] = z.y;
    }
}
template <int D>
PT_HD unsigned sweep_signed_test(unsigned m, const SweepChunk<D>& c, pt::f3 rd, pt::f3 ol, pt::f3 oh, float t0, float c_lo) {
    PT_SWEEP_UNROLL
    for (int j = 0; j < D; j++)
        m = sweep_push(m, sweep_hit_signed(c.q[j][0], c.q[j][1], c.q[j][2], c.q[j][3], c.q[j][4], c.q[j][5], rd, ol, oh, t0, c_lo));
    return m;
}
template <int D, class P>
PT_HD unsigned sweep_mask_signed_piped(pt::f3 rd, pt::f3 ol, pt::f3 oh, float t0, float c_lo, P px, P py, P pz, int n) {
    static_assert(D >= 1 && D <= 8, "boxes in flight");
    unsigned m = 0u;
    int k = n - 1;
    for (int j = n % D; j > 0; j--, k--) {
        SweepChunk<1> c;
        sweep_signed_load(c, px, py, pz, k);
        m = sweep_signed_test(m, c, rd, ol, oh, t0, c_lo);
    }
    if (k < 0) return m;
    SweepChunk<D> ca, cb;       // k + 1 is a multiple of D: whole chunks from here, the one at k in ca
    sweep_signed_load(ca, px, py, pz, k);
    for (; k >= 3 * D - 1; k -= 2 * D) {    // two more chunks below
        sweep_signed_load(cb, px, py, pz, k - D);
        sweep_issue_fence();
        m = sweep_signed_test(m, ca, rd, ol, oh, t0, c_lo);
        sweep_signed_load(ca, px, py, pz, k - 2 * D);
        sweep_issue_fence();
        m = sweep_signed_test(m, cb, rd, ol, oh, t0, c_lo);
    }
    if (k >= 2 * D - 1) {                   // one more
        sweep_signed_load(cb, px, py, pz, k - D);
        m = sweep_signed_test(m, ca, rd, ol, oh, t0, c_lo);
        return sweep_signed_test(m, cb, rd, ol, oh, t0, c_lo);
    }
    return sweep_signed_test(m, ca, rd, ol, oh, t0, c_lo);
}
// The sweep's first test where the camera stands outside the scene (KParams::sweep_root): the root box, by the same
// test.  Every leaf box lies inside it (a nested tree), the reference reaches a leaf only past the root's exact test
// at some t <= t0, which this test then passes too, and the lemma's (e) gives the root's far planes the window
// clause's bound wherever a leaf's triangle is accepted: a ray that fails here has no leaf to visit.  A wave none of
// whose rays passes skips the sweep, as the walk ends at its first node.
PT_HD bool sweep_root_hit(const float box[6], const SweepRay& r, float t0, float c_lo) {
    return sweep_hit(box[0], box[1], box[2], box[3], box[4], box[5], r, t0, c_lo);
}

}  // namespace ptc
