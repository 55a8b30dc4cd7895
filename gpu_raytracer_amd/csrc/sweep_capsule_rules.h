// sweep_capsule_rules.h — the capsule sweep (rt_sweep_capsule, include/rt_hip.h "Capsule sweeps"), stated once.
//
// Two pieces of code answer it: the kernel (sweep_capsule.hip) and the host walk of tests/check_sweep_capsule.cpp, which holds the
// whole walk to a brute force over all primitives before any kernel runs.  Both call what is here: the time of first contact of a
// moving capsule with a triangle and with a sphere, the closest pair of the capsule's axis and a triangle (the start in contact and
// the reported point), the order among candidates, the lower bound of a node's eight child boxes widened by the capsule's bounding
// box, and the visitor that group_walk (group_walk.h) runs.  It builds on sweep_rules.h (sw_vertex, sw_edge, sw_take, sw_cross, the
// order, the octant) and through it on closest_point_rules.h (cp_triangle, cp_sphere, cp_order).  Every operation is one f32 rounding
// and nothing is fused in the answer (the build uses -ffp-contract=off; the only fused operations are written fmaf, and they are in
// the box bound), so numpy reproduces the bits (tests/sweep_capsule_cases.py).
//
// The capsule is every point within r of the segment A + d t .. A + axis + d t; B = A + axis per component.  With axis == 0 exactly,
// every expression below that involves the axis either has the value of its counterpart for A (x + 0 has the value of x; only the
// sign of a zero can differ, which no comparison here sees and which the final + 0.0f removes from a time) or never accepts, and a
// candidate of the closest pair replaces an earlier one only when strictly nearer: the answer then is rt_sweep_sphere's t, position,
// prim_id and material_id bit for bit, with s = 0, by construction.
#ifndef RT_SWEEP_CAPSULE_RULES_H
#define RT_SWEEP_CAPSULE_RULES_H

#include "sweep_rules.h"

namespace rt {

// The margin of the box bound: relative to the magnitudes that enter it in space, and relative to the entry time (sc_node_bounds).
#ifndef RT_SWC_SLACK
#define RT_SWC_SLACK 1.0e-5f
#endif

// One query: the sphere sweep's query of end A (c = A, d, r, rr, dd, tmax), the axis B - A, aa = dot(axis, axis), and for the node
// bound the centre of the capsule's bounding box, bc_a = A_a + axis_a * 0.5f, and its half extents h_a = |axis_a| * 0.5f + r.
struct ScQuery {
    SwQuery s;
    float ax[3], aa, bc[3], h[3], hmax;
};
RT_RULE ScQuery sc_query(const float origin[3], float radius, const float axis[3], const float direction[3], float tmax) {
    ScQuery q;
    q.s = sw_query(origin, radius, direction, tmax);
    for (int a = 0; a < 3; a++) q.ax[a] = axis[a], q.bc[a] = origin[a] + axis[a] * 0.5f, q.h[a] = fabsf(axis[a]) * 0.5f + radius;
    q.aa = cp_dot(axis, axis);
    q.hmax = rule_max(rule_max(q.h[0], q.h[1]), q.h[2]);
    return q;
}
// a query that is a miss without a walk: the sphere sweep's (a non-finite origin or direction component, a zero direction, a radius
// that is NaN, <= 0 or infinite, a tmax that is NaN or <= 0), or a non-finite axis component
RT_RULE bool sc_query_valid(const ScQuery& q) {
    return sw_query_valid(q.s) && std::isfinite(q.ax[0]) && std::isfinite(q.ax[1]) && std::isfinite(q.ax[2]);
}

// ---- 1. The closest pair of the axis segment P .. P + axis and a triangle, from its record's v0, e1, e2: the squared distance, the
// place s on the axis (0 at P, 1 at P + axis) and the weights (v, w) of v1 and v2.  The first of these candidates, in this order,
// with the STRICTLY smallest dist2 (a NaN dist2 is never below another, and nothing is below a first NaN):
//   a. end A:  cp_triangle(v0, e1, e2, P) -> dist2, v, w;  s = 0
//   b. end B:  cp_triangle at P_a + axis_a per component;  s = 1
//   c. the axis against the edges (v0, e1), (v0, e2), (v0 + e1, e3 = e2 - e1), in this order, as two clamped segments (Ericson,
//      Real-Time Collision Detection 5.1.9), each only if aa > 0 and ee = dot(e, e) > 0.  With m = P - v_k (ap, ap, ap - e1):
//        f = dot(e, m);  c = dot(axis, m);  b = dot(axis, e);  den = aa * ee - b * b
//        s = den > 0 ? clamp((b * f - c * ee) / den) : 0;   u = (b * s + f) / ee
//        u < 0:  u = 0, s = clamp(-c / aa);      u > 1:  u = 1, s = clamp((b - c) / aa)        clamp(x) = x < 0 ? 0 : x > 1 ? 1 : x
//        g_a = (m_a + axis_a * s) - e_a * u;  dist2 = dot(g, g);   (v, w) = (u, 0), (0, u), (1 - u, u)
//   d. the axis piercing the triangle, only if aa > 0:  n = cross(e1, e2), nn = dot(n, n), hA = dot(n, ap), hB = dot(n, ap + axis)
//      with hA < 0 && hB > 0 or hA > 0 && hB < 0;  s = hA / (hA - hB);  p_a = ap_a + axis_a * s;
//      v = dot(cross(p, e2), n) / nn, w = dot(cross(e1, p), n) / nn, accepted iff v >= 0 && w >= 0 && v + w <= 1:  dist2 = 0
RT_RULE float sc_clamp01(float x) { return x < 0.0f ? 0.0f : x > 1.0f ? 1.0f : x; }
RT_RULE void sc_pair_edge(const float m[3], const float e[3], const float ax[3], float aa, float& dist2, float& s, float& u) {
    const float ee = cp_dot(e, e), f = cp_dot(e, m), c = cp_dot(ax, m), b = cp_dot(ax, e), den = aa * ee - b * b;
    s = den > 0.0f ? sc_clamp01((b * f - c * ee) / den) : 0.0f;
    u = (b * s + f) / ee;
    if (u < 0.0f) u = 0.0f, s = sc_clamp01(-c / aa);
    else if (u > 1.0f) u = 1.0f, s = sc_clamp01((b - c) / aa);
    const float g[3] = {(m[0] + ax[0] * s) - e[0] * u, (m[1] + ax[1] * s) - e[1] * u, (m[2] + ax[2] * s) - e[2] * u};
    dist2 = aa > 0.0f && ee > 0.0f ? cp_dot(g, g) : INFINITY; // absent: never strictly below
}
RT_RULE float cap_triangle(const float v0[3], const float e1[3], const float e2[3], const float P[3], const float ax[3], float aa, float& s, float& v,
                           float& w) {
    float best = cp_triangle(v0, e1, e2, P, v, w); // a.
    s = 0.0f;
    { // b.
        const float B[3] = {P[0] + ax[0], P[1] + ax[1], P[2] + ax[2]};
        float bv, bw;
        const float d2 = cp_triangle(v0, e1, e2, B, bv, bw);
        if (d2 < best) best = d2, s = 1.0f, v = bv, w = bw;
    }
    const float ap[3] = {P[0] - v0[0], P[1] - v0[1], P[2] - v0[2]};
    const float m1[3] = {ap[0] - e1[0], ap[1] - e1[1], ap[2] - e1[2]}, e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    float d2, cs, cu;
    sc_pair_edge(ap, e1, ax, aa, d2, cs, cu); // c.
    if (d2 < best) best = d2, s = cs, v = cu, w = 0.0f;
    sc_pair_edge(ap, e2, ax, aa, d2, cs, cu);
    if (d2 < best) best = d2, s = cs, v = 0.0f, w = cu;
    sc_pair_edge(m1, e3, ax, aa, d2, cs, cu);
    if (d2 < best) best = d2, s = cs, v = 1.0f - cu, w = cu;
    { // d.
        float n[3], x[3], y[3];
        sw_cross(e1, e2, n);
        const float apb[3] = {ap[0] + ax[0], ap[1] + ax[1], ap[2] + ax[2]};
        const float nn = cp_dot(n, n), hA = cp_dot(n, ap), hB = cp_dot(n, apb);
        const float ps = hA / (hA - hB);
        const float p[3] = {ap[0] + ax[0] * ps, ap[1] + ax[1] * ps, ap[2] + ax[2] * ps};
        sw_cross(p, e2, x);
        sw_cross(e1, p, y);
        const float fv = cp_dot(x, n) / nn, fw = cp_dot(y, n) / nn;
        const bool across = (hA < 0.0f && hB > 0.0f) || (hA > 0.0f && hB < 0.0f);
        if (aa > 0.0f && across && fv >= 0.0f && fw >= 0.0f && fv + fw <= 1.0f && 0.0f < best) best = 0.0f, s = ps, v = fv, w = fw;
    }
    return best;
}

// ---- 2. A triangle: the time of the first contact of the moving capsule with it, +inf when there is none.  cap_triangle at the start
// <= rr answers 0: an axis that pierces the triangle is inside the prism below and far from all its pieces.  Otherwise the point A
// enters the prism "triangle + (-axis)" widened by the ball, whose boundary pieces are, with ap_k = A - v_k (ap, ap - e1, ap - e2),
// mB_k = ap_k + axis per component, e3 = e2 - e1:
//   group 0, end A:  the face (sc_face on ap, e1, e2, the triangle's acceptance), sw_vertex(ap_k) for k = 0, 1, 2,
//                    sw_edge(ap_0, e1), sw_edge(ap_0, e2), sw_edge(ap_1, e3)                        - sw_triangle's seven pieces
//   group 1, end B:  the same seven with mB_k for ap_k
//   group 2, the cylinder wall against the vertices:  sw_edge(mB_k, axis) for k = 0, 1, 2
//   group 3, the cylinder wall against the edges:  sc_face on (mB_0, e1, axis), (mB_0, e2, axis), (mB_1, e3, axis) with the
//                    parallelogram's acceptance, both weights in [0, 1]
// 6 balls, 9 cylinders, 5 faces; the time is the minimum over the pieces that accept (sw_take), + 0.0f.  A zero axis gives A = 0 in
// group 2 and a zero normal, den not > 0, in group 3: neither accepts.  A NaN never accepts.
// sc_face: sw_triangle's face block on the origin m and the spans a, b: the face on the side m starts on.
//   n = cross(a, b); nn = dot(n, n); ln = sqrtf(nn); h = dot(n, m); nd = dot(n, d); sg = h < 0 ? -1 : 1
//   num = |h| - r * ln; den = -(sg * nd); t = num / den;  only if num >= 0 && den > 0:
//   k = sg * r / ln; p_a = (m_a + d_a * t) - n_a * k; fv = dot(cross(p, b), n) / nn; fw = dot(cross(a, p), n) / nn
//   accepts iff fv >= 0 && fw >= 0 && (triangle: fv + fw <= 1; parallelogram: fv <= 1 && fw <= 1)
template <bool PARALLELOGRAM>
RT_RULE void sc_face(const float m[3], const float a[3], const float b[3], const SwQuery& q, float& best) {
    float n[3], x[3], y[3];
    sw_cross(a, b, n);
    const float nn = cp_dot(n, n), ln = sqrtf(nn), h = cp_dot(n, m), nd = cp_dot(n, q.d);
    const float sg = h < 0.0f ? -1.0f : 1.0f;
    const float num = fabsf(h) - q.r * ln, den = -(sg * nd), t = num / den;
    if (num >= 0.0f && den > 0.0f) {
        const float k = sg * q.r / ln;
        const float p[3] = {(m[0] + q.d[0] * t) - n[0] * k, (m[1] + q.d[1] * t) - n[1] * k, (m[2] + q.d[2] * t) - n[2] * k};
        sw_cross(p, b, x);
        sw_cross(a, p, y);
        const float fv = cp_dot(x, n) / nn, fw = cp_dot(y, n) / nn;
        sw_take(best, fv >= 0.0f && fw >= 0.0f && (PARALLELOGRAM ? fv <= 1.0f && fw <= 1.0f : fv + fw <= 1.0f), t);
    }
}
// the seven pieces of one end, m0 = that end - v0
RT_RULE void sc_end(const float m0[3], const float m1[3], const float m2[3], const float e1[3], const float e2[3], const float e3[3], const SwQuery& q,
                    float& best) {
    sc_face<false>(m0, e1, e2, q, best);
    sw_vertex(m0, q, best);
    sw_vertex(m1, q, best);
    sw_vertex(m2, q, best);
    sw_edge(m0, e1, q, best);
    sw_edge(m0, e2, q, best);
    sw_edge(m1, e3, q, best);
}
// the best time of each of the four groups, +inf where none of its pieces accepts; no start rule
RT_RULE void sc_pieces(const float v0[3], const float e1[3], const float e2[3], const ScQuery& q, float g[4]) {
    const float* A = q.s.c;
    const float ap[3] = {A[0] - v0[0], A[1] - v0[1], A[2] - v0[2]};
    const float m1[3] = {ap[0] - e1[0], ap[1] - e1[1], ap[2] - e1[2]}, m2[3] = {ap[0] - e2[0], ap[1] - e2[1], ap[2] - e2[2]};
    const float e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    const float b0[3] = {ap[0] + q.ax[0], ap[1] + q.ax[1], ap[2] + q.ax[2]}, b1[3] = {m1[0] + q.ax[0], m1[1] + q.ax[1], m1[2] + q.ax[2]};
    const float b2[3] = {m2[0] + q.ax[0], m2[1] + q.ax[1], m2[2] + q.ax[2]};
    g[0] = g[1] = g[2] = g[3] = INFINITY;
    sc_end(ap, m1, m2, e1, e2, e3, q.s, g[0]);
    sc_end(b0, b1, b2, e1, e2, e3, q.s, g[1]);
    sw_edge(b0, q.ax, q.s, g[2]);
    sw_edge(b1, q.ax, q.s, g[2]);
    sw_edge(b2, q.ax, q.s, g[2]);
    sc_face<true>(b0, e1, q.ax, q.s, g[3]);
    sc_face<true>(b0, e2, q.ax, q.s, g[3]);
    sc_face<true>(b1, e3, q.ax, q.s, g[3]);
}
RT_RULE float sc_triangle(const float v0[3], const float e1[3], const float e2[3], const ScQuery& q) {
    float s, v, w, g[4];
    if (cap_triangle(v0, e1, e2, q.s.c, q.ax, q.aa, s, v, w) <= q.s.rr) return 0.0f; // in contact at the start
    sc_pieces(v0, e1, e2, q, g);
    float best = g[0];
    sw_take(best, true, g[1]);
    sw_take(best, true, g[2]);
    sw_take(best, true, g[3]);
    return best + 0.0f; // a -0 counts as +0, so that bit order stays value order
}

// ---- 3. A sphere (its surface; centre C, radius R).  mA = A - C, mB = mA + axis per component, lenA = sqrtf(dot(mA, mA)), lenB
// likewise; the foot of C on the axis: f = aa > 0 ? clamp(-dot(mA, axis) / aa) : 0, pm_a = mA_a + axis_a * f, dmin = sqrtf(dot(pm, pm));
// dmax = lenB > lenA ? lenB : lenA.
//   dmin - R <= r && R - dmax <= r                       -> t = 0   (for axis == 0: sw_sphere's fabsf(len - R) <= r)
//   OUTSIDE, dmin > R: with rs = R + r in the place of the radius (rr = rs * rs), the minimum over sw_vertex(mA), sw_vertex(mB) and
//     sw_edge(mB, axis): the two ends' entering roots and the cylinder's
//   else INSIDE: rs = R - r; per end m: b = dot(m, d); x = cross(m, d); disc = dd * (rs * rs) - dot(x, x);
//     t = (-b + sqrtf(disc)) / dd, accepted iff disc >= 0 && t >= 0: the smaller of the two ends' leaving roots
//   t is that minimum + 0.0f.
// sc_sphere_s, the place on the axis of the pose at time t (A' = A + d t per component, mA', mB', f', dmin' as above from A'):
//   dmin' > R: s = f';  else s = lenB' > lenA' ? 1 : 0  (the end farther from C; A on a tie).
RT_RULE void sc_sphere_pose(const float A[3], const float centre[3], const float ax[3], float aa, float& lenA, float& lenB, float& f, float& dmin,
                            float mA[3], float mB[3]) {
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) mA[a] = A[a] - centre[a], mB[a] = mA[a] + ax[a];
    lenA = sqrtf(cp_dot(mA, mA)), lenB = sqrtf(cp_dot(mB, mB));
    f = aa > 0.0f ? sc_clamp01(-cp_dot(mA, ax) / aa) : 0.0f;
    const float pm[3] = {mA[0] + ax[0] * f, mA[1] + ax[1] * f, mA[2] + ax[2] * f};
    dmin = sqrtf(cp_dot(pm, pm));
}
RT_RULE float sc_sphere(const float centre[3], float radius, const ScQuery& q) {
    float lenA, lenB, f, dmin, mA[3], mB[3];
    sc_sphere_pose(q.s.c, centre, q.ax, q.aa, lenA, lenB, f, dmin, mA, mB);
    const float dmax = lenB > lenA ? lenB : lenA;
    if (dmin - radius <= q.s.r && radius - dmax <= q.s.r) return 0.0f;
    float best = INFINITY;
    if (dmin > radius) {
        SwQuery o = q.s;
        const float rs = radius + q.s.r;
        o.rr = rs * rs;
        sw_vertex(mA, o, best);
        sw_vertex(mB, o, best);
        sw_edge(mB, q.ax, o, best);
    } else {
        const float rs = radius - q.s.r, rr = rs * rs;
        RT_CP_UNROLL
        for (int end = 0; end < 2; end++) {
            const float* m = end ? mB : mA;
            float x[3];
            const float b = cp_dot(m, q.s.d);
            sw_cross(m, q.s.d, x);
            const float disc = q.s.dd * rr - cp_dot(x, x), t = (-b + sqrtf(disc)) / q.s.dd;
            sw_take(best, disc >= 0.0f && t >= 0.0f, t);
        }
    }
    return best + 0.0f;
}
RT_RULE float sc_sphere_s(const float centre[3], float radius, const float Ap[3], const ScQuery& q) {
    float lenA, lenB, f, dmin, mA[3], mB[3];
    sc_sphere_pose(Ap, centre, q.ax, q.aa, lenA, lenB, f, dmin, mA, mB);
    return dmin > radius ? f : lenB > lenA ? 1.0f : 0.0f;
}

// ---- 4. Order and acceptance: the sphere sweep's, cp_order on the bits of t.  The best starts at (bits of tmax, 0): only t < tmax
// is accepted, strictly; +inf never is; equal t: the lower key, spheres before triangles, each by index.

// ---- 5. The lower bound of a node's eight child boxes: the box sweep's (sb_node_bounds, restated with this query's margin so that
// the host check can flip it alone).  At the time of contact some point of the axis lies within r of the primitive, so the centre of
// the capsule's bounding box, bc + d t, lies inside the child box widened per axis by h_a = |axis_a| / 2 + r; the ray bc + d t
// enters the child box widened by wd_a = h_a + s no later than t,
//   s = RT_SWC_SLACK * ((max_a |bc_a| + max_a (|org_a| + 255 * scale_a)) + max_a h_a)
// L = tn * (1 - RT_SWC_SLACK), dead iff tx * (1 + RT_SWC_SLACK) < L; sw_pass culls a slot iff it is dead or L > best t, strictly.
// The bound is exact for the capsule's BOX, not for the capsule: loose for a long diagonal one.  Why s suffices: DESIGN.md section 4,
// "Capsule sweeps".
RT_RULE void sc_node_bounds(const uint32_t w[20], const ScQuery& q, const float inv[3], uint32_t code, float c_max, float L[8], uint32_t& alive) {
    float scale[3], on[3], of[3], m = 0.0f;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        scale[a] = ldexpf(1.0f, (int)(int8_t)((w[3] >> (8 * a)) & 0xFFu));
        m = rule_max(m, fmaf(255.0f, scale[a], fabsf(cp_float(w[a]))));
    }
    const float s = RT_SWC_SLACK * ((c_max + m) + q.hmax);
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        const float oc = cp_float(w[a]) - q.bc[a], wd = q.h[a] + s;
        const bool neg = (code >> a) & 1u;
        on[a] = neg ? oc + wd : oc - wd;
        of[a] = neg ? oc - wd : oc + wd;
    }
    alive = 0u;
    RT_CP_UNROLL
    for (int sl = 0; sl < 8; sl++) {
        float tn = 0.0f, tx = INFINITY;
        RT_CP_UNROLL
        for (int a = 0; a < 3; a++) {
            const float lo = (float)((w[8 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xFFu);
            const float hi = (float)((w[14 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xFFu);
            const bool neg = (code >> a) & 1u;
            tn = rule_max(tn, fmaf(neg ? hi : lo, scale[a], on[a]) * inv[a]);
            tx = rule_min(tx, fmaf(neg ? lo : hi, scale[a], of[a]) * inv[a]);
        }
        L[sl] = tn * (1.0f - RT_SWC_SLACK);
        if (!(tx * (1.0f + RT_SWC_SLACK) < L[sl])) alive |= 1u << sl;
    }
}

// ---- 6. The walk: group_walk visited by the best time so far, with the direction's octant for every node's code.
struct ScVisit {
    const ScQuery& q;
    float c_max, inv[3], L[8];
    uint32_t code, alive;
    CpBest& best;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        sc_node_bounds(w, q, inv, code, c_max, L, alive);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return sw_pass(L, sw_best_t(best.order), occupied & alive); }
    template <class Access>
    RT_RULE bool leaf(Access&, uint32_t slot, const float rec[9], const uint32_t ids[3]) {
        const uint64_t c = cp_order(sc_triangle(rec, rec + 3, rec + 6, q), ids[1] ^ RT_PRIM_SPHERE_FLAG);
        if (c < best.order) best.order = c, best.slot = slot;
        return false;
    }
};
template <class Access>
RT_RULE void sc_walk(Access& acc, uint32_t n_nodes, const ScQuery& q, CpBest& best) {
    ScVisit v{q, cp_p_max(q.bc), {1.0f / q.s.d[0], 1.0f / q.s.d[1], 1.0f / q.s.d[2]}, {}, sw_octant(q.s.d), 0u, best};
    group_walk(acc, n_nodes, v);
}

// ---- 7. The answer, as the eight words of an rt_capsule_sweep_hit: position | t | s | 0 | prim_id as rt_hit | the record's material
// id, unchecked.  s and position = v0 + (e1 v + e2 w) are cap_triangle of the winner at A' = A + d t (per component A_a + d_a * t): a
// contact at t = 0 carries the closest pair of the start pose.  For a sphere s = sc_sphere_s at A' and position is cp_sphere's point
// from A'_a + axis_a * s.  Nothing accepted: position 0, tmax as given, s = 0, 0, prim_id 0xFFFFFFFF, material 0.
RT_RULE void sc_answer_miss(float tmax, uint32_t out[8]) { cp_answer_miss(tmax, out); }
RT_RULE void sc_answer_triangle(const float rec[9], uint32_t material_id, uint64_t order, const ScQuery& q, uint32_t out[8]) {
    float Ap[3], s, v, w, pos[3];
    sw_centre(q.s, sw_best_t(order), Ap);
    (void)cap_triangle(rec, rec + 3, rec + 6, Ap, q.ax, q.aa, s, v, w);
    cp_triangle_position(rec, rec + 3, rec + 6, v, w, pos);
    out[0] = cp_bits(pos[0]), out[1] = cp_bits(pos[1]), out[2] = cp_bits(pos[2]), out[3] = (uint32_t)(order >> 32);
    out[4] = cp_bits(s), out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}
RT_RULE void sc_answer_sphere(const float centre[3], float radius, uint32_t material_id, uint64_t order, const ScQuery& q, uint32_t out[8]) {
    float Ap[3], pos[3];
    sw_centre(q.s, sw_best_t(order), Ap);
    const float s = sc_sphere_s(centre, radius, Ap, q);
    const float p[3] = {Ap[0] + q.ax[0] * s, Ap[1] + q.ax[1] * s, Ap[2] + q.ax[2] * s};
    (void)cp_sphere(centre, radius, p, pos);
    out[0] = cp_bits(pos[0]), out[1] = cp_bits(pos[1]), out[2] = cp_bits(pos[2]), out[3] = (uint32_t)(order >> 32);
    out[4] = cp_bits(s), out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}

} // namespace rt
#endif
