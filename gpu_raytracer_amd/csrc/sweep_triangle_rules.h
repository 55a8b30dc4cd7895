// sweep_triangle_rules.h — the triangle sweep (rt_sweep_triangle, include/rt_hip.h "Triangle sweeps"), stated once.
//
// Two pieces of code answer it: the kernel (sweep_triangle.hip) and the host walk of tests/check_sweep_triangle.cpp, which holds the
// whole walk to a brute force over all primitives before any kernel runs.  Both call what is here: the time of first contact of a
// caller's triangle in translation with a triangle and with a sphere of the scene, the order among candidates, the node bound and the
// visitor that group_walk (group_walk.h) runs.  It builds on overlap_triangle_rules.h (the 23 axes, ot_cross, ot_sphere), on
// sweep_box_rules.h (SbSpan, sb_over, sb_node_bounds, the answer's words) and on sweep_rules.h (sw_triangle for a sphere met from
// outside, the order, the octant).  Every operation is one f32 rounding and nothing is fused in the answer (the build uses
// -ffp-contract=off; the only fused operations are in the node bound), so numpy reproduces the bits (tests/sweep_triangle_cases.py).
// dot is cp_dot, cross is ot_cross.  Every test is stated in its POSITIVE form, so that a NaN makes it false.  The answer does not
// depend on the tree: the walk only culls, and the leaf test's early returns end a test whose outcome is already decided.
//
// ---- 1. A query.  Vertices q0, q1, q2 at t = 0;  u1 = q1 - q0,  u2 = q2 - q0,  u3 = u2 - u1;  qlo, qhi the per-axis min and max of
// the three vertices (exact);  d the direction and tmax.  The triangle at time t is q_k + d t.  A finite degenerate triangle - a
// segment, a point - is allowed.  A miss without a walk (st_query_valid): a non-finite component of a vertex or of d, a zero d, a tmax
// that is NaN or <= 0.
//
// ---- 2. A triangle of the scene, from its record's v0, e1, e2:  s0 = v0, s1 = v0 + e1, s2 = v0 + e2;  f1 = e1, f2 = e2,
// f3 = e2 - e1;  a_k = s_k - q0, as ot_triangle has them.  Two convex bodies in translation touch at t iff no axis of a complete
// static axis set separates them at t, and the axes of ot_triangle do not depend on position: each gives an interval of t and the
// contact is the intersection of the intervals with t >= 0.  The 26 axes, whose numbers are rt_triangle_sweep_hit.axis:
//   0, 1, 2             the coordinate axes
//   3                   nS = cross(f1, f2)
//   4                   nQ = cross(u1, u2)
//   5 + 3(i-1) + (j-1)  cross(u_i, f_j)
//   14, 15, 16          cross(nQ, u_i)         17, 18, 19   cross(nS, f_j)        (these six decide coplanar pairs)
//   20, 21, 22          cross(nS, u_i)         23, 24, 25   cross(nQ, f_j)        (these six decide a pair one of which is a segment)
// Per axis, the span (lo, hi) of the scene's triangle relative to the query's and the projection w of d:
//   coordinate axis a:  lo = min_k s_k[a] - qhi[a],  hi = max_k s_k[a] - qlo[a],  w = d[a]
//   axis L of the 23:   pS_k = dot(L, a_k),  pQ = (0, dot(L, u1), dot(L, u2)),  lo = min pS - max pQ,  hi = max pS - min pQ,
//                       w = dot(L, d);  it holds only if ((pS_0 + pS_1) + pS_2) + (pQ_1 + pQ_2) is not a NaN (ot_span's sum)
// and then sb_axis' rule (st_axis), on the running entry (t_in, axis, w_in), which starts at (0, NONE, 0), and t_out, from +inf:
//   w > 0:   enter = lo / w, exit = hi / w          w < 0:   enter = hi / w, exit = lo / w
//            the axis HOLDS iff enter <= exit; it replaces the running entry iff enter > t_in, strictly; t_out = ov_min(t_out, exit)
//   w == 0:  the axis holds iff lo <= 0 && hi >= 0; it constrains nothing
//   else (w a NaN): the axis does not hold
// CONTACT iff all nine components of the s_k are finite, every axis holds and t_in <= t_out.  Then t = t_in + 0.0f (a -0 counts as +0,
// so that bit order stays value order) and axis is the one that set t_in: at equal enter the lowest number.  No contact: t = +inf.
// At the start: the sign of a rounded difference is exact, so lo <= 0 iff min <= max' and hi >= 0 iff max >= min' for the two
// operands of each, which are ot_triangle's own (test 1 for the coordinate axes, ot_span for the 23, the NaN sum word for word), and a
// quotient by w has the sign of its operands.  If every axis passes ot_triangle's test, every enter is <= 0 and every exit >= 0: no
// axis replaces the entry, t_out >= 0, and the pass gives (0, NONE).  If some axis fails it, that axis has enter > 0 (t > 0 if there
// is contact at all), exit < 0 (t_in > t_out: none), or w == 0 and does not hold.  Hence (t = 0, NONE) results for a record EXACTLY
// WHEN rt_overlap_triangle lists it for q0, q1, q2, and a t = 0 with another axis is impossible; the static test is not evaluated a
// second time.  Two remarks on "exactly", both outside what a finite scene and a sane direction reach: where both operands of a
// difference overflow to the same infinity the difference is a NaN and the axis does not hold here while <= holds there (this errs on
// the side of not reporting); and an enter lo / w that underflows to 0 needs |w| > 2^126 lo.
// A zero axis (a degenerate triangle, parallel edges) has lo = hi = w = 0 and holds as 0 <= 0: it never sets t_in.
// The normal (st_axis_normal), L the closing axis' vector as the statement computed it:
//   normal_a = (w_in > 0 ? -L_a : L_a) / sqrtf(dot(L, L)) + 0.0f      (against the motion; the + 0.0f turns a -0 into +0)
// and 0 for NONE, and 0 in all three components where that length is not finite or not > 0: dot(L, L) can underflow to 0 or
// overflow for an axis that still closed (w != 0), and a direction nobody can trust is not reported.
// The early returns (sb_over): a test may end as "no contact" once some axis does not hold, t_in > t_out, or t_in > limit for the
// best time of the walk so far, strictly.  t_in only grows and t_out only shrinks over the axes, so the first two are final; a
// candidate later than the best is never accepted (rule 4) whichever time it carries.  Neither changes an answer.  The three
// coordinate axes come first: most records a walk reaches end there.
// Three limits:
//   - Two DEGENERATE triangles (each a segment or a point) may be reported although they never meet: every axis of the 23 is the zero
//     vector or does not separate them, and the coordinate axes alone decide (ot_triangle's first limit, carried over).
//   - "Closed" means closed on the RECORD: the scene's vertices are s_k as computed above, one rounding from the uploaded ones.
//   - Two COPLANAR triangles moving inside their common plane: nS and nQ have w == 0 exactly only where the plane's coordinates are
//     exact (a coordinate plane, say).  Elsewhere the rounded w is a small non-zero number and the answer is that of a pair tilted by
//     rounding: exact for that pair, and within the float64 sandwich of tests/test_sweep_triangle_abi.py of the untilted one.
//
// ---- 3. A sphere (o, R), a surface as everywhere; rr = R * R, near2 and far2 as ot_sphere has them, dd = dot(d, d):
//   ot_sphere(o, R, q) holds (near2 <= rr && far2 >= rr)      -> t = 0, axis NONE
//   OUTSIDE, near2 > rr:  sw_triangle(q0, u1, u2, .) for a ball of radius R that starts at o and moves by -d (the negation is exact):
//       the first entry of the centre into the query triangle's Minkowski sum with the ball
//   INSIDE, far2 < rr:  the triangle lies inside the ball and touches when a vertex reaches the surface: the minimum over k of
//       m = o - q_k;  disc = dd * rr - dot(cross(m, d), cross(m, d));  t = (dot(m, d) + sqrtf(disc)) / dd   (the leaving root),
//       accepted iff disc >= 0 && t >= 0
//   neither (a NaN): no contact.  The candidate is best + 0.0f, +inf when no piece accepts; axis = SPHERE (26) for t > 0.
//   near2 is cp_triangle's, for a degenerate query too: where its edge rule divides 0 by 0 (q1 == q0 with the closest point not at
//   q0) near2 is a NaN and the sphere is not met, at the start or later - ot_sphere's behaviour, carried over and not mended here:
//   the fourth limit of rt_hip.h.  A segment given as q2 == q1 or q2 == q0, and a point, have no such case: a rule of cp_triangle
//   that is evaluated without a quotient of zeros holds wherever the centre lies (tests/test_sweep_triangle_abi.py).
// The normal (st_sphere_normal), a unit vector against the motion: with P_a = o_a - d_a * t the sphere's centre seen from the
// triangle at the time of contact, outside it is v = (u1 v + u2 w) - (P - q0) for cp_triangle(q0, u1, u2, P)'s v, w: from the
// sphere's centre to the point of the triangle that touches it.  Inside it is v = P - q_k for the vertex farthest from P (the
// largest dot(q_k - P, q_k - P), the lowest k at a tie), the touching one.  normal = v / sqrtf(dot(v, v)) if that length is > 0,
// else 0.  A piece that gives t = 0 is a start in contact like any other: axis NONE and normal 0 for every sphere contact at t = 0.
//
// ---- 4. Order and acceptance: rt_sweep_box's, cp_order on the bits of t.  The best starts at (bits of tmax, 0): only t < tmax is
// accepted, strictly; +inf never is; equal t: the lower key, spheres before triangles, each by index.
//
// ---- 5. The node bound: sb_node_bounds on the box of the query's bounds,
//   c_a = qlo_a * 0.5f + qhi_a * 0.5f   (cannot overflow),   h_a = ov_max(qhi_a - c_a, c_a - qlo_a)
// The coordinate axes are three of the 26, so the statement's t is at or after the entry of the record's own bounds into [qlo, qhi]
// moving by -d, as the statement rounds it, and the child box contains those bounds.  [c - h, c + h] holds [qlo, qhi] up to the
// rounding of c and of h, one each, of the size of the coordinates: 2^-24 of magnitudes that RT_SWB_SLACK multiplies by 1e-5
// ("Triangle sweeps", redoes the count).  A NaN plane (0 * inf where a bound lies in a plane, an overflowing
// grid) is dropped by max / min; a margin s that overflows makes every near plane -inf and every far plane +inf, so every slot is
// followed: both cost visits, never an answer.
#ifndef RT_SWEEP_TRIANGLE_RULES_H
#define RT_SWEEP_TRIANGLE_RULES_H

#include "overlap_triangle_rules.h"
#include "sweep_box_rules.h"

namespace rt {

// rt_triangle_sweep_hit.axis: RT_SWEEP_AXIS_NONE is SB_AXIS_NONE; RT_SWEEP_TRIANGLE_AXIS_SPHERE of rt_hip.h
constexpr uint32_t ST_AXIS_SPHERE = 26u;

// rule 1.  What the walk keeps: q0, u1, u2, the bounds, and in `b` the bound's box with d, dd and tmax.  q1 and q2 are read for the
// spheres alone and are not kept.
struct StQuery {
    float q0[3], u1[3], u2[3], lo[3], hi[3];
    SbQuery b; // c, h of rule 5; d; hmax; dd; tmax
};
RT_RULE bool st_query_valid(const float q0[3], const float q1[3], const float q2[3], const float d[3], float tmax) {
    bool ok = true, moving = false;
    for (int a = 0; a < 3; a++) ok = ok && ov_finite(q0[a]) && ov_finite(q1[a]) && ov_finite(q2[a]) && ov_finite(d[a]), moving = moving || d[a] != 0.0f;
    return ok && moving && tmax > 0.0f;
}
RT_RULE StQuery st_query(const float q0[3], const float q1[3], const float q2[3], const float d[3], float tmax) {
    StQuery q;
    float c[3], h[3];
    for (int a = 0; a < 3; a++) {
        q.q0[a] = q0[a], q.u1[a] = q1[a] - q0[a], q.u2[a] = q2[a] - q0[a];
        q.lo[a] = ov_min(ov_min(q0[a], q1[a]), q2[a]), q.hi[a] = ov_max(ov_max(q0[a], q1[a]), q2[a]);
        c[a] = q.lo[a] * 0.5f + q.hi[a] * 0.5f;
        h[a] = ov_max(q.hi[a] - c[a], c[a] - q.lo[a]);
    }
    q.b = sb_query(c, h, d, tmax);
    return q;
}

// rule 2
RT_RULE void st_axis(SbSpan& s, uint32_t axis, float lo, float hi, float w) {
    if (w > 0.0f || w < 0.0f) {
        const float enter = (w > 0.0f ? lo : hi) / w, exit = (w > 0.0f ? hi : lo) / w;
        s.ok = s.ok && enter <= exit;
        if (enter > s.t_in) s.t_in = enter, s.axis = axis, s.w_in = w;
        s.t_out = ov_min(s.t_out, exit);
    } else {
        s.ok = s.ok && w == 0.0f && lo <= 0.0f && hi >= 0.0f;
    }
}
struct StPair { // what every axis of a pair is projected on
    float a0[3], a1[3], a2[3];
    const float *u1, *u2, *d;
};
RT_RULE void st_span(SbSpan& s, uint32_t axis, const StPair& p, const float L[3]) {
    const float s0 = cp_dot(L, p.a0), s1 = cp_dot(L, p.a1), s2 = cp_dot(L, p.a2), t1 = cp_dot(L, p.u1), t2 = cp_dot(L, p.u2);
    const float sum = ((s0 + s1) + s2) + (t1 + t2);
    s.ok = s.ok && sum == sum;
    st_axis(s, axis, ov_min(ov_min(s0, s1), s2) - ov_max(ov_max(0.0f, t1), t2), ov_max(ov_max(s0, s1), s2) - ov_min(ov_min(0.0f, t1), t2), cp_dot(L, p.d));
}
// the three axes first, first + 1, first + 2 = cross(n, g_j)
RT_RULE void st_axes_with(SbSpan& s, uint32_t first, const StPair& p, const float n[3], const float g1[3], const float g2[3], const float g3[3]) {
    float L[3];
    ot_cross(n, g1, L);
    st_span(s, first, p, L);
    ot_cross(n, g2, L);
    st_span(s, first + 1u, p, L);
    ot_cross(n, g3, L);
    st_span(s, first + 2u, p, L);
}
// the time of first contact, +inf when there is none or when it is later than `limit`; axis and w_in of the axis that set it
RT_RULE float st_triangle(const float v0[3], const float e1[3], const float e2[3], const StQuery& q, float limit, uint32_t& axis, float& w_in) {
    StPair p;
    SbSpan s{0.0f, INFINITY, 0.0f, SB_AXIS_NONE, true};
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        const float s0 = v0[a], s1 = v0[a] + e1[a], s2 = v0[a] + e2[a];
        s.ok = s.ok && ov_finite(s0) && ov_finite(s1) && ov_finite(s2);
        st_axis(s, (uint32_t)a, ov_min(ov_min(s0, s1), s2) - q.hi[a], ov_max(ov_max(s0, s1), s2) - q.lo[a], q.b.d[a]);
        p.a0[a] = s0 - q.q0[a], p.a1[a] = s1 - q.q0[a], p.a2[a] = s2 - q.q0[a];
    }
    axis = SB_AXIS_NONE, w_in = 0.0f;
    if (sb_over(s, limit)) return INFINITY; // most records a walk reaches end here
    p.u1 = q.u1, p.u2 = q.u2, p.d = q.b.d;
    float nS[3], nQ[3];
    ot_cross(e1, e2, nS);
    st_span(s, 3u, p, nS);
    ot_cross(q.u1, q.u2, nQ);
    st_span(s, 4u, p, nQ);
    if (sb_over(s, limit)) return INFINITY;
    const float f3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    const float u3[3] = {q.u2[0] - q.u1[0], q.u2[1] - q.u1[1], q.u2[2] - q.u1[2]};
    st_axes_with(s, 5u, p, q.u1, e1, e2, f3);
    if (sb_over(s, limit)) return INFINITY;
    st_axes_with(s, 8u, p, q.u2, e1, e2, f3);
    if (sb_over(s, limit)) return INFINITY;
    st_axes_with(s, 11u, p, u3, e1, e2, f3);
    if (sb_over(s, limit)) return INFINITY;
    st_axes_with(s, 14u, p, nQ, q.u1, q.u2, u3);
    st_axes_with(s, 17u, p, nS, e1, e2, f3);
    if (sb_over(s, limit)) return INFINITY;
    st_axes_with(s, 20u, p, nS, q.u1, q.u2, u3);
    st_axes_with(s, 23u, p, nQ, e1, e2, f3);
    if (sb_over(s, limit)) return INFINITY;
    axis = s.axis, w_in = s.w_in;
    return s.t_in + 0.0f;
}
// the vector of axis 0 .. 25 as st_triangle computed it; no array is indexed by `axis`: registers
RT_RULE void st_axis_vector(const float e1[3], const float e2[3], const StQuery& q, uint32_t axis, float L[3]) {
    L[0] = axis == 0u ? 1.0f : 0.0f, L[1] = axis == 1u ? 1.0f : 0.0f, L[2] = axis == 2u ? 1.0f : 0.0f;
    if (axis < 3u || axis > 25u) return;
    float nS[3], nQ[3], f[3], u[3];
    ot_cross(e1, e2, nS);
    ot_cross(q.u1, q.u2, nQ);
    const uint32_t k = axis < 5u ? 0u : (axis - 5u) % 3u, g = axis < 5u ? 0u : (axis - 5u) / 3u; // g: the group of three, k: its member
    const uint32_t i = g < 3u ? g : k, j = k; // cross(u_i, f_j) has i = g, j = k; the other groups use one of the two
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        f[a] = j == 0u ? e1[a] : j == 1u ? e2[a] : e2[a] - e1[a];
        u[a] = i == 0u ? q.u1[a] : i == 1u ? q.u2[a] : q.u2[a] - q.u1[a];
    }
    if (axis == 3u) L[0] = nS[0], L[1] = nS[1], L[2] = nS[2];
    else if (axis == 4u) L[0] = nQ[0], L[1] = nQ[1], L[2] = nQ[2];
    else if (g < 3u) ot_cross(u, f, L);
    else if (g == 3u) ot_cross(nQ, u, L);
    else if (g == 4u) ot_cross(nS, f, L);
    else if (g == 5u) ot_cross(nS, u, L);
    else ot_cross(nQ, f, L);
}
RT_RULE void st_axis_normal(const float e1[3], const float e2[3], const StQuery& q, uint32_t axis, float w_in, float normal[3]) {
    float L[3];
    st_axis_vector(e1, e2, q, axis, L);
    const float len = sqrtf(cp_dot(L, L));
    const bool ok = axis < 26u && len > 0.0f && len < INFINITY;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) normal[a] = ok ? (w_in > 0.0f ? -L[a] : L[a]) / len + 0.0f : 0.0f;
}

// rule 3.  q1, q2: the query's other two vertices as given.
RT_RULE float st_sphere(const float centre[3], float radius, const StQuery& q, const float q1[3], const float q2[3]) {
    float v, w, m[3][3], x[3];
    const float near2 = cp_triangle(q.q0, q.u1, q.u2, centre, v, w);
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) m[0][a] = centre[a] - q.q0[a], m[1][a] = centre[a] - q1[a], m[2][a] = centre[a] - q2[a];
    // dot(q_k - o, q_k - o) of ot_sphere: the products of the negated differences are the same numbers
    const float far2 = ov_max(ov_max(cp_dot(m[0], m[0]), cp_dot(m[1], m[1])), cp_dot(m[2], m[2]));
    const float rr = radius * radius;
    if (near2 <= rr && far2 >= rr) return 0.0f;
    float best = INFINITY;
    if (near2 > rr) {
        const float back[3] = {-q.b.d[0], -q.b.d[1], -q.b.d[2]};
        return sw_triangle(q.q0, q.u1, q.u2, sw_query(centre, radius, back, q.b.tmax));
    } else if (far2 < rr) {
        RT_CP_UNROLL
        for (int k = 0; k < 3; k++) {
            sw_cross(m[k], q.b.d, x);
            const float disc = q.b.dd * rr - cp_dot(x, x);
            const float t = (cp_dot(m[k], q.b.d) + sqrtf(disc)) / q.b.dd;
            sw_take(best, disc >= 0.0f && t >= 0.0f, t);
        }
    }
    return best + 0.0f;
}
RT_RULE void st_sphere_normal(const float centre[3], float radius, const StQuery& q, const float q1[3], const float q2[3], float t, float normal[3]) {
    float v, w, P[3], ap[3], far[3], best = -1.0f;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) P[a] = centre[a] - q.b.d[a] * t, ap[a] = P[a] - q.q0[a];
    const bool outside = cp_triangle(q.q0, q.u1, q.u2, centre, v, w) > radius * radius; // rule 3's case, at the start
    (void)cp_triangle(q.q0, q.u1, q.u2, P, v, w);
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) normal[a] = (q.u1[a] * v + q.u2[a] * w) - ap[a], far[a] = 0.0f;
    if (!outside) {
        RT_CP_UNROLL
        for (int k = 0; k < 3; k++) {
            const float* qk = k == 0 ? q.q0 : k == 1 ? q1 : q2;
            const float g[3] = {qk[0] - P[0], qk[1] - P[1], qk[2] - P[2]};
            const float far2 = cp_dot(g, g);
            if (far2 > best) best = far2, far[0] = P[0] - qk[0], far[1] = P[1] - qk[1], far[2] = P[2] - qk[2];
        }
        normal[0] = far[0], normal[1] = far[1], normal[2] = far[2];
    }
    const float len = sqrtf(cp_dot(normal, normal));
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) normal[a] = len > 0.0f ? normal[a] / len : 0.0f;
}

// rule 5: SbVisit with this file's leaf test
struct StVisit {
    const StQuery& q;
    float c_max, inv[3], L[8];
    uint32_t code, alive;
    CpBest& best;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        sb_node_bounds(w, q.b, inv, code, c_max, L, alive);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return sw_pass(L, sw_best_t(best.order), occupied & alive); }
    template <class Access>
    RT_RULE bool leaf(Access&, uint32_t slot, const float rec[9], const uint32_t ids[3]) {
        uint32_t axis;
        float w_in;
        const uint64_t c = cp_order(st_triangle(rec, rec + 3, rec + 6, q, sw_best_t(best.order), axis, w_in), ids[1] ^ RT_PRIM_SPHERE_FLAG);
        if (c < best.order) best.order = c, best.slot = slot;
        return false;
    }
};
template <class Access>
RT_RULE void st_walk(Access& acc, uint32_t n_nodes, const StQuery& q, CpBest& best) {
    StVisit v{q, cp_p_max(q.b.c), {1.0f / q.b.d[0], 1.0f / q.b.d[1], 1.0f / q.b.d[2]}, {}, sw_octant(q.b.d), 0u, best};
    group_walk(acc, n_nodes, v);
}

// ---- 6. The answer, as the eight words of an rt_triangle_sweep_hit (rt_box_sweep_hit's layout): normal | t | axis | 0 | prim_id as
// rt_hit | the record's material id, unchecked.  Normal and axis are the winner's statement evaluated once more, with no limit; they
// are not carried through the walk.  Nothing accepted: sb_answer_miss - normal 0, tmax as given, NONE, 0, 0xFFFFFFFF, 0.
RT_RULE void st_answer_triangle(const float rec[9], uint32_t material_id, uint64_t order, const StQuery& q, uint32_t out[8]) {
    uint32_t axis;
    float w_in, normal[3];
    (void)st_triangle(rec, rec + 3, rec + 6, q, INFINITY, axis, w_in);
    st_axis_normal(rec + 3, rec + 6, q, axis, w_in, normal);
    out[0] = cp_bits(normal[0]), out[1] = cp_bits(normal[1]), out[2] = cp_bits(normal[2]), out[3] = (uint32_t)(order >> 32);
    out[4] = axis, out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}
RT_RULE void st_answer_sphere(const float centre[3], float radius, uint32_t material_id, uint64_t order, const StQuery& q, const float q1[3], const float q2[3],
                              uint32_t out[8]) {
    const float t = sw_best_t(order);
    float normal[3] = {0.0f, 0.0f, 0.0f};
    if (t > 0.0f) st_sphere_normal(centre, radius, q, q1, q2, t, normal);
    out[0] = cp_bits(normal[0]), out[1] = cp_bits(normal[1]), out[2] = cp_bits(normal[2]), out[3] = (uint32_t)(order >> 32);
    out[4] = t > 0.0f ? ST_AXIS_SPHERE : SB_AXIS_NONE, out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}

} // namespace rt
#endif
