// sweep_box_rules.h — the box sweep (rt_sweep_box, include/rt_hip.h "Box sweeps"), stated once.
//
// Two pieces of code answer it: the kernel (sweep_box.hip) and the host walk of tests/check_sweep_box.cpp, which holds the whole walk
// to a brute force over all primitives before any kernel runs.  Both call what is here: the time of first contact of a moving
// axis-aligned box with a triangle and with a sphere, the order among candidates, the lower bound of a node's eight child boxes
// widened by the half extents, and the visitor that group_walk (group_walk.h) runs.  It builds on overlap_rules.h (the thirteen axes
// and their forms, ov_min / ov_max / ov_finite, ov_sphere) and on sweep_rules.h (sw_cross, the order, the octant).  Every operation is
// one f32 rounding and nothing is fused in the answer (the build uses -ffp-contract=off; the only fused operations are written fmaf,
// and they are in the box bound), so numpy reproduces the bits (tests/sweep_box_cases.py).
//
// Every test is stated in its POSITIVE form, so that a NaN makes it false and the primitive is not touched.  The answer does not
// depend on the tree: the walk only culls, and the leaf test's early returns (rule 1) end a test whose outcome is already decided.
#ifndef RT_SWEEP_BOX_RULES_H
#define RT_SWEEP_BOX_RULES_H

#include "overlap_rules.h"
#include "sweep_rules.h"

namespace rt {

// The margin of the box bound: relative to the magnitudes that enter it in space, and relative to the entry time (sb_node_bounds).
#ifndef RT_SWB_SLACK
#define RT_SWB_SLACK 1.0e-5f
#endif

// rt_box_sweep_hit.axis: RT_SWEEP_AXIS_NONE and RT_SWEEP_AXIS_SPHERE of rt_hip.h
constexpr uint32_t SB_AXIS_NONE = 0xFFFFFFFFu, SB_AXIS_SPHERE = 13u;

// One query: the box's centre c at t = 0, its half extents h, the direction d and what every piece needs of them.
struct SbQuery {
    float c[3], h[3], d[3], hmax, dd, tmax;
};
RT_RULE SbQuery sb_query(const float center[3], const float half_extent[3], const float direction[3], float tmax) {
    SbQuery q;
    for (int a = 0; a < 3; a++) q.c[a] = center[a], q.h[a] = half_extent[a], q.d[a] = direction[a];
    q.hmax = ov_max(ov_max(half_extent[0], half_extent[1]), half_extent[2]);
    q.dd = cp_dot(direction, direction), q.tmax = tmax;
    return q;
}
// a query that is a miss without a walk: a non-finite component of centre, half extent or direction, a negative half extent, a zero
// direction, a tmax that is NaN or <= 0
RT_RULE bool sb_query_valid(const SbQuery& q) {
    bool ok = true, moving = false;
    for (int a = 0; a < 3; a++) ok = ok && ov_finite(q.c[a]) && ov_finite(q.h[a]) && ov_finite(q.d[a]) && q.h[a] >= 0.0f, moving = moving || q.d[a] != 0.0f;
    return ok && moving && q.tmax > 0.0f;
}

// ---- 1. A triangle, from its record's v0, e1, e2.  Relative to the centre at t = 0 its vertices are ov_triangle's
//   a0 = v0 - c,  a1 = (v0 + e1) - c,  a2 = (v0 + e2) - c
// and seen from the box they move by -d t.  Two convex bodies in translation touch iff they are separated on none of the thirteen
// axes of the static test, so each axis gives an interval of t and the contact is the intersection of the intervals with t >= 0.
// The axes, in this order, with their projections p_k of the vertices, the box's radius r and the projection w of d, each in the
// overlap statement's own form:
//   0, 1, 2   the box axes:  p_k = a_k[a];  r = h[a];  w = d[a]
//   3         n = cross(e1, e2):  p_0 = p_1 = p_2 = dot(n, a0);  r = dot(|n|, h);  w = dot(n, d)
//   4 + 3j + i   cross(unit_i, f_j), f = (e1, e2 - e1, e2), for f = f_j and g = |f| per component (ov_cross_axes):
//        i = x:  p_k = f.y * a_k.z - f.z * a_k.y;  r = g.z * h.y + g.y * h.z;  w = f.y * d.z - f.z * d.y
//        i = y:  p_k = f.z * a_k.x - f.x * a_k.z;  r = g.z * h.x + g.x * h.z;  w = f.z * d.x - f.x * d.z
//        i = z:  p_k = f.x * a_k.y - f.y * a_k.x;  r = g.y * h.x + g.x * h.y;  w = f.x * d.y - f.y * d.x
// Per axis (sb_axis), with pmin = min_k p_k, pmax = max_k p_k (ov_min, ov_max), lo = pmin - r, hi = pmax + r:
//   w > 0:   enter = lo / w, exit = hi / w          w < 0:   enter = hi / w, exit = lo / w
//            the axis HOLDS iff enter <= exit (false for a NaN); it replaces the running entry (t_in, axis, w_in), which starts at
//            (0, NONE, 0), iff enter > t_in, strictly; t_out, which starts at +inf, becomes ov_min(t_out, exit)
//   w == 0:  the axis holds iff pmin <= r && pmax >= -r, the overlap statement's test; it constrains nothing
//   else (w a NaN): the axis does not hold
// and an axis 4..12 holds only if (p_0 + p_1) + p_2 is no NaN (ov_span's check of its three projections).
// CONTACT iff all nine components of a0, a1, a2 are finite, every axis holds and t_in <= t_out.  Then t = t_in + 0.0f (a -0 counts as
// +0, so that bit order stays value order) and axis is the one that set t_in.  No contact: t = +inf.
// At the start: the sign of a rounded difference is exact, so lo <= 0 iff pmin <= r and hi >= 0 iff pmax >= -r, and a quotient has
// the sign of its operands.  Hence every enter is <= 0 and every exit >= 0 exactly when every axis passes ov_triangle's own test:
// the pass gives (t = 0, NONE) iff ov_triangle(v0, e1, e2, c, h) holds, and a t = 0 otherwise is impossible.  The static test
// is not evaluated a second time.
// A zero axis (a degenerate triangle, an edge along a unit axis) has w == 0 and holds as 0 <= 0: it never sets t_in.
// The normal (sb_axis_normal): L the axis' vector - unit_a; n; (0, -f.z, f.y), (f.z, 0, -f.x), (-f.y, f.x, 0) for i = x, y, z - and
//   normal_a = (w_in > 0 ? -L_a : L_a) / sqrtf(dot(L, L)) + 0.0f      (against the motion; the + 0.0f turns a -0 into +0)
// and 0 for NONE.
// The early returns: a test may end as "no contact" once some axis does not hold, t_in > t_out, or t_in > limit for the best time of
// the walk so far, strictly.  t_in only grows and t_out only shrinks over the axes, so the first two are final; a candidate later
// than the best is never accepted (rule 3) whichever time it carries.  Neither changes an answer.
struct SbSpan {
    float t_in, t_out, w_in;
    uint32_t axis;
    bool ok;
};
RT_RULE void sb_axis(SbSpan& s, uint32_t axis, float pmin, float pmax, float r, float w) {
    const float lo = pmin - r, hi = pmax + r;
    if (w > 0.0f || w < 0.0f) {
        const float enter = (w > 0.0f ? lo : hi) / w, exit = (w > 0.0f ? hi : lo) / w;
        s.ok = s.ok && enter <= exit;
        if (enter > s.t_in) s.t_in = enter, s.axis = axis, s.w_in = w;
        s.t_out = ov_min(s.t_out, exit);
    } else {
        s.ok = s.ok && w == 0.0f && pmin <= r && pmax >= -r;
    }
}
RT_RULE void sb_span(SbSpan& s, uint32_t axis, float p0, float p1, float p2, float r, float w) {
    const float sum = (p0 + p1) + p2;
    s.ok = s.ok && sum == sum;
    sb_axis(s, axis, ov_min(ov_min(p0, p1), p2), ov_max(ov_max(p0, p1), p2), r, w);
}
RT_RULE void sb_cross_axes(SbSpan& s, uint32_t first, const float f[3], const float a0[3], const float a1[3], const float a2[3], const SbQuery& q) {
    const float g[3] = {fabsf(f[0]), fabsf(f[1]), fabsf(f[2])};
    const float* h = q.h;
    const float* d = q.d;
    sb_span(s, first, f[1] * a0[2] - f[2] * a0[1], f[1] * a1[2] - f[2] * a1[1], f[1] * a2[2] - f[2] * a2[1], g[2] * h[1] + g[1] * h[2], f[1] * d[2] - f[2] * d[1]);
    sb_span(s, first + 1u, f[2] * a0[0] - f[0] * a0[2], f[2] * a1[0] - f[0] * a1[2], f[2] * a2[0] - f[0] * a2[2], g[2] * h[0] + g[0] * h[2], f[2] * d[0] - f[0] * d[2]);
    sb_span(s, first + 2u, f[0] * a0[1] - f[1] * a0[0], f[0] * a1[1] - f[1] * a1[0], f[0] * a2[1] - f[1] * a2[0], g[1] * h[0] + g[0] * h[1], f[0] * d[1] - f[1] * d[0]);
}
RT_RULE bool sb_over(const SbSpan& s, float limit) { return !s.ok || s.t_in > s.t_out || s.t_in > limit; }
// the time of first contact, +inf when there is none or when it is later than `limit`; axis and w_in of the axis that set it
// The statement is written once, over a source of the relative vertices (overlap_rules.h, OvFromRecord / OvFromRelative): sb_triangle's
// is its own subtraction from q.c, made axis by axis inside the loop as it always was; sb_triangle_rel's is a caller that has a0, a1,
// a2, e1, e2 and q.h, q.d in another frame already (obb_rules.h; q.c is not read).
template <class Rel>
RT_RULE float sb_triangle_from(const Rel& rel, const float e1[3], const float e2[3], const SbQuery& q, float limit, uint32_t& axis, float& w_in) {
    float a0[3], a1[3], a2[3];
    SbSpan s{0.0f, INFINITY, 0.0f, SB_AXIS_NONE, true};
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        rel(a, a0[a], a1[a], a2[a]);
        s.ok = s.ok && ov_finite(a0[a]) && ov_finite(a1[a]) && ov_finite(a2[a]);
        sb_axis(s, (uint32_t)a, ov_min(ov_min(a0[a], a1[a]), a2[a]), ov_max(ov_max(a0[a], a1[a]), a2[a]), q.h[a], q.d[a]);
    }
    axis = SB_AXIS_NONE, w_in = 0.0f;
    if (sb_over(s, limit)) return INFINITY; // most records a walk reaches end here
    const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float an[3] = {fabsf(n[0]), fabsf(n[1]), fabsf(n[2])};
    const float p = cp_dot(n, a0);
    sb_axis(s, 3u, p, p, cp_dot(an, q.h), cp_dot(n, q.d));
    if (sb_over(s, limit)) return INFINITY;
    const float f1[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    sb_cross_axes(s, 4u, e1, a0, a1, a2, q);
    if (sb_over(s, limit)) return INFINITY;
    sb_cross_axes(s, 7u, f1, a0, a1, a2, q);
    if (sb_over(s, limit)) return INFINITY;
    sb_cross_axes(s, 10u, e2, a0, a1, a2, q);
    if (sb_over(s, limit)) return INFINITY;
    axis = s.axis, w_in = s.w_in;
    return s.t_in + 0.0f;
}
RT_RULE float sb_triangle(const float v0[3], const float e1[3], const float e2[3], const SbQuery& q, float limit, uint32_t& axis, float& w_in) {
    return sb_triangle_from(OvFromRecord{v0, e1, e2, q.c}, e1, e2, q, limit, axis, w_in);
}
RT_RULE float sb_triangle_rel(const float a0[3], const float a1[3], const float a2[3], const float e1[3], const float e2[3], const SbQuery& q, float limit,
                              uint32_t& axis, float& w_in) {
    return sb_triangle_from(OvFromRelative{a0, a1, a2}, e1, e2, q, limit, axis, w_in);
}
RT_RULE void sb_axis_normal(const float e1[3], const float e2[3], uint32_t axis, float w_in, float normal[3]) {
    float L[3] = {axis == 0u ? 1.0f : 0.0f, axis == 1u ? 1.0f : 0.0f, axis == 2u ? 1.0f : 0.0f}; // no array is indexed by `axis`: registers
    if (axis == 3u) sw_cross(e1, e2, L);
    else if (axis > 3u && axis < 13u) {
        const uint32_t j = (axis - 4u) / 3u, i = (axis - 4u) % 3u;
        float f[3];
        RT_CP_UNROLL
        for (int a = 0; a < 3; a++) f[a] = j == 0u ? e1[a] : j == 1u ? e2[a] - e1[a] : e2[a];
        if (i == 0u) L[1] = -f[2], L[2] = f[1];
        else if (i == 1u) L[0] = f[2], L[2] = -f[0];
        else L[0] = -f[1], L[1] = f[0];
    }
    const float len = sqrtf(cp_dot(L, L));
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) normal[a] = axis < 13u ? (w_in > 0.0f ? -L[a] : L[a]) / len + 0.0f : 0.0f;
}

// ---- 2. A sphere (its surface, as everywhere; centre o, radius R, rr = R * R): g = o - c per component, so that seen from the box
// the sphere's centre is P(t) = g - d t, per component g_a - d_a * t.  With ov_sphere's near and far (gabs = |g_a|, near_a =
// ov_max(gabs - h_a, 0), far_a = gabs + h_a):
//   ov_sphere(o, R, c, h) holds                                            -> t = 0, axis NONE
//   OUTSIDE, dot(near, near) > rr: P enters the box widened by the ball; the minimum over the pieces that accept:
//     three faces: on each axis a with d_a > 0 or d_a < 0, plane = h_a + R;  t = (g_a - (d_a > 0 ? plane : -plane)) / d_a
//         accepts iff t >= 0 && |P_b(t)| <= h_b && |P_c(t)| <= h_c on the other two axes
//     twelve edges: along axis a, (b, c) = (a + 1, a + 2) mod 3, for the four signs: m_b = g_b -+ h_b, m_c = g_c -+ h_c
//         dd2 = d_b*d_b + d_c*d_c;  bq = m_b*d_b + m_c*d_c;  x = m_b*d_c - m_c*d_b;  disc = dd2*rr - x*x
//         t = (bq - sqrtf(disc)) / dd2  (the entering root);  accepts iff disc >= 0 && t >= 0 && |P_a(t)| <= h_a
//     eight corners: m = g -+ h per component;  b = dot(m, d);  x = cross(m, d);  disc = dd*rr - dot(x, x)
//         t = (b - sqrtf(disc)) / dd  (the entering root, sw_vertex' form for a point moving by -d);  accepts iff disc >= 0 && t >= 0
//   INSIDE, dot(far, far) < rr: the box lies inside the ball and touches when a corner reaches the surface: the minimum over the
//     eight corners of the leaving root t = (b + sqrtf(disc)) / dd with disc >= 0 && t >= 0
//   axis = SPHERE.  The candidate is best + 0.0f, +inf when no piece accepts.
// The pieces of edges and corners on the box's far side accept only while P is within R of the box, hence not before the first
// entry, which some piece on the near side gives; the minimum is not changed by them.
// The normal (sb_sphere_normal) at P = P(t): outside, v = clamp(P, -h, h) - P per component (ov_min(ov_max(P_a, -h_a), h_a) - P_a),
// the unit vector from the sphere's centre to the point of the box that touches it; inside, v = P - corner with corner_a = (P_a >= 0
// ? -h_a : h_a), the farthest corner, which is the touching one.  normal = v / sqrtf(dot(v, v)) if that length is > 0, else 0: a
// zero vector (a box without extent at the centre of a sphere without radius) gives no direction, and a NaN none either.
// A piece that gives t = 0 (a start within rounding of touching, which ov_sphere's squared form did not see) is a start in contact
// like any other: the answer (rule 6) reports axis NONE and normal 0 for every sphere contact at t = 0.
RT_RULE float sb_sphere(const float centre[3], float radius, const SbQuery& q) {
    if (ov_sphere(centre, radius, q.c, q.h)) return 0.0f;
    float g[3], near[3], far[3], best = INFINITY;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        g[a] = centre[a] - q.c[a];
        const float gabs = fabsf(g[a]);
        near[a] = ov_max(gabs - q.h[a], 0.0f), far[a] = gabs + q.h[a];
    }
    const float rr = radius * radius;
    const bool outside = cp_dot(near, near) > rr, inside = cp_dot(far, far) < rr;
    if (outside) {
        RT_CP_UNROLL
        for (int a = 0; a < 3; a++) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            if (q.d[a] > 0.0f || q.d[a] < 0.0f) { // the face
                const float plane = q.h[a] + radius;
                const float t = (g[a] - (q.d[a] > 0.0f ? plane : -plane)) / q.d[a];
                sw_take(best, t >= 0.0f && fabsf(g[b] - q.d[b] * t) <= q.h[b] && fabsf(g[c] - q.d[c] * t) <= q.h[c], t);
            }
            RT_CP_UNROLL
            for (int k = 0; k < 4; k++) { // the edges along a
                const float mb = (k & 1) ? g[b] + q.h[b] : g[b] - q.h[b], mc = (k & 2) ? g[c] + q.h[c] : g[c] - q.h[c];
                const float dd2 = q.d[b] * q.d[b] + q.d[c] * q.d[c], bq = mb * q.d[b] + mc * q.d[c], x = mb * q.d[c] - mc * q.d[b];
                const float disc = dd2 * rr - x * x;
                const float t = (bq - sqrtf(disc)) / dd2;
                sw_take(best, disc >= 0.0f && t >= 0.0f && fabsf(g[a] - q.d[a] * t) <= q.h[a], t);
            }
        }
    }
    if (outside || inside) {
        RT_CP_UNROLL
        for (int k = 0; k < 8; k++) { // the corners
            float m[3], x[3];
            RT_CP_UNROLL
            for (int a = 0; a < 3; a++) m[a] = ((k >> a) & 1) ? g[a] + q.h[a] : g[a] - q.h[a];
            const float b = cp_dot(m, q.d);
            sw_cross(m, q.d, x);
            const float disc = q.dd * rr - cp_dot(x, x), root = sqrtf(disc);
            const float t = (outside ? b - root : b + root) / q.dd;
            sw_take(best, disc >= 0.0f && t >= 0.0f, t);
        }
    }
    return best + 0.0f;
}
RT_RULE void sb_sphere_normal(const float centre[3], float radius, const SbQuery& q, float t, float normal[3]) {
    float near[3], v[3];
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        const float g = centre[a] - q.c[a];
        near[a] = ov_max(fabsf(g) - q.h[a], 0.0f);
        const float P = g - q.d[a] * t;
        v[a] = P; // the inside form's first operand; finished below
        normal[a] = ov_min(ov_max(P, -q.h[a]), q.h[a]) - P;
    }
    if (!(cp_dot(near, near) > radius * radius))
        RT_CP_UNROLL
        for (int a = 0; a < 3; a++) normal[a] = v[a] - (v[a] >= 0.0f ? -q.h[a] : q.h[a]);
    const float len = sqrtf(cp_dot(normal, normal));
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) normal[a] = len > 0.0f ? normal[a] / len : 0.0f;
}

// ---- 3. Order and acceptance: the sphere sweep's, cp_order on the bits of t.  The best starts at (bits of tmax, 0): only t < tmax
// is accepted, strictly; +inf never is; equal t: the lower key, spheres before triangles, each by index.

// ---- 4. The lower bound of a node's eight child boxes: sw_node_bounds with the widening per axis, wd_a = h_a + s,
//   s = RT_SWB_SLACK * ((max_a |c_a| + max_a (|org_a| + 255 * scale_a)) + max_a h_a)
// The box axes are three of the thirteen, so the statement's t lies in [enter_a, exit_a] of the triangle's own bounds widened by h_a
// as the statement rounds them, and the child box contains those bounds: the ray c + d t enters the child box widened by h_a no later
// than t.  Unlike the sphere's, this bound is exact in space - a box widened by a box is a box - and s only pays for rounding
// ("Box sweeps").  L = tn * (1 - RT_SWB_SLACK), dead iff tx * (1 + RT_SWB_SLACK) < L; sw_pass culls a slot iff it
// is dead or L > best t, strictly.
RT_RULE void sb_node_bounds(const uint32_t w[20], const SbQuery& q, const float inv[3], uint32_t code, float c_max, float L[8], uint32_t& alive) {
    float scale[3], on[3], of[3], m = 0.0f;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        scale[a] = ldexpf(1.0f, (int)(int8_t)((w[3] >> (8 * a)) & 0xFFu));
        m = rule_max(m, fmaf(255.0f, scale[a], fabsf(cp_float(w[a]))));
    }
    const float s = RT_SWB_SLACK * ((c_max + m) + q.hmax);
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        const float oc = cp_float(w[a]) - q.c[a], wd = q.h[a] + s;
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
        L[sl] = tn * (1.0f - RT_SWB_SLACK);
        if (!(tx * (1.0f + RT_SWB_SLACK) < L[sl])) alive |= 1u << sl;
    }
}

// ---- 5. The walk: group_walk visited by the best time so far, with the direction's octant for every node's code.
struct SbVisit {
    const SbQuery& q;
    float c_max, inv[3], L[8];
    uint32_t code, alive;
    CpBest& best;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        sb_node_bounds(w, q, inv, code, c_max, L, alive);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return sw_pass(L, sw_best_t(best.order), occupied & alive); }
    template <class Access>
    RT_RULE bool leaf(Access&, uint32_t slot, const float rec[9], const uint32_t ids[3]) {
        uint32_t axis;
        float w_in;
        const uint64_t c = cp_order(sb_triangle(rec, rec + 3, rec + 6, q, sw_best_t(best.order), axis, w_in), ids[1] ^ RT_PRIM_SPHERE_FLAG);
        if (c < best.order) best.order = c, best.slot = slot;
        return false;
    }
};
template <class Access>
RT_RULE void sb_walk(Access& acc, uint32_t n_nodes, const SbQuery& q, CpBest& best) {
    SbVisit v{q, cp_p_max(q.c), {1.0f / q.d[0], 1.0f / q.d[1], 1.0f / q.d[2]}, {}, sw_octant(q.d), 0u, best};
    group_walk(acc, n_nodes, v);
}

// ---- 6. The answer, as the eight words of an rt_box_sweep_hit: normal | t | axis | 0 | prim_id as rt_hit | the record's material
// id, unchecked.  Normal and axis are the winner's statement evaluated once more, with no limit; they are not carried through the
// walk.  Nothing accepted: normal 0, tmax as given, NONE, 0, 0xFFFFFFFF, 0.
RT_RULE void sb_answer_miss(float tmax, uint32_t out[8]) {
    out[0] = out[1] = out[2] = 0u, out[3] = cp_bits(tmax), out[4] = SB_AXIS_NONE, out[5] = 0u, out[6] = RT_PRIM_MISS, out[7] = 0u;
}
RT_RULE void sb_answer_triangle(const float rec[9], uint32_t material_id, uint64_t order, const SbQuery& q, uint32_t out[8]) {
    uint32_t axis;
    float w_in, normal[3];
    (void)sb_triangle(rec, rec + 3, rec + 6, q, INFINITY, axis, w_in);
    sb_axis_normal(rec + 3, rec + 6, axis, w_in, normal);
    out[0] = cp_bits(normal[0]), out[1] = cp_bits(normal[1]), out[2] = cp_bits(normal[2]), out[3] = (uint32_t)(order >> 32);
    out[4] = axis, out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}
RT_RULE void sb_answer_sphere(const float centre[3], float radius, uint32_t material_id, uint64_t order, const SbQuery& q, uint32_t out[8]) {
    const float t = sw_best_t(order);
    float normal[3] = {0.0f, 0.0f, 0.0f};
    if (t > 0.0f) sb_sphere_normal(centre, radius, q, t, normal);
    out[0] = cp_bits(normal[0]), out[1] = cp_bits(normal[1]), out[2] = cp_bits(normal[2]), out[3] = (uint32_t)(order >> 32);
    out[4] = t > 0.0f ? SB_AXIS_SPHERE : SB_AXIS_NONE, out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}

} // namespace rt
#endif
