// sweep_rules.h — the sphere sweep (rt_sweep_sphere, include/rt_hip.h "Sphere sweeps"), stated once.
//
// Two pieces of code answer it: the kernel (sweep.hip) and the host walk of tests/check_sweep.cpp, which holds the whole walk to a
// brute force before any kernel runs.  Both call what is here: the time of first contact with a triangle and with a sphere, the order
// among candidates, the lower bound of a node's eight child boxes widened by the radius, and the visitor that group_walk
// (group_walk.h) runs.  It builds on closest_point_rules.h: the overlap at the start and the reported point are the closest-point statement
// (cp_triangle, cp_sphere), the order is cp_order.  Every operation is one f32 rounding (the build uses -ffp-contract=off; the only
// fused operations are written fmaf, and they are in the box bound, not in the answer), so numpy reproduces the bits
// (tests/sweep_cases.py).
#ifndef RT_SWEEP_RULES_H
#define RT_SWEEP_RULES_H

#include "closest_point_rules.h"

namespace rt {

// The margin of the box bound: relative to the magnitudes that enter it in space, and relative to the entry time (sw_node_bounds).
#ifndef RT_SW_SLACK
#define RT_SW_SLACK 1.0e-5f
#endif

// (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x): two products and one difference per component
RT_RULE void sw_cross(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// One query: the centre c at t = 0, the direction d, the radius r and what every piece needs of them.
struct SwQuery {
    float c[3], d[3], r, rr, dd, tmax;
};
RT_RULE SwQuery sw_query(const float origin[3], float radius, const float direction[3], float tmax) {
    SwQuery q;
    for (int a = 0; a < 3; a++) q.c[a] = origin[a], q.d[a] = direction[a];
    q.r = radius, q.rr = radius * radius, q.dd = cp_dot(direction, direction), q.tmax = tmax;
    return q;
}
// a query that is a miss without a walk: a non-finite origin or direction component, a zero direction, a radius that is NaN, <= 0 or
// infinite, a tmax that is NaN or <= 0
RT_RULE bool sw_query_valid(const SwQuery& q) {
    bool finite = true, moving = false;
    for (int a = 0; a < 3; a++) finite = finite && std::isfinite(q.c[a]) && std::isfinite(q.d[a]), moving = moving || q.d[a] != 0.0f;
    return finite && moving && q.r > 0.0f && q.r < INFINITY && q.tmax > 0.0f;
}

// ---- 1. A triangle, from its record's v0, e1, e2: the time of the first contact of the moving sphere with it, +inf when there is
// none.  The triangle's Minkowski sum with the ball is its two faces pushed out by r, a ball at each vertex and a cylinder round each
// edge; the first entry into their union is the minimum over the pieces that accept.  The cylinder's caps and the prism's sides lie
// inside the vertex balls and the cylinders, so these pieces give the exact first contact.  A NaN never accepts.
// The ball and the cylinder are solved in the cross-product form: disc = dd*rr - |m x d|^2 for b*b - dd*(mm - rr), and for the
// cylinder A = |e x d|^2, B = m . ((e x d) x e), disc / ee = rr*A - (m . (e x d))^2.  The expanded forms cancel two terms of the size
// |m|^2 to get at r^2, an error that grows as |m|^2 / r with the distance |m| of the start; these lose 2^-23 |m|.
RT_RULE void sw_take(float& best, bool accepts, float t) {
    if (accepts && t < best) best = t;
}
RT_RULE void sw_vertex(const float m[3], const SwQuery& q, float& best) {
    float x[3];
    const float b = cp_dot(m, q.d);
    sw_cross(m, q.d, x);
    const float disc = q.dd * q.rr - cp_dot(x, x);
    const float t = (-b - sqrtf(disc)) / q.dd;
    sw_take(best, disc >= 0.0f && t >= 0.0f, t);
}
RT_RULE void sw_edge(const float m[3], const float e[3], const SwQuery& q, float& best) {
    float ned[3], p[3];
    sw_cross(e, q.d, ned);
    sw_cross(ned, e, p);
    const float A = cp_dot(ned, ned), B = cp_dot(m, p), h = cp_dot(m, ned), ee = cp_dot(e, e);
    const float disc = q.rr * A - h * h;
    const float t = (-B - sqrtf(ee * disc)) / A;
    const float sp = (cp_dot(m, e) + t * cp_dot(q.d, e)) / ee;
    sw_take(best, A > 0.0f && disc >= 0.0f && t >= 0.0f && 0.0f <= sp && sp <= 1.0f, t);
}
RT_RULE float sw_triangle(const float v0[3], const float e1[3], const float e2[3], const SwQuery& q) {
    float v, w;
    if (cp_triangle(v0, e1, e2, q.c, v, w) <= q.rr) return 0.0f; // overlap at the start; every other piece gives t >= 0
    float best = INFINITY;
    const float ap[3] = {q.c[0] - v0[0], q.c[1] - v0[1], q.c[2] - v0[2]};
    { // the face on the side the centre starts on
        float n[3], x[3], y[3];
        sw_cross(e1, e2, n);
        const float nn = cp_dot(n, n), ln = sqrtf(nn), h = cp_dot(n, ap), nd = cp_dot(n, q.d);
        const float s = h < 0.0f ? -1.0f : 1.0f;
        const float num = fabsf(h) - q.r * ln, den = -(s * nd), t = num / den;
        if (num >= 0.0f && den > 0.0f) {
            const float k = s * q.r / ln;
            const float p[3] = {(ap[0] + q.d[0] * t) - n[0] * k, (ap[1] + q.d[1] * t) - n[1] * k, (ap[2] + q.d[2] * t) - n[2] * k};
            sw_cross(p, e2, x);
            sw_cross(e1, p, y);
            const float fv = cp_dot(x, n) / nn, fw = cp_dot(y, n) / nn;
            sw_take(best, fv >= 0.0f && fw >= 0.0f && fv + fw <= 1.0f, t);
        }
    }
    const float m1[3] = {ap[0] - e1[0], ap[1] - e1[1], ap[2] - e1[2]}, m2[3] = {ap[0] - e2[0], ap[1] - e2[1], ap[2] - e2[2]};
    const float e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    sw_vertex(ap, q, best);
    sw_vertex(m1, q, best);
    sw_vertex(m2, q, best);
    sw_edge(ap, e1, q, best);
    sw_edge(ap, e2, q, best);
    sw_edge(m1, e3, q, best);
    return best + 0.0f; // a -0 (a tangent start) counts as +0, so that bit order stays value order
}

// ---- 2. A sphere (its surface, as cp_sphere): in contact at the start, or from outside the entering root against R + r, or from
// inside the leaving root against R - r.
RT_RULE float sw_sphere(const float centre[3], float radius, const SwQuery& q) {
    const float m[3] = {q.c[0] - centre[0], q.c[1] - centre[1], q.c[2] - centre[2]};
    const float len = sqrtf(cp_dot(m, m)), b = cp_dot(m, q.d);
    if (fabsf(len - radius) <= q.r) return 0.0f;
    float x[3], best = INFINITY;
    sw_cross(m, q.d, x);
    const float xx = cp_dot(x, x);
    if (len > radius) {
        const float rs = radius + q.r, disc = q.dd * (rs * rs) - xx, t = (-b - sqrtf(disc)) / q.dd;
        sw_take(best, disc >= 0.0f && t >= 0.0f, t);
    } else {
        const float rs = radius - q.r, disc = q.dd * (rs * rs) - xx, t = (-b + sqrtf(disc)) / q.dd;
        sw_take(best, disc >= 0.0f && t >= 0.0f, t);
    }
    return best + 0.0f;
}

// ---- 3. Order and acceptance: cp_order on the bits of t.  t >= +0 or +inf for everything the pieces return, so bit order is value
// order.  The best starts at (bits of tmax, 0) and a candidate replaces it iff it is below it: only t < tmax is ever accepted,
// strictly; +inf (no contact) never is; equal t: the lower key, spheres before triangles, each by index.  Among several primitives in
// contact at the start (all t = 0) that is the lowest key, not the nearest.
RT_RULE uint64_t sw_start(float tmax) { return cp_order(tmax, 0u); }
RT_RULE float sw_best_t(uint64_t best) { return cp_float((uint32_t)(best >> 32)); }

// ---- 4. The lower bound of a node's eight child boxes.  At the time of contact the centre lies within r of the primitive (up to the
// statement's rounding), hence on every axis inside the child slot's decoded box widened by wd = r + s, so the ray's entry time into
// the widened box bounds every candidate of the slot from below.  w[20]: the DevNode8 as 32-bit words; inv_a = 1 / d_a (+-inf for a
// zero component: the axis then only says inside or outside); code: the direction's sign bits, the ray's octant.
//   s = RT_SW_SLACK * (max_a |c_a| + max_a (|org_a| + 255 * scale_a) + r)
//   near and far plane by the sign of d_a, pushed out by wd;  tn_a = (near_a - c_a) * inv_a,  tx_a = (far_a - c_a) * inv_a
//   tn = max(tn_x, tn_y, tn_z, 0) * (1 - RT_SW_SLACK);  tx = min(tx_x, tx_y, tx_z) * (1 + RT_SW_SLACK)
// The slot is dead when tx < tn (the ray passes the widened box, or the box lies behind), else its bound is L = tn.  sw_pass culls a
// slot iff it is dead or L > best t, strictly: a tie with a lower key must still be found.  The planes are evaluated as
// fmaf(q, scale, (org_a - c_a) -+ wd): not the decoded plane's bits, but within one rounding of the magnitudes in s of them; the bound
// is no part of the answer.  Why s suffices: DESIGN.md section 4.  A NaN (0 * inf on a plane the centre lies in, an overflowing grid)
// is dropped by max / min on the device and compares false on the host: the slot is followed either way.
RT_RULE void sw_node_bounds(const uint32_t w[20], const SwQuery& q, const float inv[3], uint32_t code, float c_max, float L[8], uint32_t& alive) {
    float scale[3], on[3], of[3], m = 0.0f;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        scale[a] = ldexpf(1.0f, (int)(int8_t)((w[3] >> (8 * a)) & 0xFFu));
        m = rule_max(m, fmaf(255.0f, scale[a], fabsf(cp_float(w[a]))));
    }
    const float wd = q.r + RT_SW_SLACK * ((c_max + m) + q.r);
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        const float oc = cp_float(w[a]) - q.c[a];
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
        L[sl] = tn * (1.0f - RT_SW_SLACK);
        if (!(tx * (1.0f + RT_SW_SLACK) < L[sl])) alive |= 1u << sl;
    }
}
// the slots of `occupied` that are alive and that a best time of best_t leaves to visit
RT_RULE uint32_t sw_pass(const float L[8], float best_t, uint32_t occupied) {
    uint32_t pass = 0u;
    RT_CP_UNROLL
    for (int sl = 0; sl < 8; sl++)
        if (!(L[sl] > best_t)) pass |= 1u << sl;
    return pass & occupied;
}
RT_RULE uint32_t sw_octant(const float d[3]) { return (cp_bits(d[0]) >> 31) | ((cp_bits(d[1]) >> 31) << 1) | ((cp_bits(d[2]) >> 31) << 2); }

// ---- 5. The walk: group_walk (group_walk.h) visited by the best time so far, with the ray's octant for every node's code: nearest
// first along the ray.
struct SwVisit {
    const SwQuery& q;
    float c_max, inv[3], L[8];
    uint32_t code, alive;
    CpBest& best;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        sw_node_bounds(w, q, inv, code, c_max, L, alive);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return sw_pass(L, sw_best_t(best.order), occupied & alive); }
    template <class Access>
    RT_RULE bool leaf(Access&, uint32_t slot, const float rec[9], const uint32_t ids[3]) {
        const uint64_t c = cp_order(sw_triangle(rec, rec + 3, rec + 6, q), ids[1] ^ RT_PRIM_SPHERE_FLAG);
        if (c < best.order) best.order = c, best.slot = slot;
        return false;
    }
};
template <class Access>
RT_RULE void sw_walk(Access& acc, uint32_t n_nodes, const SwQuery& q, CpBest& best) {
    SwVisit v{q, cp_p_max(q.c), {1.0f / q.d[0], 1.0f / q.d[1], 1.0f / q.d[2]}, {}, sw_octant(q.d), 0u, best};
    group_walk(acc, n_nodes, v);
}

// ---- 6. The answer, as the eight words of an rt_sweep_hit: position | t | u, v | prim_id as rt_hit | the record's material id,
// unchecked.  position, u, v are the closest-point statement of the winner at centre = c + d*t (per component c_a + d_a*t): at t = 0
// exactly what rt_closest_point gives for that primitive from the origin.  Nothing accepted: position 0, tmax as given, u = v = 0,
// prim_id 0xFFFFFFFF, material 0.
RT_RULE void sw_answer_miss(float tmax, uint32_t out[8]) { cp_answer_miss(tmax, out); }
RT_RULE void sw_centre(const SwQuery& q, float t, float centre[3]) {
    for (int a = 0; a < 3; a++) centre[a] = q.c[a] + q.d[a] * t;
}
RT_RULE void sw_answer_triangle(const float rec[9], uint32_t material_id, uint64_t order, const SwQuery& q, uint32_t out[8]) {
    float centre[3];
    sw_centre(q, sw_best_t(order), centre);
    cp_answer_triangle(rec, material_id, order, centre, out);
    out[3] = (uint32_t)(order >> 32);
}
RT_RULE void sw_answer_sphere(const float centre_s[3], float radius, uint32_t material_id, uint64_t order, const SwQuery& q, uint32_t out[8]) {
    float centre[3];
    sw_centre(q, sw_best_t(order), centre);
    cp_answer_sphere(centre_s, radius, material_id, order, centre, out);
    out[3] = (uint32_t)(order >> 32);
}

} // namespace rt
#endif
