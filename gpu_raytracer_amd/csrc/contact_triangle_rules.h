// contact_triangle_rules.h — the triangle contact query (rt_contact_triangle, include/rt_hip.h "Triangle contacts"), stated once.
//
// For a caller's RESTING triangle q0, q1, q2 the K nearest primitives of the scene whose distance from the triangle is below the
// margin, nearest first, each with the closest pair of points: rt_contact_capsule around a triangle instead of a segment.  Two pieces
// of code answer it: the kernel (contact_triangle.hip) and the host walk of tests/check_contact_triangle.cpp, which holds every record
// and count to a brute-force sort before any kernel runs.  Both call what is here.  Almost all of it is stated elsewhere and used as
// it is:
//   cp_triangle, cp_triangle_position, cp_sphere, cp_order, cp_start, cp_pass, cp_answer_miss     closest_point_rules.h
//   CpList, cp_list_init, cp_list_offer, cp_list_cull                                              closest_point_all_rules.h
//   sc_pair_edge, sc_clamp01, sw_cross                                                             sweep_capsule_rules.h, sweep_rules.h
//   CcQuery's bounds, cc_node_bounds, CcVisit's ANY rule, cc_offer_sphere, cc_list_count, CcMode   contact_capsule_rules.h
//   group_walk                                                                                     group_walk.h
// New are the distance of two triangles with its closest pair (rule 1), the sphere candidate (rule 2) and the record (rule 6).  The
// RT_RULE convention: host and device under hipcc, host only elsewhere; every operation is one f32 rounding and nothing is fused
// outside the node bound (the build uses -ffp-contract=off), so numpy reproduces the bits (tests/contact_triangle_cases.py).
//
// With q0 == q1 == q2 exactly, a point, the query IS rt_closest_point_all at q0 with the margin as the radius: u1 = u2 = u3 = 0 and
// nQ = 0, so rule 1's candidates b and the second half of d are absent, c and the first half of d need a query edge of squared length
// > 0, and the three candidates of a are the same value, of which only a strictly smaller one replaces the first; rule 2's near2 and
// far2 are both |q0 - o|^2 (0 - x and -x are one value, and so are their squares), so that its three cases collapse to
// fabsf(len - R) and its point is q0 + (0 * qu + 0 * qv); the node bound's interval is the point, its midpoint q0 and its p_max
// cp_p_max(q0).  dist2, the list, the counts, the walk's visits and tests, position, distance, prim_id and material_id are
// rt_closest_point_all's bit for bit, and qu = qv = 0.
//
// A segment given as v2 == v1 (or v2 == v0) is rt_contact_capsule's segment in exact arithmetic; in f32 its end B is q1 as given,
// where the capsule's is origin + axis, so the two are not bit for bit the same.  A segment given as v1 == v0 is answered as one
// given as v2 == v1 or v2 == v0: rule 2 exchanges the query's edges when the first has no length, so that cp_triangle never meets the
// collapsed edge v0 v1, on which it would divide 0 by 0.
#ifndef RT_CONTACT_TRIANGLE_RULES_H
#define RT_CONTACT_TRIANGLE_RULES_H

#include "contact_capsule_rules.h"

namespace rt {

// ---- 0. A query, from the 48 bytes of an rt_triangle_contact_query (v0 margin | v1 pad | v2 pad).  q0, q1, q2 as given; the edges
// u1 = q1 - q0, u2 = q2 - q0, u3 = u2 - u1 and the normal nQ = cross(u1, u2) are recomputed per record.  `box` carries what the node
// bound reads, in cc_node_bounds' own query type: lo, hi the exact bounds of the three vertices (a minimum and a maximum round
// nothing), mid_a = lo_a + (hi_a - lo_a) * 0.5f, p_max the largest |coordinate| of the three vertices, r the margin; its A, ax and aa
// are not read.  A DEGENERATE query lists nothing and is not walked: a non-finite vertex component, or a margin that is NaN or <= 0.
// A margin of +inf is allowed.
struct CtQuery {
    float q[3][3];
    CcQuery box;
};
RT_RULE CtQuery ct_query(const float v0[3], const float v1[3], const float v2[3], float margin) {
    CtQuery t;
    t.box.r = margin;
    t.box.p_max = 0.0f;
    t.box.aa = 0.0f;
    for (int a = 0; a < 3; a++) {
        t.q[0][a] = v0[a], t.q[1][a] = v1[a], t.q[2][a] = v2[a];
        const float lo = rule_min(rule_min(v0[a], v1[a]), v2[a]), hi = rule_max(rule_max(v0[a], v1[a]), v2[a]);
        t.box.A[a] = v0[a], t.box.ax[a] = 0.0f;
        t.box.lo[a] = lo, t.box.hi[a] = hi;
        t.box.mid[a] = lo + (hi - lo) * 0.5f;
        t.box.p_max = rule_max(t.box.p_max, rule_max(rule_max(fabsf(v0[a]), fabsf(v1[a])), fabsf(v2[a])));
    }
    return t;
}
RT_RULE bool ct_query_valid(const CtQuery& t) {
    bool ok = t.box.r > 0.0f;
    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(t.q[k][0]) && std::isfinite(t.q[k][1]) && std::isfinite(t.q[k][2]);
    return ok;
}

// ---- 1. A triangle of the scene, from its record's v0, e1, e2 (s0 = v0, s1 = v0 + e1, s2 = v0 + e2 per component; e3 = e2 - e1):
// the squared distance of the two triangles, the query's weights (qu, qv) of q1 and q2 and the scene triangle's (v, w) of v1 and v2
// at the closest pair.  The first of these candidates, in this order, with the STRICTLY smallest dist2 (cap_triangle's rule: a NaN
// dist2 is never below another, and nothing is below a first NaN, so that a degenerate scene triangle, whose candidate a is a NaN,
// is never listed, as in rt_closest_point):
//   a. q0, q1, q2 against the scene triangle:  cp_triangle(v0, e1, e2, q_k) -> dist2, v, w;  (qu, qv) = (0, 0), (1, 0), (0, 1)
//   b. only if dot(nQ, nQ) > 0: s0, s1, s2 against the query triangle:  cp_triangle(q0, u1, u2, s_k) -> dist2, qu, qv;
//      (v, w) = (0, 0), (1, 0), (0, 1)
//   c. the nine edge pairs by sc_pair_edge with the query's edge as the axis - (q0, u1), (q0, u2), (q1, u3), the outer loop - and
//      the scene's edges in cap_triangle's order, m = P - v0, P - v0, (P - v0) - e1 for the axis' origin P - the inner loop; each
//      only with both squared lengths > 0 (sc_pair_edge's own condition).  From its s and u:
//      (qu, qv) = (s, 0), (0, s), (1 - s, s);  (v, w) = (u, 0), (0, u), (1 - u, u)
//   d. piercing, dist2 = 0 (ct_pierce: cap_triangle's rule d), each only while 0 < the best so far:
//      each query edge (P, ax), in c's order, through the scene triangle: ct_pierce(P - v0, ax, e1, e2) -> s, v, w; (qu, qv) from s
//      as in c;  then, only if dot(nQ, nQ) > 0, each scene edge (v0, e1), (v0, e2), (s1, e3) through the query triangle:
//      ct_pierce(P - q0, e, u1, u2) -> s, qu, qv; (v, w) from s as c's from u
// Why these suffice: the distance of two triangles that do not intersect is attained at a pair of boundary points, or one triangle
// would cross the other's plane inside it; two closest points on segments or faces can always be moved to a vertex - face pair (a,
// b) or to an edge - edge pair (c) without growing their distance (the distance is convex along each feature).  Two triangles that
// intersect either have an edge of one passing through the other (d, both halves), or they are coplanar, where either two edges
// cross (c gives 0 for them) or a vertex of one lies in the other (a or b gives 0).  A segment or a point for the query loses b and
// d's second half, which need an area, and keeps a, c and d's first half: cap_triangle's candidates.
// ct_pierce: the segment m .. m + ax (relative to the triangle's first vertex) through the triangle with the edges a, b:
//   n = cross(a, b), nn = dot(n, n), hA = dot(n, m), hB = dot(n, m + ax) with hA < 0 && hB > 0 or hA > 0 && hB < 0;
//   s = hA / (hA - hB);  p = m + ax * s;  fv = dot(cross(p, b), n) / nn, fw = dot(cross(a, p), n) / nn
//   accepted iff dot(ax, ax) > 0 && fv >= 0 && fw >= 0 && fv + fw <= 1
RT_RULE bool ct_pierce(const float m[3], const float ax[3], const float a[3], const float b[3], float& s, float& fv, float& fw) {
    float n[3], x[3], y[3];
    sw_cross(a, b, n);
    const float mb[3] = {m[0] + ax[0], m[1] + ax[1], m[2] + ax[2]};
    const float nn = cp_dot(n, n), hA = cp_dot(n, m), hB = cp_dot(n, mb);
    s = hA / (hA - hB);
    const float p[3] = {m[0] + ax[0] * s, m[1] + ax[1] * s, m[2] + ax[2] * s};
    sw_cross(p, b, x);
    sw_cross(a, p, y);
    fv = cp_dot(x, n) / nn, fw = cp_dot(y, n) / nn;
    const bool across = (hA < 0.0f && hB > 0.0f) || (hA > 0.0f && hB < 0.0f);
    return cp_dot(ax, ax) > 0.0f && across && fv >= 0.0f && fw >= 0.0f && fv + fw <= 1.0f;
}
// the weights of a triangle's second and third vertex at the place t of its edge number `edge` (0: first - second, 1: first -
// third, 2: second - third)
RT_RULE void ct_edge_weights(int edge, float t, float& a, float& b) {
    a = edge == 0 ? t : edge == 1 ? 0.0f : 1.0f - t;
    b = edge == 0 ? 0.0f : t;
}
RT_RULE float ct_triangle(const float v0[3], const float e1[3], const float e2[3], const CtQuery& t, float& qu, float& qv, float& v, float& w) {
    const float* q0 = t.q[0];
    float u1[3], u2[3], u3[3], e3[3], nQ[3];
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) u1[a] = t.q[1][a] - q0[a], u2[a] = t.q[2][a] - q0[a], e3[a] = e2[a] - e1[a];
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) u3[a] = u2[a] - u1[a];
    sw_cross(u1, u2, nQ);
    const bool area = cp_dot(nQ, nQ) > 0.0f;
    float best = cp_triangle(v0, e1, e2, q0, v, w); // a.
    qu = 0.0f, qv = 0.0f;
    RT_CP_UNROLL
    for (int k = 1; k < 3; k++) {
        float cv, cw;
        const float d2 = cp_triangle(v0, e1, e2, t.q[k], cv, cw);
        if (d2 < best) best = d2, qu = k == 1 ? 1.0f : 0.0f, qv = k == 2 ? 1.0f : 0.0f, v = cv, w = cw;
    }
    if (area) { // b.
        RT_CP_UNROLL
        for (int k = 0; k < 3; k++) {
            const float s[3] = {k == 0 ? v0[0] : v0[0] + (k == 1 ? e1 : e2)[0], k == 0 ? v0[1] : v0[1] + (k == 1 ? e1 : e2)[1],
                                k == 0 ? v0[2] : v0[2] + (k == 1 ? e1 : e2)[2]};
            float cu, cv;
            const float d2 = cp_triangle(q0, u1, u2, s, cu, cv);
            if (d2 < best) best = d2, qu = cu, qv = cv, v = k == 1 ? 1.0f : 0.0f, w = k == 2 ? 1.0f : 0.0f;
        }
    }
    RT_CP_UNROLL
    for (int i = 0; i < 3; i++) { // c.
        const float* P = i == 2 ? t.q[1] : q0;
        const float* ax = i == 0 ? u1 : i == 1 ? u2 : u3;
        const float ap[3] = {P[0] - v0[0], P[1] - v0[1], P[2] - v0[2]};
        const float m1[3] = {ap[0] - e1[0], ap[1] - e1[1], ap[2] - e1[2]};
        const float aa = cp_dot(ax, ax);
        RT_CP_UNROLL
        for (int j = 0; j < 3; j++) {
            float d2, cs, cu;
            sc_pair_edge(j == 2 ? m1 : ap, j == 0 ? e1 : j == 1 ? e2 : e3, ax, aa, d2, cs, cu);
            if (d2 < best) {
                best = d2;
                ct_edge_weights(i, cs, qu, qv);
                ct_edge_weights(j, cu, v, w);
            }
        }
    }
    RT_CP_UNROLL
    for (int i = 0; i < 3; i++) { // d, the query's edges through the scene triangle
        const float* P = i == 2 ? t.q[1] : q0;
        const float ap[3] = {P[0] - v0[0], P[1] - v0[1], P[2] - v0[2]};
        float ps, fv, fw;
        if (ct_pierce(ap, i == 0 ? u1 : i == 1 ? u2 : u3, e1, e2, ps, fv, fw) && 0.0f < best) {
            best = 0.0f, v = fv, w = fw;
            ct_edge_weights(i, ps, qu, qv);
        }
    }
    if (area) {
        RT_CP_UNROLL
        for (int j = 0; j < 3; j++) { // d, the scene's edges through the query triangle
            const float a0[3] = {v0[0] - q0[0], v0[1] - q0[1], v0[2] - q0[2]};
            const float a1[3] = {(v0[0] + e1[0]) - q0[0], (v0[1] + e1[1]) - q0[1], (v0[2] + e1[2]) - q0[2]};
            float ps, fu, fv;
            if (ct_pierce(j == 2 ? a1 : a0, j == 0 ? e1 : j == 1 ? e2 : e3, u1, u2, ps, fu, fv) && 0.0f < best) {
                best = 0.0f, qu = fu, qv = fv;
                ct_edge_weights(j, ps, v, w);
            }
        }
    }
    return best;
}

// ---- 2. A sphere is its surface (centre o, radius R), as everywhere.  near2, (qu, qv) = cp_triangle(q0, u1, u2, o) - or, if not
// dot(u1, u1) > 0, near2, (qv, qu) = cp_triangle(q0, u2, u1, o), the edges exchanged, which for a point changes nothing - : the query's
// point nearest the centre; far2 = max_k dot(q_k - o, q_k - o), the lowest k on a tie: its farthest, a vertex.  dn = sqrtf(near2),
// df = sqrtf(far2).  The first of these that holds gives the distance d of the surface from the triangle and the query's point:
//   OUTSIDE        dn > R:              d = dn - R at the nearest point
//   WHOLLY INSIDE  df < R:              d = R - df at the farthest vertex, (qu, qv) = (0, 0), (1, 0) or (0, 1)
//   CROSSING       dn <= R && R <= df:  d = 0 at the point of the segment from the nearest point Pn = q0 + (u1 qu + u2 qv) to the
//        farthest vertex Pf whose distance from o is R, cc_sphere's crossing root with that segment as the axis:
//        ax = Pf - Pn; aa = dot(ax, ax); mA = Pn - o; b = dot(mA, ax); c = dot(mA, mA) - R * R; disc = b * b - aa * c
//        q = disc > 0 ? sqrtf(disc) : 0;  s = aa > 0 ? clamp((q - b) / aa) : 0       (Pn is inside or on the surface: the upper root)
//        qu = qu_n + (qu_f - qu_n) * s, qv likewise
//   none (a NaN in the centre or the radius):  d = NaN
// dist2 = d * d.  The point of the sphere is cp_sphere's from the query's point p = q0 + (u1 qu + u2 qv) (ct_sphere_position).
RT_RULE float ct_sphere(const float centre[3], float radius, const CtQuery& t, float& qu, float& qv) {
    const float* q0 = t.q[0];
    float u1[3], u2[3];
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) u1[a] = t.q[1][a] - q0[a], u2[a] = t.q[2][a] - q0[a];
    const bool exchanged = !(cp_dot(u1, u1) > 0.0f);
    const float near2 = exchanged ? cp_triangle(q0, u2, u1, centre, qv, qu) : cp_triangle(q0, u1, u2, centre, qu, qv);
    float far2 = 0.0f, fu = 0.0f, fv = 0.0f;
    RT_CP_UNROLL
    for (int k = 0; k < 3; k++) {
        const float m[3] = {t.q[k][0] - centre[0], t.q[k][1] - centre[1], t.q[k][2] - centre[2]};
        const float d2 = cp_dot(m, m);
        if (k == 0 || d2 > far2) far2 = d2, fu = k == 1 ? 1.0f : 0.0f, fv = k == 2 ? 1.0f : 0.0f;
    }
    const float dn = sqrtf(near2), df = sqrtf(far2);
    float d = NAN;
    if (dn > radius) d = dn - radius;
    else if (df < radius) d = radius - df, qu = fu, qv = fv;
    else if (dn <= radius && radius <= df) {
        float pn[3], ax[3], mA[3];
        cp_triangle_position(q0, u1, u2, qu, qv, pn);
        RT_CP_UNROLL
        for (int a = 0; a < 3; a++) ax[a] = (fu != 0.0f ? t.q[1][a] : fv != 0.0f ? t.q[2][a] : q0[a]) - pn[a], mA[a] = pn[a] - centre[a];
        const float aa = cp_dot(ax, ax), b = cp_dot(mA, ax), c = cp_dot(mA, mA) - radius * radius, disc = b * b - aa * c;
        const float sq = disc > 0.0f ? sqrtf(disc) : 0.0f;
        const float s = aa > 0.0f ? sc_clamp01((sq - b) / aa) : 0.0f;
        d = 0.0f;
        qu = qu + (fu - qu) * s, qv = qv + (fv - qv) * s;
    }
    return d * d;
}
RT_RULE void ct_sphere_position(const float centre[3], float radius, const CtQuery& t, float qu, float qv, float pos[3]) {
    const float* q0 = t.q[0];
    float u1[3], u2[3], p[3];
    for (int a = 0; a < 3; a++) u1[a] = t.q[1][a] - q0[a], u2[a] = t.q[2][a] - q0[a];
    cp_triangle_position(q0, u1, u2, qu, qv, p);
    (void)cp_sphere(centre, radius, p, pos);
}

// ---- 3. Order, range and list: rt_contact_capsule's (contact_capsule_rules.h rule 3) with the margin where the radius is: a
// candidate is cp_order(dist2, key) and is IN RANGE iff it is below cp_start(margin).

// ---- 4. The lower bound of a node's eight child boxes: cc_node_bounds on t.box, as it is.  The distance between the box of the
// query's vertices and a child box is a lower bound of the distance between the triangle and anything in the child box; lo and hi
// are exact here, so that only the planes' and the records' roundings remain for RT_CP_SLACK to cover (DESIGN.md section 4,
// "Triangle contacts").  The bound is loose for a large triangle askew to the axes, whose box is mostly empty.

// ---- 5. The walk: CcVisit's, with this query's candidate.  In ANY mode the list has cap 0 and the walk ends at the first
// candidate in range.  Spheres are offered by cc_offer_sphere and the count is cc_list_count, unchanged.
template <bool COUNT_ALL, bool ANY>
struct CtVisit {
    const CtQuery& t;
    float L[8];
    CpList& list;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        uint32_t code;
        cc_node_bounds(w, t.box, L, code);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return cp_pass(L, cp_list_cull<COUNT_ALL>(list), occupied); }
    template <class Access>
    RT_RULE bool leaf(Access& acc, uint32_t slot, const float rec[9], const uint32_t ids[3]) {
        float qu, qv, v, wgt;
        const uint64_t c = cp_order(ct_triangle(rec, rec + 3, rec + 6, t, qu, qv, v, wgt), ids[1] ^ RT_PRIM_SPHERE_FLAG);
        if (ANY) {
            if (!(c < list.start)) return false;
            list.total++;
            return true;
        }
        cp_list_offer<COUNT_ALL>(acc, list, c, slot);
        return false;
    }
};
template <int MODE, class Access>
RT_RULE void ct_walk(Access& acc, uint32_t n_nodes, const CtQuery& t, CpList& list) {
    CtVisit<MODE == CC_COUNT_ALL, MODE == CC_ANY> v{t, {}, list};
    group_walk(acc, n_nodes, v);
}

// ---- 6. The answer, as the eight words of an rt_triangle_contact: position | distance = sqrtf(dist2) | qu | qv | prim_id as rt_hit
// | the record's material id, unchecked - rt_nearest's layout with the QUERY's weights where the primitive's are.  A listed entry's
// statement is evaluated once more for qu, qv, v, w and the point: position = v0 + (e1 v + e2 w), or ct_sphere_position.  An unused
// slot is cp_answer_miss(margin).
RT_RULE void ct_answer_triangle(const float rec[9], uint32_t material_id, uint64_t order, const CtQuery& t, uint32_t out[8]) {
    float qu, qv, v, w, pos[3];
    (void)ct_triangle(rec, rec + 3, rec + 6, t, qu, qv, v, w);
    cp_triangle_position(rec, rec + 3, rec + 6, v, w, pos);
    out[0] = cp_bits(pos[0]), out[1] = cp_bits(pos[1]), out[2] = cp_bits(pos[2]), out[3] = cp_bits(sqrtf(cp_best_dist2(order)));
    out[4] = cp_bits(qu), out[5] = cp_bits(qv), out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}
RT_RULE void ct_answer_sphere(const float centre[3], float radius, uint32_t material_id, uint64_t order, const CtQuery& t, uint32_t out[8]) {
    float qu, qv, pos[3];
    (void)ct_sphere(centre, radius, t, qu, qv);
    ct_sphere_position(centre, radius, t, qu, qv, pos);
    out[0] = cp_bits(pos[0]), out[1] = cp_bits(pos[1]), out[2] = cp_bits(pos[2]), out[3] = cp_bits(sqrtf(cp_best_dist2(order)));
    out[4] = cp_bits(qu), out[5] = cp_bits(qv), out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}

} // namespace rt
#endif
