// overlap_triangle_rules.h — the triangle query (rt_overlap_triangle, include/rt_hip.h "Triangle queries"), stated once.
//
// Two pieces of code answer it: the kernel (overlap_triangle.hip) and the host walk of tests/check_overlap_triangle.cpp, which holds
// the whole walk to a brute force over all primitives before any kernel runs.  Both call what is here: when a triangle and when a
// sphere of the scene TOUCHES a caller's triangle, and the visitor that group_walk (group_walk.h) runs.  The list, the node test and
// the modes are overlap_rules.h's and are not restated.  The RT_RULE convention of group_walk.h: every operation is one f32 rounding
// and nothing is fused (the build uses -ffp-contract=off), so numpy reproduces the bits (tests/overlap_triangle_cases.py).  dot is
// cp_dot; cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x).  Every test is stated in its POSITIVE form, so
// that a NaN makes it false; a primitive touches iff ALL its tests hold, in whatever order they are evaluated.
//
// ---- 1. A query.  Vertices q0, q1, q2;  u1 = q1 - q0,  u2 = q2 - q0,  u3 = u2 - u1;  qlo, qhi the per-axis min and max of the three
// vertices (exact).  A query with a non-finite component touches nothing and is not walked.  A finite degenerate query - a segment, a
// point - is allowed.
// ---- 2. A triangle of the scene, from its record's v0, e1, e2:  s0 = v0, s1 = v0 + e1, s2 = v0 + e2;  f1 = e1, f2 = e2,
// f3 = e2 - e1.  It touches iff
//   0. all nine components of the s_k are finite;
//   1. per coordinate axis a:  min_k s_k[a] <= qhi[a] && max_k s_k[a] >= qlo[a]   (most records a walk reaches fail here, and the
//      cull of the walk rests on it: DESIGN.md section 4, "Triangle queries");
//   2. with a_k = s_k - q0, for each of the 23 axes L below (ot_span):
//        pS_k = dot(L, a_k),  pQ = (0, dot(L, u1), dot(L, u2))
//        min_k pS_k <= max pQ && max_k pS_k >= min pQ, and ((pS_0 + pS_1) + pS_2) + (pQ_1 + pQ_2) is not a NaN
//      (the min and max ignore a NaN operand, as ov_span notes; the sum is what fails one).
// The axes:  nS = cross(f1, f2) and nQ = cross(u1, u2);  the nine cross(u_i, f_j);  cross(nQ, u_i) and cross(nS, f_j), which decide
// coplanar pairs;  cross(nS, u_i) and cross(nQ, f_j), which decide a pair in which one triangle is a segment.  Any vector is a
// legitimate candidate for a separating axis, so a noisy axis from nearly parallel edges can never wrongly separate in exact
// arithmetic: only the rounding of the projections matters.
// Two limits:
//   - Two DEGENERATE triangles (each a segment or a point) can be listed although they are disjoint: both normals vanish, and for
//     two parallel segments or two points every axis is the zero vector, which separates nothing, so test 1 alone decides.  This
//     errs on the side of listing.
//   - "Closed" means closed on the RECORD: the scene's vertices are s_k as computed above, one rounding from the uploaded ones.  A
//     vertex the caller shares with the scene is bit-equal only where v0 + e reproduces it.
// ---- 3. A sphere (o, R), a surface as everywhere:  near2 = cp_triangle(q0, u1, u2, o),  far2 = max_k dot(q_k - o, q_k - o) over
// the query's three vertices as given,  rr = R * R.  It touches iff near2 <= rr && far2 >= rr: a triangle wholly inside the ball is
// not touched.  A NaN centre or radius makes near2 or rr a NaN and fails.
// ---- 4. The walk: ov_node_reach (overlap_rules.h) on the OvBox of the query's bounds (ov_box_init_bounds), the list and the
// modes as for rt_overlap_box.
#ifndef RT_OVERLAP_TRIANGLE_RULES_H
#define RT_OVERLAP_TRIANGLE_RULES_H

#include "overlap_rules.h"

namespace rt {

RT_RULE void ot_cross(const float a[3], const float b[3], float out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1], out[1] = a[2] * b[0] - a[0] * b[2], out[2] = a[0] * b[1] - a[1] * b[0];
}

// rule 1.  q1 and q2 are kept for the spheres' far2 alone; the walk reads q0, u1, u2 and the bounds.
struct OtQuery {
    float q0[3], q1[3], q2[3], u1[3], u2[3];
    OvBox box; // lo = qlo, hi = qhi
};
RT_RULE bool ot_query_valid(const float q0[3], const float q1[3], const float q2[3]) {
    bool ok = true;
    for (int a = 0; a < 3; a++) ok = ok && ov_finite(q0[a]) && ov_finite(q1[a]) && ov_finite(q2[a]);
    return ok;
}
RT_RULE void ot_query_init(OtQuery& q, const float q0[3], const float q1[3], const float q2[3]) {
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        q.q0[a] = q0[a], q.q1[a] = q1[a], q.q2[a] = q2[a];
        q.u1[a] = q1[a] - q0[a], q.u2[a] = q2[a] - q0[a];
        lo[a] = ov_min(ov_min(q0[a], q1[a]), q2[a]), hi[a] = ov_max(ov_max(q0[a], q1[a]), q2[a]);
    }
    ov_box_init_bounds(q.box, lo, hi);
}

// rule 2, test 2 on one axis
RT_RULE bool ot_span(float s0, float s1, float s2, float t1, float t2) {
    const float sum = ((s0 + s1) + s2) + (t1 + t2);
    return ov_min(ov_min(s0, s1), s2) <= ov_max(ov_max(0.0f, t1), t2) && ov_max(ov_max(s0, s1), s2) >= ov_min(ov_min(0.0f, t1), t2) && sum == sum;
}
struct OtPair { // what every axis of a pair is projected on
    float a0[3], a1[3], a2[3];
    const float *u1, *u2;
};
RT_RULE bool ot_axis(const OtPair& p, const float L[3]) {
    return ot_span(cp_dot(L, p.a0), cp_dot(L, p.a1), cp_dot(L, p.a2), cp_dot(L, p.u1), cp_dot(L, p.u2));
}
RT_RULE bool ot_axis_cross(const OtPair& p, const float a[3], const float b[3]) {
    float L[3];
    ot_cross(a, b, L);
    return ot_axis(p, L);
}
// the three axes cross(n, g_j)
RT_RULE bool ot_axes_with(const OtPair& p, const float n[3], const float g1[3], const float g2[3], const float g3[3]) {
    return ot_axis_cross(p, n, g1) && ot_axis_cross(p, n, g2) && ot_axis_cross(p, n, g3);
}

RT_RULE bool ot_triangle(const float v0[3], const float e1[3], const float e2[3], const OtQuery& q) {
    OtPair p;
    bool ok = true;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        const float s0 = v0[a], s1 = v0[a] + e1[a], s2 = v0[a] + e2[a];
        ok = ok && ov_finite(s0) && ov_finite(s1) && ov_finite(s2);
        ok = ok && ov_min(ov_min(s0, s1), s2) <= q.box.hi[a] && ov_max(ov_max(s0, s1), s2) >= q.box.lo[a];
        p.a0[a] = s0 - q.q0[a], p.a1[a] = s1 - q.q0[a], p.a2[a] = s2 - q.q0[a];
    }
    if (!ok) return false; // most records a walk reaches end here
    p.u1 = q.u1, p.u2 = q.u2;
    float nS[3], nQ[3];
    ot_cross(e1, e2, nS);
    if (!ot_axis(p, nS)) return false;
    ot_cross(q.u1, q.u2, nQ);
    if (!ot_axis(p, nQ)) return false;
    const float f3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    const float u3[3] = {q.u2[0] - q.u1[0], q.u2[1] - q.u1[1], q.u2[2] - q.u1[2]};
    return ot_axes_with(p, q.u1, e1, e2, f3) && ot_axes_with(p, q.u2, e1, e2, f3) && ot_axes_with(p, u3, e1, e2, f3) && // cross(u_i, f_j)
           ot_axes_with(p, nQ, q.u1, q.u2, u3) && ot_axes_with(p, nS, e1, e2, f3) &&                                    // coplanar pairs
           ot_axes_with(p, nS, q.u1, q.u2, u3) && ot_axes_with(p, nQ, e1, e2, f3);                                      // one is a segment
}

// rule 3
RT_RULE bool ot_sphere(const float centre[3], float radius, const OtQuery& q) {
    float v, w, d0[3], d1[3], d2[3];
    const float near2 = cp_triangle(q.q0, q.u1, q.u2, centre, v, w);
    for (int a = 0; a < 3; a++) d0[a] = q.q0[a] - centre[a], d1[a] = q.q1[a] - centre[a], d2[a] = q.q2[a] - centre[a];
    const float far2 = ov_max(ov_max(cp_dot(d0, d0), cp_dot(d1, d1)), cp_dot(d2, d2));
    const float rr = radius * radius;
    return near2 <= rr && far2 >= rr;
}

// rule 4: OvVisit with this file's leaf test
template <int MODE>
struct OtVisit {
    const OtQuery& q;
    OvList& list;
    uint32_t reach;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        uint32_t code;
        reach = ov_node_reach(w, q.box, code);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return reach & occupied; }
    template <class Access>
    RT_RULE bool leaf(Access& acc, uint32_t, const float rec[9], const uint32_t ids[3]) {
        const uint32_t key = ids[1] ^ RT_PRIM_SPHERE_FLAG;
        if (!(ov_list_wants<MODE>(list, key) && ot_triangle(rec, rec + 3, rec + 6, q))) return false;
        ov_list_offer(acc, list, key);
        return MODE == OV_ANY;
    }
};
template <int MODE, class Access>
RT_RULE void ot_walk(Access& acc, uint32_t n_nodes, const OtQuery& q, OvList& list) {
    OtVisit<MODE> v{q, list, 0u};
    group_walk(acc, n_nodes, v);
}

} // namespace rt
#endif
