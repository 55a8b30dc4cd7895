// obb_rules.h — the oriented-box queries (rt_overlap_obb, rt_sweep_obb, include/rt_hip.h "Oriented boxes"), stated once.
//
// Two pieces of code answer each: the kernels (overlap_obb.hip, sweep_obb.hip) and the host walk of tests/check_obb.cpp, which holds
// the whole walk to a brute force over all primitives before any kernel runs.  Both call what is here: the box's frame from its
// quaternion, the triangle and the sphere taken into that frame, the world bounding box the walk culls by, and the visitors that
// group_walk (group_walk.h) runs.  What happens IN the frame is not restated: it is overlap_rules.h (ov_triangle_rel, ov_sphere, the
// list) and sweep_box_rules.h (sb_triangle_rel, sb_axis_normal, sb_sphere, sb_sphere_normal, the order, the node bound), applied to
// (a'_0, a'_1, a'_2, e1', e2', h[, d']).  Every operation is one f32 rounding and nothing is fused (the build uses -ffp-contract=off;
// the only fused operations are the fmaf of the node bounds), so numpy reproduces the bits (tests/obb_cases.py).
//
// ---- 1. The frame.  q = rotation = (x, y, z, w), the quaternion that turns the box's own axes into world axes, not necessarily of
// unit length:
//   n = ((x*x + y*y) + z*z) + w*w;  s = 2.0f / n
//   xs = x*s, ys = y*s, zs = z*s;   wx = w*xs, wy = w*ys, wz = w*zs
//   xx = x*xs, xy = x*ys, xz = x*zs, yy = y*ys, yz = y*zs, zz = z*zs
//   R = [[1-(yy+zz), xy-wz, xz+wy], [xy+wz, 1-(xx+zz), yz-wx], [xz-wy, yz+wx, 1-(xx+yy)]]      (R[3*a + j] = R_aj)
// The columns of R are the box's axes in the world.
//   into the frame (ob_into):     u'_j = (R_0j*u_0 + R_1j*u_1) + R_2j*u_2
//   back to the world (ob_back):  u_a  = (R_a0*u'_0 + R_a1*u'_1) + R_a2*u'_2
// ---- 2. Validity.  A query is valid iff it passes ov_query_valid (overlap) or sb_query_valid (sweep) on center, half_extent (and
// direction, tmax), all four components of q are finite, and n is finite and > 0.  Anything else touches nothing, or is the miss
// record carrying tmax as given, without a walk.  (An n that overflows, the zero quaternion and an n that underflows to 0 are
// invalid; (0, 0, 1e-10, 1e-10) has n = 2e-20 and is valid.)
// ---- 3. A triangle, from its record's v0, e1, e2: a_k exactly as ov_triangle / sb_triangle compute them - v0 - c, (v0 + e1) - c,
// (v0 + e2) - c - then a'_k = into(a_k), e1' = into(e1), e2' = into(e2) and, for the sweep, d' = into(direction).  The answer is
// ov_triangle_rel(a'_0, a'_1, a'_2, e1', e2', h) or sb_triangle_rel(.., q') with q' = (h, d', dd = dot(d', d')): inside them f1 =
// e2' - e1', and "all nine components finite" is asked of the a'_k.
// ---- 4. A sphere primitive (centre o): o' = into(o - c), then ov_sphere / sb_sphere / sb_sphere_normal with centre o', box centre
// 0, h and d'.
// ---- 5. The sweep's answer: t, axis, prim_id, material_id as in "Box sweeps", axis read in the box's frame; normal =
// back(normal') + 0.0f per component.  Order and acceptance are unchanged: (bits of t, key) from (bits of tmax, 0), strict.
// ---- 6. Consequences.
// (a) rotation = (0, 0, 0, w), w finite and != 0: every product with x, y or z is a zero, every off-diagonal entry a sum or
//     difference of zeros, every diagonal entry 1 - 0 = 1: R is the identity up to the signs of its zeros.  With x = y = z = +0 the
//     off-diagonal entries are all +0, also for w < 0 (0 - (-0) = +0, 0 + (-0) = +0); a -0 among x, y, z makes some of them -0
//     (x = -0, w > 0: xy - wz = -0 - 0 = -0).  Either way into and back are (1*u_j + (+-0)*u_b) + (+-0)*u_c = u_j for finite u, so
//     both calls return rt_overlap_box's and rt_sweep_box's bytes; a non-finite a_k gives a NaN (0 * inf) and is rejected, as there.
//     The one thing that can change is the sign of a zero: u_j = -0 may come out +0, never anything else.  No comparison of the
//     statement tells the zeros apart, t is t_in + 0.0f and a triangle's normal has its own + 0.0f, so no output bit moves - with ONE
//     exception: sb_sphere_normal may return a component -0 (a half extent 0 on an axis on which the sphere's centre lies at +0 at
//     the contact: clamp(P) - P = -0 - +0), and back(..) + 0.0f turns it into +0 here.
// (b) rt_sweep_obb answers t = 0 with axis NONE for a triangle exactly when rt_overlap_obb lists it for the start pose: both run
//     the same a'_k, e1', e2', h through sb_triangle_rel and ov_triangle_rel, and sweep_box_rules.h shows that the first gives (0,
//     NONE) iff the second holds.
// (c) The walks only cull: the result does not depend on the tree, the device count, the kind of memory or the chunking.
// ---- 7. The cull, in world space.  The world bounding box of the turned box has half extents
//   H_a = ((|R_a0|*h_0 + |R_a1|*h_1) + |R_a2|*h_2) + RT_OBB_SLACK * max_j h_j
// The overlap walk is ov_node_reach with (c, H), the sweep walk sb_node_bounds with (c, H, direction) and the direction's octant,
// culled by the best time.  A half extent so large that H overflows to +inf (h near FLT_MAX) makes every slot's test hold: every
// slot is followed, which costs visits and never an answer.  Why their own margins with this widening cover the rounding of R, of H
// and of the frame products: DESIGN.md section 4, "Oriented boxes".  The bound is loose for a long box turned 45 degrees (its
// bounding box has up to 3 sqrt 3 times the volume).
#ifndef RT_OBB_RULES_H
#define RT_OBB_RULES_H

#include "sweep_box_rules.h"

namespace rt {

#ifndef RT_OBB_SLACK
#define RT_OBB_SLACK 1.0e-5f
#endif

// rules 1 and 2: R from q; false when q is not a valid rotation (R is then not to be used)
RT_RULE bool ob_frame(const float q[4], float R[9]) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float n = ((x * x + y * y) + z * z) + w * w, s = 2.0f / n;
    const float xs = x * s, ys = y * s, zs = z * s;
    const float wx = w * xs, wy = w * ys, wz = w * zs;
    const float xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, yz = y * zs, zz = z * zs;
    R[0] = 1.0f - (yy + zz), R[1] = xy - wz, R[2] = xz + wy;
    R[3] = xy + wz, R[4] = 1.0f - (xx + zz), R[5] = yz - wx;
    R[6] = xz - wy, R[7] = yz + wx, R[8] = 1.0f - (xx + yy);
    return ov_finite(x) && ov_finite(y) && ov_finite(z) && ov_finite(w) && ov_finite(n) && n > 0.0f;
}
RT_RULE void ob_into(const float R[9], const float u[3], float out[3]) {
    RT_CP_UNROLL
    for (int j = 0; j < 3; j++) out[j] = (R[j] * u[0] + R[3 + j] * u[1]) + R[6 + j] * u[2];
}
RT_RULE void ob_back(const float R[9], const float u[3], float out[3]) {
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) out[a] = (R[3 * a] * u[0] + R[3 * a + 1] * u[1]) + R[3 * a + 2] * u[2];
}
// rule 7
RT_RULE void ob_world_half(const float R[9], const float h[3], float H[3]) {
    const float wd = RT_OBB_SLACK * ov_max(ov_max(h[0], h[1]), h[2]);
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) H[a] = ((fabsf(R[3 * a]) * h[0] + fabsf(R[3 * a + 1]) * h[1]) + fabsf(R[3 * a + 2]) * h[2]) + wd;
}
// rule 3: the record in the frame
struct ObTriangle {
    float a0[3], a1[3], a2[3], e1[3], e2[3];
};
RT_RULE void ob_triangle_into(const float rec[9], const float c[3], const float R[9], ObTriangle& t) {
    float a0[3], a1[3], a2[3];
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) a0[a] = rec[a] - c[a], a1[a] = (rec[a] + rec[3 + a]) - c[a], a2[a] = (rec[a] + rec[6 + a]) - c[a];
    ob_into(R, a0, t.a0), ob_into(R, a1, t.a1), ob_into(R, a2, t.a2), ob_into(R, rec + 3, t.e1), ob_into(R, rec + 6, t.e2);
}
// rule 4
RT_RULE void ob_sphere_into(const float centre[3], const float c[3], const float R[9], float o[3]) {
    const float g[3] = {centre[0] - c[0], centre[1] - c[1], centre[2] - c[2]};
    ob_into(R, g, o);
}

// ---- The overlap query.  `world` is what the walk culls by; c, h, R are what the leaves are tested with.
struct ObBox {
    float c[3], h[3], R[9];
    OvBox world;
};
RT_RULE bool ob_query_valid(const float c[3], const float h[3], const float q[4], float R[9]) { return ob_frame(q, R) && ov_query_valid(c, h); }
// after ob_query_valid has filled b.R
RT_RULE void ob_box_init(ObBox& b, const float c[3], const float h[3]) {
    float H[3];
    for (int a = 0; a < 3; a++) b.c[a] = c[a], b.h[a] = h[a];
    ob_world_half(b.R, h, H);
    ov_box_init(b.world, c, H);
}
RT_RULE bool ob_triangle(const float rec[9], const ObBox& b) {
    ObTriangle t;
    ob_triangle_into(rec, b.c, b.R, t);
    return ov_triangle_rel(t.a0, t.a1, t.a2, t.e1, t.e2, b.h);
}
RT_RULE bool ob_sphere(const float centre[3], float radius, const ObBox& b) {
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    float o[3];
    ob_sphere_into(centre, b.c, b.R, o);
    return ov_sphere(o, radius, zero, b.h);
}
template <int MODE>
struct ObVisit {
    const ObBox& b;
    OvList& list;
    uint32_t reach;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        uint32_t code;
        reach = ov_node_reach(w, b.world, code);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return reach & occupied; }
    template <class Access>
    RT_RULE bool leaf(Access& acc, uint32_t, const float q[9], const uint32_t ids[3]) {
        const uint32_t key = ids[1] ^ RT_PRIM_SPHERE_FLAG;
        if (!(ov_list_wants<MODE>(list, key) && ob_triangle(q, b))) return false;
        ov_list_offer(acc, list, key);
        return MODE == OV_ANY;
    }
};
template <int MODE, class Access>
RT_RULE void ob_walk(Access& acc, uint32_t n_nodes, const ObBox& b, OvList& list) {
    ObVisit<MODE> v{b, list, 0u};
    group_walk(acc, n_nodes, v);
}

// ---- The sweep.  f is the query in the frame (centre 0, h, d'), w the query the walk culls by (c, H, direction).
struct ObSweep {
    float c[3], R[9];
    SbQuery f, w;
};
// false: a miss without a walk, carrying tmax as given
RT_RULE bool ob_sweep_init(ObSweep& s, const float c[3], const float h[3], const float q[4], const float d[3], float tmax) {
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    float dl[3], H[3];
    const bool ok = ob_frame(q, s.R) && sb_query_valid(sb_query(c, h, d, tmax));
    for (int a = 0; a < 3; a++) s.c[a] = c[a];
    // (an invalid query's R may hold NaNs; what is built from it below is not read, the caller reports the miss)
    ob_into(s.R, d, dl);
    s.f = sb_query(zero, h, dl, tmax);
    ob_world_half(s.R, h, H);
    s.w = sb_query(c, H, d, tmax);
    return ok;
}
RT_RULE float ob_sweep_triangle(const float rec[9], const ObSweep& s, float limit, uint32_t& axis, float& w_in, ObTriangle& t) {
    ob_triangle_into(rec, s.c, s.R, t);
    return sb_triangle_rel(t.a0, t.a1, t.a2, t.e1, t.e2, s.f, limit, axis, w_in);
}
RT_RULE float ob_sweep_sphere(const float centre[3], float radius, const ObSweep& s) {
    float o[3];
    ob_sphere_into(centre, s.c, s.R, o);
    return sb_sphere(o, radius, s.f);
}
struct ObSweepVisit {
    const ObSweep& s;
    float c_max, inv[3], L[8];
    uint32_t code, alive;
    CpBest& best;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        sb_node_bounds(w, s.w, inv, code, c_max, L, alive);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return sw_pass(L, sw_best_t(best.order), occupied & alive); }
    template <class Access>
    RT_RULE bool leaf(Access&, uint32_t slot, const float rec[9], const uint32_t ids[3]) {
        uint32_t axis;
        float w_in;
        ObTriangle t;
        const uint64_t c = cp_order(ob_sweep_triangle(rec, s, sw_best_t(best.order), axis, w_in, t), ids[1] ^ RT_PRIM_SPHERE_FLAG);
        if (c < best.order) best.order = c, best.slot = slot;
        return false;
    }
};
template <class Access>
RT_RULE void ob_sweep_walk(Access& acc, uint32_t n_nodes, const ObSweep& s, CpBest& best) {
    ObSweepVisit v{s, cp_p_max(s.c), {1.0f / s.w.d[0], 1.0f / s.w.d[1], 1.0f / s.w.d[2]}, {}, sw_octant(s.w.d), 0u, best};
    group_walk(acc, n_nodes, v);
}
// rule 5: the eight words of an rt_box_sweep_hit, the winner's statement evaluated once more with no limit (the miss is sb_answer_miss)
RT_RULE void ob_answer_normal(const ObSweep& s, const float local[3], uint32_t out[8]) {
    float normal[3];
    ob_back(s.R, local, normal);
    out[0] = cp_bits(normal[0] + 0.0f), out[1] = cp_bits(normal[1] + 0.0f), out[2] = cp_bits(normal[2] + 0.0f);
}
RT_RULE void ob_answer_triangle(const float rec[9], uint32_t material_id, uint64_t order, const ObSweep& s, uint32_t out[8]) {
    uint32_t axis;
    float w_in, local[3];
    ObTriangle t;
    (void)ob_sweep_triangle(rec, s, INFINITY, axis, w_in, t);
    sb_axis_normal(t.e1, t.e2, axis, w_in, local);
    ob_answer_normal(s, local, out);
    out[3] = (uint32_t)(order >> 32), out[4] = axis, out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}
RT_RULE void ob_answer_sphere(const float centre[3], float radius, uint32_t material_id, uint64_t order, const ObSweep& s, uint32_t out[8]) {
    const float t = sw_best_t(order);
    float o[3], local[3] = {0.0f, 0.0f, 0.0f};
    ob_sphere_into(centre, s.c, s.R, o);
    if (t > 0.0f) sb_sphere_normal(o, radius, s.f, t, local);
    ob_answer_normal(s, local, out);
    out[3] = (uint32_t)(order >> 32), out[4] = t > 0.0f ? SB_AXIS_SPHERE : SB_AXIS_NONE, out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG;
    out[7] = material_id;
}

} // namespace rt
#endif
