// contact_capsule_rules.h — the contact query (rt_contact_capsule, include/rt_hip.h "Contact queries"), stated once.
//
// For a RESTING capsule - every point within `radius` of the segment origin .. origin + axis - the K nearest primitives whose distance
// from the axis segment is below the radius, nearest first: a nearest-K query around a segment instead of a point.  Two pieces of code
// answer it: the kernel (contact_capsule.hip) and the host walk of tests/check_contact_capsule.cpp, which holds every record and count
// to a brute-force sort before any kernel runs.  Both call what is here.  Almost all of it is stated elsewhere and used as it is:
//   cap_triangle, sc_sphere_pose, sc_clamp01     sweep_capsule_rules.h: the closest pair of an axis segment and a triangle; a sphere's
//                                                centre against the axis
//   cp_order, cp_start, cp_pass, cp_sphere, cp_triangle_position, cp_answer_miss      closest_point_rules.h
//   CpList, cp_list_init, cp_list_offer, cp_list_cull, cp_list_count                  closest_point_all_rules.h
//   group_walk                                                                        group_walk.h
// New are the sphere candidate (rule 2), the node bound (rule 4), the visitor (rule 5) and the record (rule 6).  The RT_RULE convention:
// host and device under hipcc, host only elsewhere; every operation is one f32 rounding and nothing is fused outside the node bound
// (the build uses -ffp-contract=off; the fused operations are written fmaf), so numpy reproduces the bits
// (tests/contact_capsule_cases.py).
//
// With axis == 0 exactly the query IS rt_closest_point_all: B = A + 0 has the value of A, cap_triangle's candidates b, c and d never
// replace candidate a (b ties, and only a strictly nearer one replaces; c and d need aa > 0), the sphere's three cases collapse to
// fabsf(len - R), the node bound's interval is the point, its p_max is cp_p_max(A) and the midpoint is A: dist2, the list, the counts,
// the walk's visits and tests, position, distance, prim_id and material_id are rt_closest_point_all's bit for bit, and s = 0.
#ifndef RT_CONTACT_CAPSULE_RULES_H
#define RT_CONTACT_CAPSULE_RULES_H

#include "closest_point_all_rules.h"
#include "sweep_capsule_rules.h"

namespace rt {

enum CcMode : int { CC_LIST = 0, CC_COUNT_ALL = 1, CC_ANY = 2 };

// ---- 0. A query, from the 32 bytes of an rt_capsule (origin radius | axis pad; the first 32 bytes of an rt_capsule_sweep).  B = A +
// axis and the midpoint A + axis * 0.5f per component; p_max is the largest |coordinate| of either end.  A DEGENERATE query lists
// nothing and is not walked: a non-finite component of origin or axis, or a radius that is NaN or <= 0 (cp_query_valid and a finite
// axis).  A radius of +inf is allowed, as for rt_closest_point.
struct CcQuery {
    float A[3], r, ax[3], aa;
    float lo[3], hi[3], mid[3], p_max; // for the node bound: the axis segment's interval per axis, its midpoint, max over both ends
};
RT_RULE CcQuery cc_query(const float origin[3], float radius, const float axis[3]) {
    CcQuery q;
    q.r = radius;
    q.p_max = 0.0f;
    for (int a = 0; a < 3; a++) {
        const float B = origin[a] + axis[a];
        q.A[a] = origin[a], q.ax[a] = axis[a];
        q.lo[a] = B < origin[a] ? B : origin[a], q.hi[a] = B > origin[a] ? B : origin[a];
        q.mid[a] = origin[a] + axis[a] * 0.5f;
        q.p_max = rule_max(q.p_max, rule_max(fabsf(origin[a]), fabsf(B)));
    }
    q.aa = cp_dot(axis, axis);
    return q;
}
RT_RULE bool cc_query_valid(const CcQuery& q) {
    return cp_query_valid(q.A, q.r) && std::isfinite(q.ax[0]) && std::isfinite(q.ax[1]) && std::isfinite(q.ax[2]);
}

// ---- 1. A triangle, from its record's v0, e1, e2:  dist2, s, v, w = cap_triangle(v0, e1, e2, origin, axis, aa), as it is.
RT_RULE float cc_triangle(const float v0[3], const float e1[3], const float e2[3], const CcQuery& q, float& s, float& v, float& w) {
    return cap_triangle(v0, e1, e2, q.A, q.ax, q.aa, s, v, w);
}

// ---- 2. A sphere is its surface (centre C, radius R), as in rt_closest_point.  lenA, lenB, f, dmin, mA = A - C from sc_sphere_pose;
// dmax = lenB > lenA ? lenB : lenA.  The first of these that holds gives the distance d of the surface from the axis and the place s:
//   OUTSIDE        dmin > R:                d = dmin - R;  s = f, the foot of C on the axis
//   WHOLLY INSIDE  dmax < R:                d = R - dmax;  s = lenB > lenA ? 1 : 0, the end farther from C, A on a tie (sc_sphere_s)
//   CROSSING       dmin <= R && R <= dmax:  d = 0;  s = the smallest root in [0, 1] of |mA + axis s| = R:
//        b = dot(mA, axis);  c = dot(mA, mA) - R * R;  disc = b * b - aa * c;  q = disc > 0 ? sqrtf(disc) : 0
//        s = aa > 0 ? clamp((lenA > R ? -b - q : q - b) / aa) : 0
//      A outside the ball: the axis enters it, the lower root; A inside or on the surface: B is outside or on it, the upper root.  A
//      zero axis has lenA == R here and s = 0.
//   none (a NaN in the centre or the radius):  d = NaN
// dist2 = d * d, so a NaN sphere is never in range.  The point is cp_sphere's from p_a = A_a + axis_a * s.
RT_RULE float cc_sphere(const float centre[3], float radius, const CcQuery& q, float& s) {
    float lenA, lenB, f, dmin, mA[3], mB[3];
    sc_sphere_pose(q.A, centre, q.ax, q.aa, lenA, lenB, f, dmin, mA, mB);
    const float dmax = lenB > lenA ? lenB : lenA;
    float d = NAN;
    s = 0.0f;
    if (dmin > radius) d = dmin - radius, s = f;
    else if (dmax < radius) d = radius - dmax, s = lenB > lenA ? 1.0f : 0.0f;
    else if (dmin <= radius && radius <= dmax) {
        const float b = cp_dot(mA, q.ax), c = cp_dot(mA, mA) - radius * radius, disc = b * b - q.aa * c;
        const float sq = disc > 0.0f ? sqrtf(disc) : 0.0f;
        d = 0.0f;
        s = q.aa > 0.0f ? sc_clamp01((lenA > radius ? -b - sq : sq - b) / q.aa) : 0.0f;
    }
    return d * d;
}
RT_RULE void cc_sphere_position(const float centre[3], float radius, const CcQuery& q, float s, float pos[3]) {
    const float p[3] = {q.A[0] + q.ax[0] * s, q.A[1] + q.ax[1] * s, q.A[2] + q.ax[2] * s};
    (void)cp_sphere(centre, radius, p, pos);
}

// ---- 3. Order, range and list: rt_closest_point_all's.  A candidate is cp_order(dist2, key), key = prim_id ^ RT_PRIM_SPHERE_FLAG; it
// is IN RANGE iff it is below cp_start(radius): only dist2 < radius * radius is accepted, strictly, and a NaN or infinite dist2 never.
// The list is CpList with cp_list_offer and cp_list_cull, unchanged.
// This differs from rt_sweep_capsule's start-in-contact test (cap_triangle <= rr; for a sphere dmin - R <= r && R - dmax <= r) exactly
// at equality: a listed contact implies t = 0 there for the same pose (for a triangle by the same dist2 and rr; for a sphere both of
// its differences are then at most d < r), and the converse fails only at dist2 == radius * radius, which the sweep counts as contact
// and this query, like every closest-point query, does not list.

// ---- 4. The lower bound of a node's eight child boxes: a lower bound of dist2 for every record under a child box.  The planes as
// cp_node_bounds decodes them, lo = fmaf(q_lo, scale, org), hi likewise.  Per axis the gap between the axis segment's interval
// [min(A_a, B_a), max(A_a, B_a)] and [lo_a, hi_a], reduced by cp_node_bounds' slack and clamped at 0:
//   g_a = max(lo_a - qhi_a, qlo_a - hi_a, 0);  g'_a = max(g_a - s, 0);  L = dot(g', g')
//   s = RT_CP_SLACK * (p_max + max_a (|org_a| + 255 * scale_a)),  p_max over both ends
// and `code`: bit a set when the MIDPOINT of the axis lies on the high side of the node's box centre on axis a.  With a zero axis
// qlo = qhi = A and this is cp_node_bounds value for value.  A slot is culled iff L > the cull distance, strictly (cp_pass).
// The bound is the distance between two BOXES, the segment's and the child's: exact for an axis along a coordinate axis, loose for a
// long diagonal capsule, whose box is mostly empty.  A tighter segment-box distance is out of scope here.
// Why s suffices: DESIGN.md section 4, "Contact queries".  A NaN bound (B overflowed to an infinity) compares false and is followed.
RT_RULE void cc_node_bounds(const uint32_t w[20], const CcQuery& q, float L[8], uint32_t& code) {
    float org[3], scale[3], m = 0.0f;
    code = 0u;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        org[a] = cp_float(w[a]);
        scale[a] = ldexpf(1.0f, (int)(int8_t)((w[3] >> (8 * a)) & 0xFFu));
        m = rule_max(m, fmaf(255.0f, scale[a], fabsf(org[a])));
        if (q.mid[a] > fmaf(127.5f, scale[a], org[a])) code |= 1u << a;
    }
    const float s = RT_CP_SLACK * (q.p_max + m);
    RT_CP_UNROLL
    for (int sl = 0; sl < 8; sl++) {
        float g[3];
        RT_CP_UNROLL
        for (int a = 0; a < 3; a++) {
            const float lo = fmaf((float)((w[8 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xFFu), scale[a], org[a]);
            const float hi = fmaf((float)((w[14 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xFFu), scale[a], org[a]);
            g[a] = rule_max(rule_max(rule_max(lo - q.hi[a], q.lo[a] - hi), 0.0f) - s, 0.0f);
        }
        L[sl] = cp_dot(g, g);
    }
}

// ---- 5. The walk: group_walk with CpAllVisit's passes and every record offered to the list.  In ANY mode the list has cap 0 (its
// bound stays cp_start(radius)) and the walk ends at the first candidate in range, which it counts in list.total; the caller does not
// start the walk when a sphere is already in range.
template <bool COUNT_ALL, bool ANY>
struct CcVisit {
    const CcQuery& q;
    float L[8];
    CpList& list;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        uint32_t code;
        cc_node_bounds(w, q, L, code);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return cp_pass(L, cp_list_cull<COUNT_ALL>(list), occupied); }
    template <class Access>
    RT_RULE bool leaf(Access& acc, uint32_t slot, const float rec[9], const uint32_t ids[3]) {
        float s, v, wgt;
        const uint64_t c = cp_order(cc_triangle(rec, rec + 3, rec + 6, q, s, v, wgt), ids[1] ^ RT_PRIM_SPHERE_FLAG);
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
RT_RULE void cc_walk(Access& acc, uint32_t n_nodes, const CcQuery& q, CpList& list) {
    CcVisit<MODE == CC_COUNT_ALL, MODE == CC_ANY> v{q, {}, list};
    group_walk(acc, n_nodes, v);
}
// a sphere's candidate, offered as a record's is; true: ANY mode has its answer
template <int MODE, class Access>
RT_RULE bool cc_offer_sphere(Access& acc, CpList& list, uint64_t c, uint32_t index) {
    if (MODE == CC_ANY) {
        if (!(c < list.start)) return false;
        list.total++;
        return true;
    }
    cp_list_offer<MODE == CC_COUNT_ALL>(acc, list, c, index);
    return false;
}
// what rt_contact_capsule reports in counts[i]
template <int MODE>
RT_RULE uint32_t cc_list_count(const CpList& l) {
    return MODE == CC_LIST ? l.n : MODE == CC_COUNT_ALL ? l.total : (l.total ? 1u : 0u);
}

// ---- 6. The answer, as the eight words of an rt_contact: position | distance = sqrtf(dist2) | s | 0 | prim_id as rt_hit | the
// record's material id, unchecked - rt_capsule_sweep_hit's layout with the distance where t is.  A listed entry's statement is
// evaluated once more for s, v, w and the point: position = v0 + (e1 v + e2 w), or cp_sphere's point from A + axis s.  An unused slot
// is cp_answer_miss(radius): position 0, the radius as given, s = 0, 0, prim_id 0xFFFFFFFF, material 0.
RT_RULE void cc_answer_triangle(const float rec[9], uint32_t material_id, uint64_t order, const CcQuery& q, uint32_t out[8]) {
    float s, v, w, pos[3];
    (void)cc_triangle(rec, rec + 3, rec + 6, q, s, v, w);
    cp_triangle_position(rec, rec + 3, rec + 6, v, w, pos);
    out[0] = cp_bits(pos[0]), out[1] = cp_bits(pos[1]), out[2] = cp_bits(pos[2]), out[3] = cp_bits(sqrtf(cp_best_dist2(order)));
    out[4] = cp_bits(s), out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}
RT_RULE void cc_answer_sphere(const float centre[3], float radius, uint32_t material_id, uint64_t order, const CcQuery& q, uint32_t out[8]) {
    float s, pos[3];
    (void)cc_sphere(centre, radius, q, s);
    cc_sphere_position(centre, radius, q, s, pos);
    out[0] = cp_bits(pos[0]), out[1] = cp_bits(pos[1]), out[2] = cp_bits(pos[2]), out[3] = cp_bits(sqrtf(cp_best_dist2(order)));
    out[4] = cp_bits(s), out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}

} // namespace rt
#endif
