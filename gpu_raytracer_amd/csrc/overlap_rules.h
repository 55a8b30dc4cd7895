// overlap_rules.h — the overlap query (rt_overlap_box, include/rt_hip.h "Overlap queries"), stated once.
//
// Two pieces of code answer it: the kernel (overlap.hip) and the host walk of tests/check_overlap.cpp, which holds the whole walk to a
// brute force over all primitives before any kernel runs.  Both call what is here: when a triangle and when a sphere TOUCHES a closed
// axis-aligned box, the list of the K lowest keys, which child boxes of a node the query box reaches, and the visitor that
// group_walk (group_walk.h) runs.  The RT_RULE convention of group_walk.h: host and device under hipcc, host only elsewhere;
// every operation is one f32 rounding and nothing is fused (the build uses -ffp-contract=off), so numpy reproduces the bits
// (tests/overlap_cases.py).  dot is cp_dot.
//
// Every test is stated in its POSITIVE form - "not separated on this axis" - so that a NaN makes it false and the primitive is not
// listed.  A primitive touches iff ALL its tests hold; the answer does not depend on the order in which they are evaluated, so
// ov_triangle orders them for early rejection.
#ifndef RT_OVERLAP_RULES_H
#define RT_OVERLAP_RULES_H

#include <cfloat>

#include "closest_point_rules.h"

namespace rt {

enum OvMode : int { OV_LIST = 0, OV_COUNT_ALL = 1, OV_ANY = 2 };

// min and max that ignore a NaN operand, the same on host and device (rule_min / rule_max differ between the two there).  Where a NaN
// must make a test false the test says so itself (ov_span).
RT_RULE float ov_min(float a, float b) { return fminf(a, b); }
RT_RULE float ov_max(float a, float b) { return fmaxf(a, b); }
RT_RULE bool ov_finite(float x) { return fabsf(x) <= FLT_MAX; }

// ---- 1. A query.  c the centre and h the half extent of a closed box; h = 0 on an axis is allowed (a slab, a segment, a point).  A
// DEGENERATE query - a non-finite component of either, or a negative half extent - touches nothing and is not walked.
struct OvBox {
    float c[3], h[3];
    float lo[3], hi[3]; // c - h, c + h: what the node test holds the child boxes against
    float reach;        // max_a |c_a| + max_a h_a: the query's share of the node test's slack
};
RT_RULE bool ov_query_valid(const float c[3], const float h[3]) {
    bool ok = true;
    for (int a = 0; a < 3; a++) ok = ok && ov_finite(c[a]) && ov_finite(h[a]) && h[a] >= 0.0f;
    return ok;
}
RT_RULE void ov_box_init(OvBox& b, const float c[3], const float h[3]) {
    for (int a = 0; a < 3; a++) b.c[a] = c[a], b.h[a] = h[a], b.lo[a] = c[a] - h[a], b.hi[a] = c[a] + h[a];
    b.reach = cp_p_max(c) + ov_max(ov_max(h[0], h[1]), h[2]);
}
// The same from finite bounds lo <= hi that are exact (overlap_triangle_rules.h: the min and max of a triangle's vertices), for a
// caller whose leaf test does not read c and h: the node test holds the child boxes against lo and hi as given, c = 0.5 lo + 0.5 hi
// serves the visiting order only, h = hi - c is not read by the node test, and reach = max_a max(|lo_a|, |hi_a|) bounds every
// coordinate of the query as max_a |c_a| + max_a h_a does above.
RT_RULE void ov_box_init_bounds(OvBox& b, const float lo[3], const float hi[3]) {
    b.reach = 0.0f;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = lo[a], b.hi[a] = hi[a], b.c[a] = 0.5f * lo[a] + 0.5f * hi[a], b.h[a] = hi[a] - b.c[a];
        b.reach = ov_max(b.reach, ov_max(fabsf(lo[a]), fabsf(hi[a])));
    }
}

// ---- 2. A triangle, from its record's v0, e1, e2 (the stored f32 differences).  Relative to the centre its vertices are
//   a0 = v0 - c,  a1 = (v0 + e1) - c,  a2 = (v0 + e2) - c
// and it touches iff it is separated from the box on none of thirteen axes (Akenine-Moeller, Fast 3D Triangle-Box Overlap Testing,
// 2001), after
//   0. all nine components of a0, a1, a2 are finite: a triangle with a non-finite vertex is never listed (an infinite vertex alone
//      would pass the comparisons below as inf <= inf).
//   1. the three box axes:    min_k a_k[x] <= h[x] && max_k a_k[x] >= -h[x], likewise y and z
//   2. the normal:            n = cross(e1, e2); d = dot(n, a0); r = dot(|n|, h);  d <= r && d >= -r
//   3. the nine cross(unit_i, f_j), f_0 = e1, f_1 = e2 - e1, f_2 = e2, without the multiplications by 0 and 1; for f = f_j:
//        i = x:  p_k = f.y * a_k.z - f.z * a_k.y;  r = |f.z| * h.y + |f.y| * h.z
//        i = y:  p_k = f.z * a_k.x - f.x * a_k.z;  r = |f.z| * h.x + |f.x| * h.z
//        i = z:  p_k = f.x * a_k.y - f.y * a_k.x;  r = |f.y| * h.x + |f.x| * h.y
//      for all three vertices k, and the test ov_span:  min_k p_k <= r && max_k p_k >= -r, and no p_k is a NaN.
// The box is closed: a triangle that only touches a face, an edge or a corner is listed (every comparison admits equality), one that
// lies an ulp outside is not.  A degenerate triangle has n = 0 and some f = 0, whose tests hold as 0 <= 0: it comes out as the
// segment or point test the remaining axes make.  After test 0 the a_k are finite, so the min and max of test 1 see no NaN; d and r
// of test 2 are single values, which a NaN fails by itself; the p_k of test 3 can only be NaN through an overflow in f or in the
// products, and ov_span's sum, which is NaN as soon as one of them is, fails it then.
RT_RULE bool ov_span(float p0, float p1, float p2, float r) {
    const float s = (p0 + p1) + p2;
    return ov_min(ov_min(p0, p1), p2) <= r && ov_max(ov_max(p0, p1), p2) >= -r && s == s;
}
RT_RULE bool ov_cross_axes(const float f[3], const float a0[3], const float a1[3], const float a2[3], const float h[3]) {
    const float g[3] = {fabsf(f[0]), fabsf(f[1]), fabsf(f[2])};
    return ov_span(f[1] * a0[2] - f[2] * a0[1], f[1] * a1[2] - f[2] * a1[1], f[1] * a2[2] - f[2] * a2[1], g[2] * h[1] + g[1] * h[2]) &&
           ov_span(f[2] * a0[0] - f[0] * a0[2], f[2] * a1[0] - f[0] * a1[2], f[2] * a2[0] - f[0] * a2[2], g[2] * h[0] + g[0] * h[2]) &&
           ov_span(f[0] * a0[1] - f[1] * a0[0], f[0] * a1[1] - f[1] * a1[0], f[0] * a2[1] - f[1] * a2[0], g[1] * h[0] + g[0] * h[1]);
}
// The statement is written once, over a source of the relative vertices: `rel(a, p0, p1, p2)` gives component a of a0, a1, a2.
// ov_triangle's source is its own subtraction, made axis by axis inside the loop as it always was; ov_triangle_rel's is a caller
// that has the three relative vertices already, in another frame (obb_rules.h: a0, a1, a2, e1, e2 in the box's own axes).
template <class Rel>
RT_RULE bool ov_triangle_from(const Rel& rel, const float e1[3], const float e2[3], const float h[3]) {
    float a0[3], a1[3], a2[3];
    bool ok = true;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        rel(a, a0[a], a1[a], a2[a]);
        ok = ok && ov_finite(a0[a]) && ov_finite(a1[a]) && ov_finite(a2[a]);
        ok = ok && ov_min(ov_min(a0[a], a1[a]), a2[a]) <= h[a] && ov_max(ov_max(a0[a], a1[a]), a2[a]) >= -h[a];
    }
    if (!ok) return false; // most records a walk reaches end here
    const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float an[3] = {fabsf(n[0]), fabsf(n[1]), fabsf(n[2])};
    const float d = cp_dot(n, a0), r = cp_dot(an, h);
    if (!(d <= r && d >= -r)) return false;
    const float f1[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    return ov_cross_axes(e1, a0, a1, a2, h) && ov_cross_axes(f1, a0, a1, a2, h) && ov_cross_axes(e2, a0, a1, a2, h);
}
// (sweep_box_rules.h uses the same two sources for sb_triangle_from, with q.c as c: change them with both statements in mind)
struct OvFromRecord { // a_k = v0 - c, (v0 + e1) - c, (v0 + e2) - c
    const float *v0, *e1, *e2, *c;
    RT_RULE void operator()(int a, float& p0, float& p1, float& p2) const { p0 = v0[a] - c[a], p1 = (v0[a] + e1[a]) - c[a], p2 = (v0[a] + e2[a]) - c[a]; }
};
struct OvFromRelative {
    const float *a0, *a1, *a2;
    RT_RULE void operator()(int a, float& p0, float& p1, float& p2) const { p0 = a0[a], p1 = a1[a], p2 = a2[a]; }
};
RT_RULE bool ov_triangle(const float v0[3], const float e1[3], const float e2[3], const float c[3], const float h[3]) {
    return ov_triangle_from(OvFromRecord{v0, e1, e2, c}, e1, e2, h);
}
RT_RULE bool ov_triangle_rel(const float a0[3], const float a1[3], const float a2[3], const float e1[3], const float e2[3], const float h[3]) {
    return ov_triangle_from(OvFromRelative{a0, a1, a2}, e1, e2, h);
}

// ---- 3. A sphere is its surface, as in rt_closest_point:
//   oc = centre - c;  g = |oc| per axis;  near = max(g - h, 0);  far = g + h;  rr = radius * radius
// near is the box's point nearest the centre and far its farthest corner, both relative to the centre, so the surface passes through
// the box iff dot(near, near) <= rr && dot(far, far) >= rr: a box wholly inside the ball is not touched.  A NaN centre or radius
// makes far or rr a NaN and fails the second comparison.
RT_RULE bool ov_sphere(const float centre[3], float radius, const float c[3], const float h[3]) {
    float near[3], far[3];
    for (int a = 0; a < 3; a++) {
        const float g = fabsf(centre[a] - c[a]);
        near[a] = ov_max(g - h[a], 0.0f), far[a] = g + h[a];
    }
    const float rr = radius * radius;
    return cp_dot(near, near) <= rr && cp_dot(far, far) >= rr;
}

// ---- 4. The list.  key = prim_id ^ RT_PRIM_SPHERE_FLAG: spheres first by sphere index, then triangles by original triangle index
// (rt_closest_point's key).  A lane's list holds the K lowest keys of the touching primitives met so far, ascending, one word per
// entry, where the caller's Access puts it:
//   uint32_t list_get(uint32_t k) / void list_set(uint32_t k, uint32_t key)
// with k < cap always (the host check verifies every index against the K the launch provides).  Insertion is cp_list_offer's: the
// tail moves up one entry at a time from the end and a full list drops its last.  Each primitive is offered once (one record per
// triangle, one parent per leaf), so `total` counts every touching primitive once.
// The list gives NO SPATIAL BOUND: a key says nothing about where its primitive lies, so list mode and COUNT_ALL both visit every node
// the box reaches.  What a full list does spare is the test of a record whose key is above its last entry's (ov_list_wants): such a
// record could not enter, and in list mode nothing else is asked about it.
struct OvList {
    uint32_t cap, n, total;
    uint32_t last; // the list's last key once it is full; 0xFFFFFFFF before (no key is that high: RT_PRIM_MISS is no primitive)
};
RT_RULE void ov_list_init(OvList& l, uint32_t cap) { l.cap = cap, l.n = l.total = 0u, l.last = 0xFFFFFFFFu; }
template <int MODE>
RT_RULE bool ov_list_wants(const OvList& l, uint32_t key) {
    return MODE != OV_LIST || key < l.last;
}
// a touching primitive's key
template <class Access>
RT_RULE void ov_list_offer(Access& acc, OvList& l, uint32_t key) {
    l.total++;
    if (l.cap == 0u || !(key < l.last)) return;
    uint32_t j = l.n < l.cap ? l.n : l.cap - 1u;
    while (j > 0u) {
        const uint32_t prev = acc.list_get(j - 1u);
        if (!(key < prev)) break;
        acc.list_set(j, prev);
        j--;
    }
    acc.list_set(j, key);
    if (l.n < l.cap) l.n++;
    if (l.n == l.cap) l.last = acc.list_get(l.cap - 1u);
}
// what rt_overlap_box reports in counts[i]
template <int MODE>
RT_RULE uint32_t ov_list_count(const OvList& l) {
    return MODE == OV_LIST ? l.n : MODE == OV_COUNT_ALL ? l.total : (l.total ? 1u : 0u);
}

// ---- 5. The node test.  The child boxes as cp_node_bounds decodes them: lo = fmaf(q_lo, scale, org), hi likewise.  A slot is CULLED
// iff on some axis a
//   lo_a - (c_a + h_a) > s   or   (c_a - h_a) - hi_a > s,     s = RT_CP_SLACK * ((max_a |c_a| + max_a h_a) + M)
// with M = max_a (|org_a| + 255 * scale_a) as in cp_node_bounds.  The result is the mask of the slots that are not culled - a NaN
// compares false and is followed - to be masked with imask or lmask (empty slots are inverted boxes and must never be followed), and
// `code`: bit a set when the box centre lies on the high side of the node's centre on axis a (the visiting order, which is free: it
// lets ANY mode find its first primitive early).  Why s suffices: DESIGN.md section 4, "Overlap queries".
RT_RULE uint32_t ov_node_reach(const uint32_t w[20], const OvBox& b, uint32_t& code) {
    float org[3], scale[3], m = 0.0f;
    code = 0u;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        org[a] = cp_float(w[a]);
        scale[a] = ldexpf(1.0f, (int)(int8_t)((w[3] >> (8 * a)) & 0xFFu));
        m = rule_max(m, fmaf(255.0f, scale[a], fabsf(org[a])));
        if (b.c[a] > fmaf(127.5f, scale[a], org[a])) code |= 1u << a;
    }
    const float s = RT_CP_SLACK * (b.reach + m);
    uint32_t reach = 0u;
    RT_CP_UNROLL
    for (int sl = 0; sl < 8; sl++) {
        bool culled = false;
        RT_CP_UNROLL
        for (int a = 0; a < 3; a++) {
            const float lo = fmaf((float)((w[8 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xFFu), scale[a], org[a]);
            const float hi = fmaf((float)((w[14 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xFFu), scale[a], org[a]);
            culled = culled || lo - b.hi[a] > s || b.lo[a] - hi > s;
        }
        if (!culled) reach |= 1u << sl;
    }
    return reach;
}

// ---- 6. The walk: group_walk (group_walk.h).  What a node's box reaches does not change during a walk, so one mask serves its
// leaves and its inner children.  The caller supplies the Access with the list of rule 4.  In ANY mode the walk ends at the first
// touching primitive (the caller does not start it when a sphere already touches).
template <int MODE>
struct OvVisit {
    const OvBox& b;
    OvList& list;
    uint32_t reach;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        uint32_t code;
        reach = ov_node_reach(w, b, code);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return reach & occupied; }
    template <class Access>
    RT_RULE bool leaf(Access& acc, uint32_t, const float q[9], const uint32_t ids[3]) {
        const uint32_t key = ids[1] ^ RT_PRIM_SPHERE_FLAG;
        if (!(ov_list_wants<MODE>(list, key) && ov_triangle(q, q + 3, q + 6, b.c, b.h))) return false;
        ov_list_offer(acc, list, key);
        return MODE == OV_ANY;
    }
};
template <int MODE, class Access>
RT_RULE void ov_walk(Access& acc, uint32_t n_nodes, const OvBox& b, OvList& list) {
    OvVisit<MODE> v{b, list, 0u};
    group_walk(acc, n_nodes, v);
}

} // namespace rt
#endif
