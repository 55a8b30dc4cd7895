// closest_point_rules.h — the closest-point query (rt_closest_point, include/rt_hip.h "Closest-point queries"), stated once.
//
// Two pieces of code answer it: the kernel (closest_point.hip) and the host walk of tests/check_closest_point.cpp, which holds the
// whole walk to a brute force before any kernel runs.  Both call what is here: the candidate of a triangle and of a sphere, the order
// among candidates, the lower bound of a node's eight child boxes and the visitor that group_walk (group_walk.h) runs.  Plain inline
// functions under the RT_RULE convention of group_walk.h: host and device under hipcc, host only under any other compiler.  Every
// operation is one f32 rounding (the build uses -ffp-contract=off; the one fused operation is written fmaf), so numpy reproduces
// the bits (tests/closest_point_cases.py).
#ifndef RT_CLOSEST_POINT_RULES_H
#define RT_CLOSEST_POINT_RULES_H

#include <cmath>
#include <cstdint>

#include "group_walk.h"

namespace rt {

// The margin of the box bound, relative to the magnitudes that enter it (cp_node_bounds).
#ifndef RT_CP_SLACK
#define RT_CP_SLACK 1.0e-5f
#endif

RT_RULE uint32_t cp_bits(float f) {
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(f);
#else
    uint32_t u;
    __builtin_memcpy(&u, &f, sizeof u);
    return u;
#endif
}
RT_RULE float cp_float(uint32_t u) {
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float f;
    __builtin_memcpy(&f, &u, sizeof f);
    return f;
#endif
}

// (x*x + y*y) + z*z, as everywhere in this code
RT_RULE float cp_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// ---- 1. A triangle, from its record's v0, e1, e2: the weights (v, w) of v1 and v2 at the nearest point (Ericson, Real-Time
// Collision Detection 5.1.5, on the stored edges; the first region that holds, in the book's order) and the squared distance.
// Quantities are evaluated when a region first needs them; each has one expression, so the bits are those of evaluating all up front.
RT_RULE float cp_triangle(const float v0[3], const float e1[3], const float e2[3], const float p[3], float& v, float& w) {
    const float ap[3] = {p[0] - v0[0], p[1] - v0[1], p[2] - v0[2]};
    const float d1 = cp_dot(e1, ap), d2 = cp_dot(e2, ap);
    v = 0.0f, w = 0.0f;
    if (!(d1 <= 0.0f && d2 <= 0.0f)) { // else vertex v0
        const float bp[3] = {ap[0] - e1[0], ap[1] - e1[1], ap[2] - e1[2]};
        const float d3 = cp_dot(e1, bp), d4 = cp_dot(e2, bp);
        const float vc = d1 * d4 - d3 * d2;
        if (d3 >= 0.0f && d4 <= d3) v = 1.0f; // vertex v1
        else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) v = d1 / (d1 - d3); // edge v0 v1
        else {
            const float cp[3] = {ap[0] - e2[0], ap[1] - e2[1], ap[2] - e2[2]};
            const float d5 = cp_dot(e1, cp), d6 = cp_dot(e2, cp);
            const float vb = d5 * d2 - d1 * d6;
            if (d6 >= 0.0f && d5 <= d6) w = 1.0f; // vertex v2
            else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) w = d2 / (d2 - d6); // edge v0 v2
            else {
                const float va = d3 * d6 - d5 * d4;
                const float d43 = d4 - d3, d56 = d5 - d6;
                if (va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f) { // edge v1 v2
                    w = d43 / (d43 + d56);
                    v = 1.0f - w;
                } else { // the face
                    const float den = 1.0f / ((va + vb) + vc);
                    v = vb * den;
                    w = vc * den;
                }
            }
        }
    }
    const float r[3] = {(e1[0] * v + e2[0] * w) - ap[0], (e1[1] * v + e2[1] * w) - ap[1], (e1[2] * v + e2[2] * w) - ap[2]};
    return cp_dot(r, r);
}
RT_RULE void cp_triangle_position(const float v0[3], const float e1[3], const float e2[3], float v, float w, float pos[3]) {
    for (int a = 0; a < 3; a++) pos[a] = v0[a] + (e1[a] * v + e2[a] * w);
}

// ---- 2. A sphere: the nearest point of its surface, from inside or outside; at the centre the point toward +x.
RT_RULE float cp_sphere(const float centre[3], float radius, const float p[3], float pos[3]) {
    const float oc[3] = {p[0] - centre[0], p[1] - centre[1], p[2] - centre[2]};
    const float len = sqrtf(cp_dot(oc, oc));
    const float d = fabsf(len - radius);
    if (len > 0.0f) {
        const float k = radius / len;
        for (int a = 0; a < 3; a++) pos[a] = centre[a] + oc[a] * k;
    } else {
        pos[0] = centre[0] + radius, pos[1] = centre[1] + 0.0f, pos[2] = centre[2] + 0.0f;
    }
    return d * d;
}

// ---- 3. Order and acceptance.  A candidate is (dist2 bits, key) as one 64-bit unsigned number, key = prim_id ^ RT_PRIM_SPHERE_FLAG
// (sphere i -> i, triangle t -> 0x80000000 | t: rt_intersect_all's key).  dist2 >= +0 or NaN, so for everything that can be accepted bit
// order is value order.  The best starts at (bits of radius * radius, 0) and a candidate replaces it iff it is below it: only dist2 <
// radius^2 is ever accepted, strictly; a NaN (bits above +inf's) or infinite dist2 never is; equal dist2: the lower key.
RT_RULE uint64_t cp_order(float dist2, uint32_t key) { return ((uint64_t)cp_bits(dist2) << 32) | key; }
RT_RULE uint64_t cp_start(float radius) { return cp_order(radius * radius, 0u); }
RT_RULE float cp_best_dist2(uint64_t best) { return cp_float((uint32_t)(best >> 32)); }
// a query that is a miss without a walk: a non-finite position component, a NaN radius, radius <= 0
RT_RULE bool cp_query_valid(const float p[3], float radius) {
    return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && radius > 0.0f;
}

// ---- 4. The lower bound of a node's eight child boxes.  w[20]: the DevNode8 as 32-bit words.  Gives the bound L of every slot and
// `code`: bit a set when p lies on the high side of the node's box centre on axis a (the visiting order, rule 5).  cp_pass then gives
// the mask of the occupied slots (of imask or lmask: empty slots are inverted boxes and must never be followed) whose L does not
// exceed the best distance.
//   planes as visit_node8 decodes them: lo = fmaf(q_lo, scale, org), hi likewise
//   g_a = max(lo_a - p_a, p_a - hi_a, 0);  g'_a = max(g_a - s, 0);  L = dot(g', g')
//   s = RT_CP_SLACK * (max_a |p_a| + max_a (|org_a| + 255 * scale_a))
// A slot is culled iff L > best_dist2, strictly: a tie with a lower key must still be found.  Why s suffices:
// a record in the slot lies inside the decoded box up to the rounding of the planes (2^-24 M per plane, M the second max above, which
// bounds every coordinate in the node) and of the stored edges (2^-23 M); its r = (e1 v + e2 w) - ap carries at most six roundings of
// magnitudes <= 4 M + |p| per component, and v, w leave the triangle by a few 2^-24: in all below 2^-20 (M + |p|) ~ 1e-6, a tenth of
// s.  So per component g' <= |r|, and L <= dist2 in f32, both being the same monotone expression of their components.  A NaN bound (an
// overflowing grid) compares false and is followed.
RT_RULE void cp_node_bounds(const uint32_t w[20], const float p[3], float p_max, float L[8], uint32_t& code) {
    float org[3], scale[3], m = 0.0f;
    code = 0u;
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) {
        org[a] = cp_float(w[a]);
        scale[a] = ldexpf(1.0f, (int)(int8_t)((w[3] >> (8 * a)) & 0xFFu));
        m = rule_max(m, fmaf(255.0f, scale[a], fabsf(org[a])));
        if (p[a] > fmaf(127.5f, scale[a], org[a])) code |= 1u << a;
    }
    const float s = RT_CP_SLACK * (p_max + m);
    RT_CP_UNROLL
    for (int sl = 0; sl < 8; sl++) {
        float g[3];
        RT_CP_UNROLL
        for (int a = 0; a < 3; a++) {
            const float lo = fmaf((float)((w[8 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xFFu), scale[a], org[a]);
            const float hi = fmaf((float)((w[14 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xFFu), scale[a], org[a]);
            g[a] = rule_max(rule_max(rule_max(lo - p[a], p[a] - hi), 0.0f) - s, 0.0f);
        }
        L[sl] = cp_dot(g, g);
    }
}
// the slots of `occupied` a best distance of best_dist2 leaves to visit
RT_RULE uint32_t cp_pass(const float L[8], float best_dist2, uint32_t occupied) {
    uint32_t pass = 0u;
    RT_CP_UNROLL
    for (int sl = 0; sl < 8; sl++)
        if (!(L[sl] > best_dist2)) pass |= 1u << sl;
    return pass & occupied;
}
RT_RULE float cp_p_max(const float p[3]) { return rule_max(rule_max(fabsf(p[0]), fabsf(p[1])), fabsf(p[2])); }

// ---- 5. The walk: group_walk (group_walk.h, which states the groups, the stack discipline and its bound) visited by the best
// candidate so far.  `code`: the corner of the node nearest p first.
struct CpBest {
    uint64_t order;  // cp_order of the best candidate so far, cp_start(radius) while there is none
    uint32_t slot;   // its record in DevScene::tris, or its sphere index; 0xFFFFFFFF: none
};
struct CpVisit {
    const float* p;
    float p_max, L[8];
    CpBest& best;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        uint32_t code;
        cp_node_bounds(w, p, p_max, L, code);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return cp_pass(L, cp_best_dist2(best.order), occupied); }
    template <class Access>
    RT_RULE bool leaf(Access&, uint32_t slot, const float q[9], const uint32_t ids[3]) {
        float v, wgt;
        const uint64_t c = cp_order(cp_triangle(q, q + 3, q + 6, p, v, wgt), ids[1] ^ RT_PRIM_SPHERE_FLAG);
        if (c < best.order) best.order = c, best.slot = slot;
        return false;
    }
};
template <class Access>
RT_RULE void cp_walk(Access& acc, uint32_t n_nodes, const float p[3], CpBest& best) {
    CpVisit v{p, cp_p_max(p), {}, best};
    group_walk(acc, n_nodes, v);
}

// ---- 6. The answer, as the eight words of an rt_nearest: position | distance = sqrtf(dist2) | u, v (the weights of v1 and v2; 0 for
// a sphere) | prim_id as rt_hit | the record's material id, unchecked.  The winner's statement is evaluated once more for its point.
// Nothing accepted: position 0, the radius as given, u = v = 0, prim_id 0xFFFFFFFF, material 0.
RT_RULE void cp_answer_miss(float radius, uint32_t out[8]) {
    out[0] = out[1] = out[2] = 0u, out[3] = cp_bits(radius), out[4] = out[5] = 0u, out[6] = RT_PRIM_MISS, out[7] = 0u;
}
RT_RULE void cp_answer_triangle(const float q[9], uint32_t material_id, uint64_t order, const float p[3], uint32_t out[8]) {
    float v, w, pos[3];
    (void)cp_triangle(q, q + 3, q + 6, p, v, w);
    cp_triangle_position(q, q + 3, q + 6, v, w, pos);
    out[0] = cp_bits(pos[0]), out[1] = cp_bits(pos[1]), out[2] = cp_bits(pos[2]), out[3] = cp_bits(sqrtf(cp_best_dist2(order)));
    out[4] = cp_bits(v), out[5] = cp_bits(w), out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}
RT_RULE void cp_answer_sphere(const float centre[3], float radius, uint32_t material_id, uint64_t order, const float p[3], uint32_t out[8]) {
    float pos[3];
    (void)cp_sphere(centre, radius, p, pos);
    out[0] = cp_bits(pos[0]), out[1] = cp_bits(pos[1]), out[2] = cp_bits(pos[2]), out[3] = cp_bits(sqrtf(cp_best_dist2(order)));
    out[4] = out[5] = 0u, out[6] = (uint32_t)order ^ RT_PRIM_SPHERE_FLAG, out[7] = material_id;
}

} // namespace rt
#endif
