// inside_rules.h — the inside test and the signed distance (rt_inside, rt_signed_distance, include/rt_hip.h "Inside tests and signed
// distance"), stated once: the directions of the parity rays, sphere containment, the stop rule and the majority, and the signing of
// an rt_nearest record.  What a vote counts is the walk of multi_hit_walk.h (traverse_all with a list of capacity 0), and the
// magnitude is the walk of closest_point_rules.h; nothing of either is restated here.  Plain inline functions under the RT_RULE
// convention of bvh_rules.h: host and device under hipcc, host only under any other compiler.  Every operation is one f32 rounding, so
// numpy reproduces the bits (tests/signed_distance_cases.py).
#ifndef RT_INSIDE_RULES_H
#define RT_INSIDE_RULES_H

#include <cstdint>

#include "../../include/rt_hip.h"
#include "closest_point_rules.h"

namespace rt {

// ---- 1. The directions: the header's table, used as given.  Vote k of a point is taken along direction k.
RT_RULE void inside_direction(uint32_t k, float d[3]) {
    constexpr float table[RT_INSIDE_MAX_RAYS][3] = {RT_INSIDE_DIRECTIONS};
    d[0] = table[k][0], d[1] = table[k][1], d[2] = table[k][2];
}
// R is one of 1, 3, 5, 7
RT_RULE bool inside_rays_valid(uint32_t rays) { return rays <= RT_INSIDE_MAX_RAYS && (rays & 1u) != 0u; }

// ---- 2. A query that traces nothing: a non-finite position component.  (rt_signed_distance asks cp_query_valid instead, which
// holds the radius to rt_closest_point's rules as well.)
RT_RULE bool inside_query_valid(const float p[3]) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// ---- 3. Sphere containment: strictly inside, by the squared distance of the closest-point statement's dot.
RT_RULE bool inside_sphere(const float centre[3], float radius, const float p[3]) {
    const float oc[3] = {p[0] - centre[0], p[1] - centre[1], p[2] - centre[2]};
    return cp_dot(oc, oc) < radius * radius;
}

// ---- 4. The stop rule and the majority.  odd / even: the votes taken so far of R.  A majority once reached cannot change, so a
// point whose votes are not asked for stops there.
RT_RULE bool inside_decided(uint32_t odd, uint32_t even, uint32_t rays) { return odd * 2u > rays || even * 2u > rays; }
RT_RULE bool inside_majority(uint32_t odd, uint32_t rays) { return odd * 2u > rays; }

// ---- 5. The signed record: rt_closest_point's eight words, the sign bit of the distance set when the point is inside - on a miss
// within the radius too (-radius: the truncated field).
RT_RULE void inside_sign(uint32_t r[8], bool inside) {
    if (inside) r[3] |= 0x80000000u;
}

} // namespace rt
#endif
