// closest_point_all_rules.h — the nearest-K query (rt_closest_point_all, include/rt_hip.h "Closest-point queries"), stated once.
//
// What closest_point_rules.h states for the single nearest primitive stays as it is and is used as it is: the candidate of a triangle
// and of a sphere, the order among candidates, the lower bound of a node's child boxes and the visiting order.
// This file adds the two things a collecting query needs: a sorted list of the K lowest candidates with the bound that follows from
// it, and the walk of cp_walk culled by that bound.  Two pieces of code call it: the kernel (closest_point_all.hip) and the host walk
// of tests/check_closest_point_all.cpp, which holds every record and count to a brute-force sort before any kernel runs.  The same
// RT_RULE convention: host and device under hipcc, host only elsewhere; every operation one f32 rounding.
#ifndef RT_CLOSEST_POINT_ALL_RULES_H
#define RT_CLOSEST_POINT_ALL_RULES_H

#include "closest_point_rules.h"

namespace rt {

// ---- 7. The list.  A lane's K lowest candidates in range so far, ascending by cp_order.  An entry is three words - the bits of
// dist2, the key, and the slot (the record's index in DevScene::tris, or the sphere index) - and lives where the caller's Access
// puts it:
//   void list_get(uint32_t k, uint32_t& d2, uint32_t& key, uint32_t& slot) / void list_set(uint32_t k, uint32_t d2, uint32_t key, uint32_t slot)
// with k < cap always (the host check verifies every index against the K the launch provides).
//   start  cp_start(radius): a candidate is IN RANGE iff its order is below it - rt_closest_point's acceptance, so dist2 < radius *
//          radius strictly, and a NaN or infinite dist2 never.
//   bound  a candidate ENTERS the list iff its order is below it: `start` until the list holds cap entries, its last entry's order
//          afterwards.  bound never rises, and bound <= start.
//   total  the candidates in range that were offered (kept under COUNT_ALL only).  Each primitive is offered once - a triangle has one
//          record (bvh_rules.h: no spatial splits; bvh_check.h placed_once) and a leaf one parent - so one that entered and was later
//          dropped has been counted once.
// With cap == 1 the list is cp_walk's CpBest: bound is best.order at every step.
struct CpList {
    uint64_t start, bound;
    uint32_t cap, n, total;
};
RT_RULE void cp_list_init(CpList& l, uint32_t cap, float radius) {
    l.start = l.bound = cp_start(radius);
    l.cap = cap;
    l.n = l.total = 0u;
}
// The dist2 a slot's lower bound L is held against: the slot is culled iff L > it, strictly (cp_pass), so a candidate that ties with
// the last entry's dist2 on a lower key is still reached and displaces it.  Every record under a culled slot has dist2 >= L > this,
// so its order is above `bound` now and, since bound never rises, for the rest of the walk: it could never have entered.  COUNT_ALL
// has to reach every candidate in range, so its walk is culled by `start` throughout.
template <bool COUNT_ALL>
RT_RULE float cp_list_cull(const CpList& l) {
    return cp_best_dist2(COUNT_ALL ? l.start : l.bound);
}
// Offers candidate c = cp_order(dist2, key) of `slot`.  Insertion moves the tail up one entry at a time from the end; a full list
// drops its last entry.
template <bool COUNT_ALL, class Access>
RT_RULE void cp_list_offer(Access& acc, CpList& l, uint64_t c, uint32_t slot) {
    if (COUNT_ALL) {
        if (!(c < l.start)) return;
        l.total++;
    }
    if (!(c < l.bound) || l.cap == 0u) return;
    uint32_t j = l.n < l.cap ? l.n : l.cap - 1u;
    while (j > 0u) {
        uint32_t pd, pk, ps;
        acc.list_get(j - 1u, pd, pk, ps);
        if (!(c < (((uint64_t)pd << 32) | pk))) break;
        acc.list_set(j, pd, pk, ps);
        j--;
    }
    acc.list_set(j, (uint32_t)(c >> 32), (uint32_t)c, slot);
    if (l.n < l.cap) l.n++;
    if (l.n == l.cap) {
        uint32_t pd, pk, ps;
        acc.list_get(l.cap - 1u, pd, pk, ps);
        l.bound = ((uint64_t)pd << 32) | pk;
    }
}
// what rt_closest_point_all reports in counts[i]
template <bool COUNT_ALL>
RT_RULE uint32_t cp_list_count(const CpList& l) {
    return COUNT_ALL ? l.total : l.n;
}

// ---- 8. The walk: group_walk (group_walk.h) with cp_walk's bound and order, every record offered to the list and both passes held
// against cp_list_cull instead of the best distance.
template <bool COUNT_ALL>
struct CpAllVisit {
    const float* p;
    float p_max, L[8];
    CpList& list;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        uint32_t code;
        cp_node_bounds(w, p, p_max, L, code);
        return code;
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return cp_pass(L, cp_list_cull<COUNT_ALL>(list), occupied); }
    template <class Access>
    RT_RULE bool leaf(Access& acc, uint32_t slot, const float q[9], const uint32_t ids[3]) {
        float v, wgt;
        cp_list_offer<COUNT_ALL>(acc, list, cp_order(cp_triangle(q, q + 3, q + 6, p, v, wgt), ids[1] ^ RT_PRIM_SPHERE_FLAG), slot);
        return false;
    }
};
template <bool COUNT_ALL, class Access>
RT_RULE void cp_walk_all(Access& acc, uint32_t n_nodes, const float p[3], CpList& list) {
    CpAllVisit<COUNT_ALL> v{p, cp_p_max(p), {}, list};
    group_walk(acc, n_nodes, v);
}

} // namespace rt
#endif
