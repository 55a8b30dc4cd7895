// closest_point_all_rules.h — the nearest-K query (rt_closest_point_all, include/rt_hip.h "Closest-point queries"), stated once.
//
// What closest_point_rules.h states for the single nearest primitive stays as it is and is used as it is: the candidate of a triangle
// and of a sphere, the order among candidates, the lower bound of a node's child boxes, the visiting order and the stack discipline.
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

// ---- 8. The walk: cp_walk's loop (rule 5) - the same groups, cp_node_bounds / cp_pass / cp_first_slot, one stack entry per visit at
// most, the same clamp of a leaf's length - with every record offered to the list and both cp_pass calls held against cp_list_cull
// instead of the best distance.  The stack bound of rule 5 does not depend on what culls, so it holds here unchanged.
template <bool COUNT_ALL, class Access>
RT_RULE void cp_walk_all(Access& acc, uint32_t n_nodes, const float p[3], CpList& list) {
    if (n_nodes == 0u) return;
    const float p_max = cp_p_max(p);
    uint32_t g_base = 0u, g_bits = 1u | (1u << 8); // the root as the only child of a group
    int sp = 0;
    for (;;) {
        if ((g_bits & 0xFFu) == 0u) {
            if (sp == 0) break;
            sp--;
            acc.pop(sp, g_base, g_bits);
        }
        const uint32_t i = cp_first_slot(g_bits, (g_bits >> 16) & 7u);
        g_bits ^= 1u << i;
        const uint32_t idx = g_base + cp_popc((g_bits >> 8) & ((1u << i) - 1u)); // inner slots below i
        if (g_bits & 0xFFu) {
            acc.push(sp, g_base, g_bits);
            sp++;
        }
        uint32_t w[20], code;
        float L[8];
        acc.node(idx, w);
        cp_node_bounds(w, p, p_max, L, code);
        const uint32_t imask = w[3] >> 24, lmask = w[6] & 0xFFu;
        uint32_t t = cp_pass(L, cp_list_cull<COUNT_ALL>(list), lmask);
        while (t) {
            const uint32_t sl = cp_first_slot(t, code);
            t ^= 1u << sl;
            const uint32_t first = w[5] + RT_DEV_LEAF_STRIDE * cp_popc(lmask & ((1u << sl) - 1u));
            uint32_t len = 1u;
            for (uint32_t x = 0; x < len; x++) {
                float q[9], v, wgt;
                uint32_t ids[3];
                acc.record(first + x, q, ids);
                if (x == 0u) len = ids[2] < RT_DEV_LEAF_STRIDE ? ids[2] : RT_DEV_LEAF_STRIDE; // 1..4; never past the leaf's own records
                cp_list_offer<COUNT_ALL>(acc, list, cp_order(cp_triangle(q, q + 3, q + 6, p, v, wgt), ids[1] ^ RT_PRIM_SPHERE_FLAG), first + x);
            }
        }
        g_base = w[4];
        g_bits = cp_pass(L, cp_list_cull<COUNT_ALL>(list), imask) | (imask << 8) | (code << 16); // by the bound the leaves left
    }
}

} // namespace rt
#endif
