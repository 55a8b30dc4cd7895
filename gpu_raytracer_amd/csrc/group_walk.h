// group_walk.h — the walk of the wide BVH that the volume queries share (closest point, nearest-K, the sweeps, box overlap, contact), stated
// once: the groups, the stack discipline with its bound, and the loop.  What differs between the queries - the bound of a node's child
// boxes, which slots pass it, what is done with a record - is a Visit, stated in the query's own rules header next to the statements
// it calls (CpVisit, CpAllVisit, SwVisit, OvVisit, CcVisit).
//
// The convention of every rules header: plain inline functions under RT_RULE (bvh_rules.h) - host and device under hipcc, host only
// under any other compiler - so the kernel and the host check (tests/check_*.cpp) run the same statements; loops over slots and axes
// carry RT_CP_UNROLL so that the per-slot arrays stay in registers on the device.
#ifndef RT_GROUP_WALK_H
#define RT_GROUP_WALK_H

#include <cstdint>

#include "bvh_rules.h"

#ifdef __HIPCC__
#define RT_CP_UNROLL _Pragma("unroll")
#else
#define RT_CP_UNROLL
#endif

namespace rt {

// The set slot of the 8-bit mask m (!= 0) with the smallest (slot XOR code): first_slot of device_common.h.
RT_RULE uint32_t cp_first_slot(uint32_t m, uint32_t code) {
    uint32_t q = m & 0xFFu;
    if (code & 1u) q = ((q & 0x55u) << 1) | ((q >> 1) & 0x55u);
    if (code & 2u) q = ((q & 0x33u) << 2) | ((q >> 2) & 0x33u);
    if (code & 4u) q = ((q & 0x0Fu) << 4) | (q >> 4);
    return (uint32_t)__builtin_ctz(q) ^ code;
}
RT_RULE uint32_t cp_popc(uint32_t x) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}

// The walk.  An Access supplies how a node and a record are read, the stack and the counters (query_lane.h for a lane of a kernel,
// tests/host_access.h for the host checks, which verify every index):
//   node(idx, w[20])              the words of node idx (the DevNode8), and one node visit
//   record(slot, q[9], ids[3])    v0 e1 e2 | material_id, prim_id, leaf_count of record `slot`, and one test
//   push(sp, base, bits) / pop(sp, base&, bits&)      entry sp of the lane's stack
// A Visit supplies the query:
//   uint32_t enter(const uint32_t w[20])     the bound of the node's eight child boxes, into the visitor's own state; returns the
//                                            node's code (bits 0..2), the order in which its slots are visited
//   uint32_t pass(uint32_t occupied)         the slots of `occupied` (lmask or imask: empty slots are inverted boxes and must never
//                                            be followed) that the current bound leaves to visit
//   bool leaf(acc, slot, q, ids)             tests record `slot` and keeps or offers it; true ends the walk
// A GROUP is what is left of a node's inner children: g_base = the node's child_base, g_bits = the slots still to visit (bits 0..7),
// the node's imask (bits 8..15) and the node's code (bits 16..18), so that a group taken off the stack keeps its order: its slots are
// visited in increasing (slot XOR code).  A visit takes one slot off the current group, parks the rest if any is left - AT MOST ONE
// ENTRY PER VISIT - then tests the node's leaves that pass the bound, in the same order; then its inner children that pass the bound
// the leaves left become the current group.  A parked child that has since fallen outside the bound costs one node visit and is
// culled there.  A leaf starts at the node's tri_base + RT_DEV_LEAF_STRIDE * (the leaf slots below it) and its first record says how
// many of its records are triangles.
// Stack: entries are only added on the way down, one per level at most, and the level that holds the deepest inner nodes parks
// nothing below it, so a tree of `depth` inner levels holds at most depth - 1 entries at a time: inside the depth + 2 =
// DevScene::stack_entries / 2 + 1 entries the query kernels give a lane (lane_stack_entries, device_common.h).  The bound does not
// depend on what culls or on the order of the slots, so it holds for every Visit.
template <class Access, class Visit>
RT_RULE void group_walk(Access& acc, uint32_t n_nodes, Visit& v) {
    if (n_nodes == 0u) return;
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
        uint32_t w[20];
        acc.node(idx, w);
        const uint32_t code = v.enter(w);
        const uint32_t imask = w[3] >> 24, lmask = w[6] & 0xFFu;
        uint32_t t = v.pass(lmask);
        while (t) {
            const uint32_t sl = cp_first_slot(t, code);
            t ^= 1u << sl;
            const uint32_t first = w[5] + RT_DEV_LEAF_STRIDE * cp_popc(lmask & ((1u << sl) - 1u));
            uint32_t len = 1u;
            for (uint32_t x = 0; x < len; x++) {
                float q[9];
                uint32_t ids[3];
                acc.record(first + x, q, ids);
                if (x == 0u) len = ids[2] < RT_DEV_LEAF_STRIDE ? ids[2] : RT_DEV_LEAF_STRIDE; // 1..4; never past the leaf's own records
                if (v.leaf(acc, first + x, q, ids)) return;
            }
        }
        g_base = w[4];
        g_bits = v.pass(imask) | (imask << 8) | (code << 16); // by the bound the leaves left
    }
}

} // namespace rt
#endif
