// query_lane.h — how one lane of a volume-query kernel reads a node and a record and keeps its stack and its list: the Access that
// group_walk (group_walk.h) asks of its caller, stated once for k_cp_nearest, k_cp_nearest_all, k_sweep_sphere, k_overlap_box,
// k_contact_capsule and k_inside; and the closest-point answer of one lane, which k_cp_nearest and k_inside share.
#ifndef RT_QUERY_LANE_H
#define RT_QUERY_LANE_H

#include "closest_point_rules.h"
#include "device_common.h"

namespace rtdev {

template <bool COUNT>
struct LaneAccess {
    const uint4* __restrict__ nodes;
    const DevTri* __restrict__ tris;
    uint2* stack; // lane-interleaved: entry k of this lane at stack[k * WAVE]; at most depth - 1 of the depth + 2 entries are in use (group_walk.h)
    Counts cnt;

    // the walk's access of a lane whose stack starts at s_stack; a null stack serves record() alone
    __device__ __forceinline__ LaneAccess(const DevScene& sc, uint2* s_stack)
        : nodes(reinterpret_cast<const uint4*>(sc.nodes)), tris(sc.tris), stack(s_stack ? s_stack + threadIdx.x : nullptr), cnt{0u, 0u} {}

    __device__ __forceinline__ void node(uint32_t idx, uint32_t w[20]) {
        const uint4* n = nodes + (size_t)idx * 5;
        const uint4 w0 = n[0], w1 = n[1], w2 = n[2], w3 = n[3], w4 = n[4]; // one visit = 5 x dwordx4, as visit_node8
        if (COUNT) cnt.nodes++;
        w[0] = w0.x, w[1] = w0.y, w[2] = w0.z, w[3] = w0.w;
        w[4] = w1.x, w[5] = w1.y, w[6] = w1.z, w[7] = w1.w;
        w[8] = w2.x, w[9] = w2.y, w[10] = w2.z, w[11] = w2.w;
        w[12] = w3.x, w[13] = w3.y, w[14] = w3.z, w[15] = w3.w;
        w[16] = w4.x, w[17] = w4.y, w[18] = w4.z, w[19] = w4.w;
    }
    __device__ __forceinline__ void record(uint32_t slot, float q[9], uint32_t ids[3]) {
        if (COUNT) cnt.tris++;
        const float4* p = reinterpret_cast<const float4*>(tris + slot);
        float4 q0 = p[0], q1 = p[1], q2 = p[2]; // the record in three loads issued together, as traverse_all
        asm volatile("" : "+v"(q0.x), "+v"(q0.y), "+v"(q0.z), "+v"(q0.w), "+v"(q1.x), "+v"(q1.y), "+v"(q1.z), "+v"(q1.w), "+v"(q2.x), "+v"(q2.y), "+v"(q2.z), "+v"(q2.w));
        q[0] = q0.x, q[1] = q0.y, q[2] = q0.z, q[3] = q0.w, q[4] = q1.x, q[5] = q1.y, q[6] = q1.z, q[7] = q1.w, q[8] = q2.x;
        ids[0] = __float_as_uint(q2.y), ids[1] = __float_as_uint(q2.z), ids[2] = __float_as_uint(q2.w);
    }
    __device__ __forceinline__ void push(int sp, uint32_t base, uint32_t bits) { stack[sp * WAVE] = make_uint2(base, bits); }
    __device__ __forceinline__ void pop(int sp, uint32_t& base, uint32_t& bits) {
        const uint2 e = stack[sp * WAVE];
        base = e.x, bits = e.y;
    }
};

// The lists live behind the launch's stack (lane_stack_entries), lane-interleaved like it.
// Nearest-K (closest_point_all_rules.h, rule 7; the contact query's list is the same): word f of entry k of this lane at
// list[(3 * k + f) * WAVE], k < max_nearest.
template <bool COUNT>
struct LaneListAccess : LaneAccess<COUNT> {
    uint32_t* list;

    __device__ __forceinline__ LaneListAccess(const DevScene& sc, uint2* s_stack)
        : LaneAccess<COUNT>(sc, s_stack), list(reinterpret_cast<uint32_t*>(s_stack + (size_t)lane_stack_entries(sc) * WAVE) + threadIdx.x) {}
    __device__ __forceinline__ void list_get(uint32_t k, uint32_t& d2, uint32_t& key, uint32_t& slot) const {
        d2 = list[(3u * k) * WAVE], key = list[(3u * k + 1u) * WAVE], slot = list[(3u * k + 2u) * WAVE];
    }
    __device__ __forceinline__ void list_set(uint32_t k, uint32_t d2, uint32_t key, uint32_t slot) {
        list[(3u * k) * WAVE] = d2, list[(3u * k + 1u) * WAVE] = key, list[(3u * k + 2u) * WAVE] = slot;
    }
};
// Overlap (overlap_rules.h, rule 4): entry k of this lane at list[k * WAVE], k < max_prims.
template <bool COUNT>
struct LaneKeyAccess : LaneAccess<COUNT> {
    uint32_t* list;

    __device__ __forceinline__ LaneKeyAccess(const DevScene& sc, uint2* s_stack)
        : LaneAccess<COUNT>(sc, s_stack), list(reinterpret_cast<uint32_t*>(s_stack + (size_t)lane_stack_entries(sc) * WAVE) + threadIdx.x) {}
    __device__ __forceinline__ uint32_t list_get(uint32_t k) const { return list[k * WAVE]; }
    __device__ __forceinline__ void list_set(uint32_t k, uint32_t key) { list[k * WAVE] = key; }
};

// One rt_point_query (p, radius) -> the eight words of its rt_nearest: the spheres by brute force in index order, cp_walk, and the
// winner's statement once more, uncounted, for its point.  A degenerate query is a miss without a walk.
template <bool COUNT>
__device__ __forceinline__ void cp_nearest_lane(const DevScene& sc, LaneAccess<COUNT>& acc, const float p[3], float radius, uint32_t r[8]) {
    rt::cp_answer_miss(radius, r);
    if (!rt::cp_query_valid(p, radius)) return;
    rt::CpBest best;
    best.order = rt::cp_start(radius);
    best.slot = 0xFFFFFFFFu;
    float pos[3];
    for (uint32_t s = 0; s < sc.n_spheres; s++) {
        const uint64_t c = rt::cp_order(rt::cp_sphere(sc.spheres[s].center, sc.spheres[s].radius, p, pos), s);
        if (c < best.order) best.order = c, best.slot = s;
    }
    rt::cp_walk(acc, sc.n_nodes, p, best);
    if (best.slot == 0xFFFFFFFFu) return;
    if ((uint32_t)best.order & RT_PRIM_SPHERE_FLAG) { // a triangle's key
        float q[9];
        uint32_t ids[3];
        LaneAccess<false>(sc, nullptr).record(best.slot, q, ids);
        rt::cp_answer_triangle(q, ids[0], best.order, p, r);
    } else {
        const DevSphere& s = sc.spheres[best.slot];
        rt::cp_answer_sphere(s.center, s.radius, s.material_id, best.order, p, r);
    }
}

} // namespace rtdev
#endif
