// closest_point_lane.h — how one lane of a closest-point kernel reads a node and a record and keeps its stack: what cp_walk
// (closest_point_rules.h, rule 5) asks of its caller, stated once for k_cp_nearest (closest_point.hip) and k_inside (inside.hip).
#ifndef RT_CLOSEST_POINT_LANE_H
#define RT_CLOSEST_POINT_LANE_H

#include "closest_point_rules.h"
#include "device_common.h"

namespace rtdev {

// What cp_walk (closest_point_rules.h, rule 5) asks of its caller, for one lane.
template <bool COUNT>
struct LaneAccess {
    const uint4* __restrict__ nodes;
    const DevTri* __restrict__ tris;
    uint2* stack; // lane-interleaved: entry k of this lane at stack[k * WAVE]; at most depth - 1 of the depth + 2 entries are in use (rule 5)
    Counts cnt;

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

} // namespace rtdev
#endif
