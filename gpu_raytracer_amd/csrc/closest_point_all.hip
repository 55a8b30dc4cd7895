// closest_point_all.hip — the kernel of the nearest-K query of include/rt_hip.h (rt_closest_point_all): for each point the caller
// supplies, the max_nearest nearest primitives of the scene within the query's radius, nearest first.
//
// Every statement that decides a bit of the answer, the list and the walk are in closest_point_rules.h and
// closest_point_all_rules.h, which the host check (tests/check_closest_point_all.cpp) runs against a brute-force sort; this file
// supplies how a lane reads a node and a record, its stack, where its list lives and the output records.  One lane per point, one wave
// per block, the launch shape of k_cp_nearest; the per-lane stack in LDS and the list behind it, as k_rq_trace_all's HitList.
#include "closest_point_all.h"

#include "closest_point_all_rules.h"
#include "device_common.h"

using namespace rtdev;

namespace {

// What cp_walk_all (closest_point_all_rules.h, rule 8) asks of its caller, for one lane: LaneAccess of closest_point.hip and the list.
template <bool COUNT>
struct LaneListAccess {
    const uint4* __restrict__ nodes;
    const DevTri* __restrict__ tris;
    uint2* stack;   // lane-interleaved: entry k of this lane at stack[k * WAVE]; at most depth - 1 of the depth + 2 entries are in use (rule 5)
    uint32_t* list; // lane-interleaved: word f of entry k of this lane at list[(3 * k + f) * WAVE], k < max_nearest (rule 7)
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
    __device__ __forceinline__ void list_get(uint32_t k, uint32_t& d2, uint32_t& key, uint32_t& slot) const {
        d2 = list[(3u * k) * WAVE], key = list[(3u * k + 1u) * WAVE], slot = list[(3u * k + 2u) * WAVE];
    }
    __device__ __forceinline__ void list_set(uint32_t k, uint32_t d2, uint32_t key, uint32_t slot) {
        list[(3u * k) * WAVE] = d2, list[(3u * k + 1u) * WAVE] = key, list[(3u * k + 2u) * WAVE] = slot;
    }
};

// One rt_point_query (px py pz radius) per lane -> max_nearest rt_nearest records at out[i * max_nearest ..] (the listed primitives,
// then misses) and, counts != null, counts[i] = the records listed, or COUNT_ALL: all candidates in range.  max_nearest == 0
// (COUNT_ALL only): `out` is not touched.
template <bool COUNT, bool COUNT_ALL>
__global__ __launch_bounds__(WAVE) void k_cp_nearest_all(DevScene sc, const float4* __restrict__ points, uint4* __restrict__ out,
                                                          uint32_t* __restrict__ counts, uint32_t n, uint32_t max_nearest,
                                                          unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // the stack of k_cp_nearest, then 3 * max_nearest * 64 list words
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const float4 pq = points[i];
    const float p[3] = {pq.x, pq.y, pq.z};
    LaneListAccess<COUNT> acc;
    acc.nodes = reinterpret_cast<const uint4*>(sc.nodes);
    acc.tris = sc.tris;
    acc.stack = s_stack + threadIdx.x;
    acc.list = reinterpret_cast<uint32_t*>(s_stack + (size_t)(sc.stack_entries / 2u + 1u) * WAVE) + threadIdx.x;
    acc.cnt = {0u, 0u};
    rt::CpList list;
    rt::cp_list_init(list, max_nearest < rt::CP_NEAREST_MAX ? max_nearest : rt::CP_NEAREST_MAX, pq.w); // the launch's list words hold no more
    if (rt::cp_query_valid(p, pq.w)) { // degenerate queries are misses without a walk
        float pos[3];
        for (uint32_t s = 0; s < sc.n_spheres; s++) // the spheres by brute force, in index order
            rt::cp_list_offer<COUNT_ALL>(acc, list, rt::cp_order(rt::cp_sphere(sc.spheres[s].center, sc.spheres[s].radius, p, pos), s), s);
        rt::cp_walk_all<COUNT_ALL>(acc, sc.n_nodes, p, list);
    }
    uint4* rec = out + 2 * (size_t)i * max_nearest;
    LaneListAccess<false> plain{nullptr, sc.tris, nullptr, acc.list, {0u, 0u}}; // the records once more, uncounted
    for (uint32_t k = 0; k < list.cap; k++) {
        uint32_t r[8];
        rt::cp_answer_miss(pq.w, r);
        if (k < list.n) {
            uint32_t d2, key, slot;
            plain.list_get(k, d2, key, slot);
            const uint64_t order = ((uint64_t)d2 << 32) | key;
            if (key & RT_PRIM_SPHERE_FLAG) { // a triangle's key
                float q[9];
                uint32_t ids[3];
                plain.record(slot, q, ids);
                rt::cp_answer_triangle(q, ids[0], order, p, r);
            } else {
                const DevSphere& s = sc.spheres[slot];
                rt::cp_answer_sphere(s.center, s.radius, s.material_id, order, p, r);
            }
        }
        rec[2 * k] = make_uint4(r[0], r[1], r[2], r[3]);
        rec[2 * k + 1] = make_uint4(r[4], r[5], r[6], r[7]);
    }
    if (counts) counts[i] = rt::cp_list_count<COUNT_ALL>(list);
    if (COUNT) {
        atomicAdd(&counters[RT_CNT_NODE_VISITS], (unsigned long long)acc.cnt.nodes);
        atomicAdd(&counters[RT_CNT_TRI_TESTS], (unsigned long long)acc.cnt.tris);
    }
}

} // namespace

namespace rt {

hipError_t launch_closest_point_all(const DevScene& sc, const void* points, void* out, uint32_t* counts, uint32_t n, uint32_t max_nearest, bool count_all,
                                    unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (max_nearest > CP_NEAREST_MAX) return hipErrorInvalidValue;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = (size_t)(sc.stack_entries / 2u + 1u) * WAVE * sizeof(uint2) + (size_t)max_nearest * 3u * WAVE * sizeof(uint32_t); // stack + list
    const float4* p = reinterpret_cast<const float4*>(points);
    uint4* o = reinterpret_cast<uint4*>(out);
    if (count_all) {
        if (counters) hipLaunchKernelGGL((k_cp_nearest_all<true, true>), grid, block, lds, stream, sc, p, o, counts, n, max_nearest, counters);
        else hipLaunchKernelGGL((k_cp_nearest_all<false, true>), grid, block, lds, stream, sc, p, o, counts, n, max_nearest, counters);
    } else {
        if (counters) hipLaunchKernelGGL((k_cp_nearest_all<true, false>), grid, block, lds, stream, sc, p, o, counts, n, max_nearest, counters);
        else hipLaunchKernelGGL((k_cp_nearest_all<false, false>), grid, block, lds, stream, sc, p, o, counts, n, max_nearest, counters);
    }
    return hipGetLastError();
}

} // namespace rt
