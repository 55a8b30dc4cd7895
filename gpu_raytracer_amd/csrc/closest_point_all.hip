// closest_point_all.hip — the kernel of the nearest-K query of include/rt_hip.h (rt_closest_point_all): for each point the caller
// supplies, the max_nearest nearest primitives of the scene within the query's radius, nearest first.
//
// Every statement that decides a bit of the answer and the list are in closest_point_rules.h and closest_point_all_rules.h and the
// walk in group_walk.h, which the host check (tests/check_closest_point_all.cpp) runs against a brute-force sort; how a lane reads a
// node and a record, its stack and where its list lives are LaneListAccess of query_lane.h; this file supplies the output records.
// One lane per point, one wave per block, the launch shape of k_cp_nearest; the per-lane stack in LDS and the list behind it, as
// k_rq_trace_all's HitList.
#include "closest_point_all.h"

#include "closest_point_all_rules.h"
#include "query_lane.h"

using namespace rtdev;

namespace {

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
    LaneListAccess<COUNT> acc(sc, s_stack);
    rt::CpList list;
    rt::cp_list_init(list, max_nearest < rt::CP_NEAREST_MAX ? max_nearest : rt::CP_NEAREST_MAX, pq.w); // the launch's list words hold no more
    if (rt::cp_query_valid(p, pq.w)) { // degenerate queries are misses without a walk
        float pos[3];
        for (uint32_t s = 0; s < sc.n_spheres; s++) // the spheres by brute force, in index order
            rt::cp_list_offer<COUNT_ALL>(acc, list, rt::cp_order(rt::cp_sphere(sc.spheres[s].center, sc.spheres[s].radius, p, pos), s), s);
        rt::cp_walk_all<COUNT_ALL>(acc, sc.n_nodes, p, list);
    }
    uint4* rec = out + 2 * (size_t)i * max_nearest;
    LaneAccess<false> plain(sc, nullptr); // the records once more, uncounted
    for (uint32_t k = 0; k < list.cap; k++) {
        uint32_t r[8];
        rt::cp_answer_miss(pq.w, r);
        if (k < list.n) {
            uint32_t d2, key, slot;
            acc.list_get(k, d2, key, slot);
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
    if (COUNT) flush_counts(counters, acc.cnt);
}

} // namespace

namespace rt {

hipError_t launch_closest_point_all(const DevScene& sc, const void* points, void* out, uint32_t* counts, uint32_t n, uint32_t max_nearest, bool count_all,
                                    unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (max_nearest > CP_NEAREST_MAX) return hipErrorInvalidValue;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = lane_stack_bytes(sc) + (size_t)max_nearest * 3u * WAVE * sizeof(uint32_t); // stack + list
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
