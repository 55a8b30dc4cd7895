// closest_point.hip — the kernel of the closest-point query of include/rt_hip.h (rt_closest_point): for each point the caller
// supplies, the nearest point of the scene's surface within the query's radius.
//
// Every statement that decides a bit of the answer, and the walk itself, is in closest_point_rules.h, which the host check
// (tests/check_closest_point.cpp) runs against a brute force; this file supplies the output record, and
// closest_point_lane.h, which inside.hip shares, how a lane reads a node and a record and keeps its stack.  One lane per point, one
// wave per block, the per-lane stack in LDS: the launch shape of k_rq_trace.
#include "closest_point.h"

#include "closest_point_lane.h"
#include "closest_point_rules.h"
#include "device_common.h"

using namespace rtdev;

namespace {

// One rt_point_query (px py pz radius) per lane -> one rt_nearest (position | distance | u v | prim_id material_id).
template <bool COUNT>
__global__ __launch_bounds__(WAVE) void k_cp_nearest(DevScene sc, const float4* __restrict__ points, uint4* __restrict__ out, uint32_t n,
                                                      unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // (DevScene::stack_entries / 2 + 1) * 64 64-bit entries
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const float4 pq = points[i];
    const float p[3] = {pq.x, pq.y, pq.z};
    LaneAccess<COUNT> acc;
    acc.nodes = reinterpret_cast<const uint4*>(sc.nodes);
    acc.tris = sc.tris;
    acc.stack = s_stack + threadIdx.x;
    acc.cnt = {0u, 0u};
    uint32_t r[8];
    rt::cp_answer_miss(pq.w, r);
    if (rt::cp_query_valid(p, pq.w)) { // degenerate queries are misses without a walk
        rt::CpBest best;
        best.order = rt::cp_start(pq.w);
        best.slot = 0xFFFFFFFFu;
        float pos[3];
        for (uint32_t s = 0; s < sc.n_spheres; s++) { // the spheres by brute force, in index order
            const uint64_t c = rt::cp_order(rt::cp_sphere(sc.spheres[s].center, sc.spheres[s].radius, p, pos), s);
            if (c < best.order) best.order = c, best.slot = s;
        }
        rt::cp_walk(acc, sc.n_nodes, p, best);
        if (best.slot != 0xFFFFFFFFu) {
            if ((uint32_t)best.order & RT_PRIM_SPHERE_FLAG) { // a triangle's key
                float q[9];
                uint32_t ids[3];
                LaneAccess<false>{nullptr, sc.tris, nullptr, {0u, 0u}}.record(best.slot, q, ids);
                rt::cp_answer_triangle(q, ids[0], best.order, p, r);
            } else {
                const DevSphere& s = sc.spheres[best.slot];
                rt::cp_answer_sphere(s.center, s.radius, s.material_id, best.order, p, r);
            }
        }
    }
    out[2 * (size_t)i] = make_uint4(r[0], r[1], r[2], r[3]);
    out[2 * (size_t)i + 1] = make_uint4(r[4], r[5], r[6], r[7]);
    if (COUNT) {
        atomicAdd(&counters[RT_CNT_NODE_VISITS], (unsigned long long)acc.cnt.nodes);
        atomicAdd(&counters[RT_CNT_TRI_TESTS], (unsigned long long)acc.cnt.tris);
    }
}

} // namespace

namespace rt {

hipError_t launch_closest_point(const DevScene& sc, const void* points, void* out, uint32_t n, unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = (size_t)(sc.stack_entries / 2u + 1u) * WAVE * sizeof(uint2); // as launch_ray_query
    const float4* p = reinterpret_cast<const float4*>(points);
    uint4* o = reinterpret_cast<uint4*>(out);
    if (counters) hipLaunchKernelGGL((k_cp_nearest<true>), grid, block, lds, stream, sc, p, o, n, counters);
    else hipLaunchKernelGGL((k_cp_nearest<false>), grid, block, lds, stream, sc, p, o, n, counters);
    return hipGetLastError();
}

} // namespace rt
