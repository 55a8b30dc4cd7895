// closest_point.hip — the kernel of the closest-point query of include/rt_hip.h (rt_closest_point): for each point the caller
// supplies, the nearest point of the scene's surface within the query's radius.
//
// Every statement that decides a bit of the answer is in closest_point_rules.h and the walk in group_walk.h, which the host check
// (tests/check_closest_point.cpp) runs against a brute force; query_lane.h, which every volume-query kernel shares, holds how a lane
// reads a node and a record and keeps its stack, and the lane's answer (cp_nearest_lane); this file supplies the output record.  One
// lane per point, one wave per block, the per-lane stack in LDS: the launch shape of k_rq_trace.
#include "closest_point.h"

#include "query_lane.h"

using namespace rtdev;

namespace {

// One rt_point_query (px py pz radius) per lane -> one rt_nearest (position | distance | u v | prim_id material_id).
template <bool COUNT>
__global__ __launch_bounds__(WAVE) void k_cp_nearest(DevScene sc, const float4* __restrict__ points, uint4* __restrict__ out, uint32_t n,
                                                      unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const float4 pq = points[i];
    const float p[3] = {pq.x, pq.y, pq.z};
    LaneAccess<COUNT> acc(sc, s_stack);
    uint32_t r[8];
    cp_nearest_lane(sc, acc, p, pq.w, r);
    out[2 * (size_t)i] = make_uint4(r[0], r[1], r[2], r[3]);
    out[2 * (size_t)i + 1] = make_uint4(r[4], r[5], r[6], r[7]);
    if (COUNT) flush_counts(counters, acc.cnt);
}

} // namespace

namespace rt {

hipError_t launch_closest_point(const DevScene& sc, const void* points, void* out, uint32_t n, unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = lane_stack_bytes(sc);
    const float4* p = reinterpret_cast<const float4*>(points);
    uint4* o = reinterpret_cast<uint4*>(out);
    if (counters) hipLaunchKernelGGL((k_cp_nearest<true>), grid, block, lds, stream, sc, p, o, n, counters);
    else hipLaunchKernelGGL((k_cp_nearest<false>), grid, block, lds, stream, sc, p, o, n, counters);
    return hipGetLastError();
}

} // namespace rt
