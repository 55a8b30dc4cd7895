// overlap_triangle.hip — the kernel of the triangle query of include/rt_hip.h (rt_overlap_triangle): for each triangle the caller
// supplies, the primitives of the scene that touch it - their ids, their number, or only whether there is one.
//
// Every statement that decides a bit of the answer is in overlap_triangle_rules.h (the pair test; the list and the node test are
// overlap_rules.h's) and the walk in group_walk.h, which the host check (tests/check_overlap_triangle.cpp) runs against a brute force
// over all primitives; how a lane reads a node and a record, its stack and where its list lives are LaneKeyAccess of query_lane.h;
// this file supplies the output words.  The launch shape of k_overlap_box: one lane per query, one wave per block, the per-lane
// stack in LDS and the list's max_prims words per lane behind it.  A lane keeps q0, u1, u2 and the bounds; the in-plane axes are
// computed again for every pair that passes the bounds.
#include "overlap_triangle.h"

#include "overlap_triangle_rules.h"
#include "query_lane.h"

using namespace rtdev;

namespace {

// One rt_query_triangle (v0, pad | v1, pad | v2, pad) per lane -> k_overlap_box's outputs.
template <bool COUNT, int MODE>
__global__ __launch_bounds__(WAVE) void k_overlap_triangle(DevScene sc, const float4* __restrict__ triangles, uint32_t* __restrict__ prims,
                                                            uint32_t* __restrict__ counts, uint32_t n, uint32_t max_prims,
                                                            unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // the stack of k_cp_nearest, then max_prims * 64 list words
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const float4 t0 = triangles[3 * (size_t)i], t1 = triangles[3 * (size_t)i + 1], t2 = triangles[3 * (size_t)i + 2];
    const float q0[3] = {t0.x, t0.y, t0.z}, q1[3] = {t1.x, t1.y, t1.z}, q2[3] = {t2.x, t2.y, t2.z};
    LaneKeyAccess<COUNT> acc(sc, s_stack);
    rt::OvList list;
    rt::ov_list_init(list, MODE == rt::OV_ANY ? 0u : (max_prims < rt::OV_PRIMS_MAX ? max_prims : rt::OV_PRIMS_MAX)); // the launch's list words hold no more
    if (rt::ot_query_valid(q0, q1, q2)) { // a non-finite query touches nothing, without a walk
        rt::OtQuery q;
        rt::ot_query_init(q, q0, q1, q2);
        for (uint32_t s = 0; s < sc.n_spheres; s++) { // the spheres by brute force, in index order
            if (MODE == rt::OV_ANY && list.total) break;
            if (rt::ov_list_wants<MODE>(list, s) && rt::ot_sphere(sc.spheres[s].center, sc.spheres[s].radius, q)) rt::ov_list_offer(acc, list, s);
        }
        if (MODE != rt::OV_ANY || list.total == 0u) rt::ot_walk<MODE>(acc, sc.n_nodes, q, list);
    }
    uint32_t* ids = prims + (size_t)i * max_prims;
    for (uint32_t k = 0; k < list.cap; k++) ids[k] = k < list.n ? (acc.list_get(k) ^ RT_PRIM_SPHERE_FLAG) : RT_PRIM_MISS;
    if (counts) counts[i] = rt::ov_list_count<MODE>(list);
    if (COUNT) flush_counts(counters, acc.cnt);
}

template <int MODE>
void launch_mode(const DevScene& sc, const float4* triangles, uint32_t* prims, uint32_t* counts, uint32_t n, uint32_t max_prims, size_t lds,
                 unsigned long long* counters, hipStream_t stream) {
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    if (counters) hipLaunchKernelGGL((k_overlap_triangle<true, MODE>), grid, block, lds, stream, sc, triangles, prims, counts, n, max_prims, counters);
    else hipLaunchKernelGGL((k_overlap_triangle<false, MODE>), grid, block, lds, stream, sc, triangles, prims, counts, n, max_prims, counters);
}

} // namespace

namespace rt {

hipError_t launch_overlap_triangle(const DevScene& sc, const void* triangles, uint32_t* prims, uint32_t* counts, uint32_t n, uint32_t max_prims,
                                   int mode, unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (max_prims > OV_PRIMS_MAX || (mode == OV_ANY && max_prims != 0u) || (max_prims != 0u && !prims)) return hipErrorInvalidValue;
    const size_t lds = lane_stack_bytes(sc) + (size_t)max_prims * WAVE * sizeof(uint32_t); // stack + list
    const float4* t = reinterpret_cast<const float4*>(triangles);
    switch (mode) {
    case OV_LIST: launch_mode<OV_LIST>(sc, t, prims, counts, n, max_prims, lds, counters, stream); break;
    case OV_COUNT_ALL: launch_mode<OV_COUNT_ALL>(sc, t, prims, counts, n, max_prims, lds, counters, stream); break;
    case OV_ANY: launch_mode<OV_ANY>(sc, t, prims, counts, n, max_prims, lds, counters, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace rt
