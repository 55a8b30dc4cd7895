// overlap_obb.hip — the kernel of the oriented overlap query of include/rt_hip.h (rt_overlap_obb): for each oriented box the caller
// supplies, the primitives of the scene that touch it - their ids, their number, or only whether there is one.
//
// Every statement that decides a bit of the answer is in obb_rules.h (the frame; what happens in it is overlap_rules.h) and the walk
// in group_walk.h, which the host check (tests/check_obb.cpp) runs against a brute force over all primitives; how a lane reads a node
// and a record, its stack and where its list lives are LaneKeyAccess of query_lane.h; this file supplies the output words.  The
// launch shape of k_overlap_box: one lane per box, one wave per block, the per-lane stack in LDS and the list's max_prims words per
// lane behind it.  The frame's nine floats are computed once per query and stay in registers.
#include "overlap_obb.h"

#include "obb_rules.h"
#include "query_lane.h"

using namespace rtdev;

namespace {

// One rt_obb (centre, pad | half extent, pad | rotation) per lane -> k_overlap_box's outputs.
template <bool COUNT, int MODE>
__global__ __launch_bounds__(WAVE) void k_overlap_obb(DevScene sc, const float4* __restrict__ boxes, uint32_t* __restrict__ prims,
                                                       uint32_t* __restrict__ counts, uint32_t n, uint32_t max_prims,
                                                       unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // the stack of k_cp_nearest, then max_prims * 64 list words
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const float4 bc = boxes[3 * (size_t)i], bh = boxes[3 * (size_t)i + 1], bq = boxes[3 * (size_t)i + 2];
    const float c[3] = {bc.x, bc.y, bc.z}, h[3] = {bh.x, bh.y, bh.z}, q[4] = {bq.x, bq.y, bq.z, bq.w};
    LaneKeyAccess<COUNT> acc(sc, s_stack);
    rt::OvList list;
    rt::ov_list_init(list, MODE == rt::OV_ANY ? 0u : (max_prims < rt::OV_PRIMS_MAX ? max_prims : rt::OV_PRIMS_MAX)); // the launch's list words hold no more
    rt::ObBox box;
    if (rt::ob_query_valid(c, h, q, box.R)) { // degenerate queries touch nothing, without a walk
        rt::ob_box_init(box, c, h);
        for (uint32_t s = 0; s < sc.n_spheres; s++) { // the spheres by brute force, in index order
            if (MODE == rt::OV_ANY && list.total) break;
            if (rt::ov_list_wants<MODE>(list, s) && rt::ob_sphere(sc.spheres[s].center, sc.spheres[s].radius, box)) rt::ov_list_offer(acc, list, s);
        }
        if (MODE != rt::OV_ANY || list.total == 0u) rt::ob_walk<MODE>(acc, sc.n_nodes, box, list);
    }
    uint32_t* ids = prims + (size_t)i * max_prims;
    for (uint32_t k = 0; k < list.cap; k++) ids[k] = k < list.n ? (acc.list_get(k) ^ RT_PRIM_SPHERE_FLAG) : RT_PRIM_MISS;
    if (counts) counts[i] = rt::ov_list_count<MODE>(list);
    if (COUNT) flush_counts(counters, acc.cnt);
}

template <int MODE>
void launch_mode(const DevScene& sc, const float4* boxes, uint32_t* prims, uint32_t* counts, uint32_t n, uint32_t max_prims, size_t lds,
                 unsigned long long* counters, hipStream_t stream) {
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    if (counters) hipLaunchKernelGGL((k_overlap_obb<true, MODE>), grid, block, lds, stream, sc, boxes, prims, counts, n, max_prims, counters);
    else hipLaunchKernelGGL((k_overlap_obb<false, MODE>), grid, block, lds, stream, sc, boxes, prims, counts, n, max_prims, counters);
}

} // namespace

namespace rt {

hipError_t launch_overlap_obb(const DevScene& sc, const void* boxes, uint32_t* prims, uint32_t* counts, uint32_t n, uint32_t max_prims, int mode,
                              unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (max_prims > OV_PRIMS_MAX || (mode == OV_ANY && max_prims != 0u) || (max_prims != 0u && !prims)) return hipErrorInvalidValue;
    const size_t lds = lane_stack_bytes(sc) + (size_t)max_prims * WAVE * sizeof(uint32_t); // stack + list
    const float4* b = reinterpret_cast<const float4*>(boxes);
    switch (mode) {
    case OV_LIST: launch_mode<OV_LIST>(sc, b, prims, counts, n, max_prims, lds, counters, stream); break;
    case OV_COUNT_ALL: launch_mode<OV_COUNT_ALL>(sc, b, prims, counts, n, max_prims, lds, counters, stream); break;
    case OV_ANY: launch_mode<OV_ANY>(sc, b, prims, counts, n, max_prims, lds, counters, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace rt
