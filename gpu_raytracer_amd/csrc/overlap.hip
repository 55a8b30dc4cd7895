// overlap.hip — the kernel of the overlap query of include/rt_hip.h (rt_overlap_box): for each axis-aligned box the caller supplies,
// the primitives of the scene that touch it - their ids, their number, or only whether there is one.
//
// Every statement that decides a bit of the answer, the list and the walk are in overlap_rules.h, which the host check
// (tests/check_overlap.cpp) runs against a brute force over all primitives; this file supplies how a lane reads a node and a record,
// its stack, where its list lives and the output words.  One lane per box, one wave per block, the launch shape of k_cp_nearest_all;
// the per-lane stack in LDS and the list's max_prims words per lane behind it.
#include "overlap.h"

#include "device_common.h"
#include "overlap_rules.h"

using namespace rtdev;

namespace {

// What ov_walk (overlap_rules.h, rule 6) asks of its caller, for one lane: LaneListAccess of closest_point_all.hip with one-word entries.
template <bool COUNT>
struct LaneKeyAccess {
    const uint4* __restrict__ nodes;
    const DevTri* __restrict__ tris;
    uint2* stack;   // lane-interleaved: entry k of this lane at stack[k * WAVE]; at most depth - 1 of the depth + 2 entries are in use
    uint32_t* list; // lane-interleaved: entry k of this lane at list[k * WAVE], k < max_prims (rule 4)
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
        float4 q0 = p[0], q1 = p[1], q2 = p[2]; // the record in three loads issued together, as closest_point_all.hip
        asm volatile("" : "+v"(q0.x), "+v"(q0.y), "+v"(q0.z), "+v"(q0.w), "+v"(q1.x), "+v"(q1.y), "+v"(q1.z), "+v"(q1.w), "+v"(q2.x), "+v"(q2.y), "+v"(q2.z), "+v"(q2.w));
        q[0] = q0.x, q[1] = q0.y, q[2] = q0.z, q[3] = q0.w, q[4] = q1.x, q[5] = q1.y, q[6] = q1.z, q[7] = q1.w, q[8] = q2.x;
        ids[0] = __float_as_uint(q2.y), ids[1] = __float_as_uint(q2.z), ids[2] = __float_as_uint(q2.w);
    }
    __device__ __forceinline__ void push(int sp, uint32_t base, uint32_t bits) { stack[sp * WAVE] = make_uint2(base, bits); }
    __device__ __forceinline__ void pop(int sp, uint32_t& base, uint32_t& bits) {
        const uint2 e = stack[sp * WAVE];
        base = e.x, bits = e.y;
    }
    __device__ __forceinline__ uint32_t list_get(uint32_t k) const { return list[k * WAVE]; }
    __device__ __forceinline__ void list_set(uint32_t k, uint32_t key) { list[k * WAVE] = key; }
};

// One rt_box (centre, pad, half extent, pad) per lane -> max_prims ids at prims[i * max_prims ..] (the listed primitives, ascending in
// their key, then 0xFFFFFFFF) and, counts != null, counts[i] = ov_list_count.  max_prims == 0: `prims` is not touched.
template <bool COUNT, int MODE>
__global__ __launch_bounds__(WAVE) void k_overlap_box(DevScene sc, const float4* __restrict__ boxes, uint32_t* __restrict__ prims,
                                                       uint32_t* __restrict__ counts, uint32_t n, uint32_t max_prims,
                                                       unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // the stack of k_cp_nearest, then max_prims * 64 list words
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const float4 bc = boxes[2 * (size_t)i], bh = boxes[2 * (size_t)i + 1];
    const float c[3] = {bc.x, bc.y, bc.z}, h[3] = {bh.x, bh.y, bh.z};
    LaneKeyAccess<COUNT> acc;
    acc.nodes = reinterpret_cast<const uint4*>(sc.nodes);
    acc.tris = sc.tris;
    acc.stack = s_stack + threadIdx.x;
    acc.list = reinterpret_cast<uint32_t*>(s_stack + (size_t)(sc.stack_entries / 2u + 1u) * WAVE) + threadIdx.x;
    acc.cnt = {0u, 0u};
    rt::OvList list;
    rt::ov_list_init(list, MODE == rt::OV_ANY ? 0u : (max_prims < rt::OV_PRIMS_MAX ? max_prims : rt::OV_PRIMS_MAX)); // the launch's list words hold no more
    if (rt::ov_query_valid(c, h)) { // degenerate queries touch nothing, without a walk
        rt::OvBox box;
        rt::ov_box_init(box, c, h);
        for (uint32_t s = 0; s < sc.n_spheres; s++) { // the spheres by brute force, in index order
            if (MODE == rt::OV_ANY && list.total) break;
            if (rt::ov_list_wants<MODE>(list, s) && rt::ov_sphere(sc.spheres[s].center, sc.spheres[s].radius, c, h)) rt::ov_list_offer(acc, list, s);
        }
        if (MODE != rt::OV_ANY || list.total == 0u) rt::ov_walk<MODE>(acc, sc.n_nodes, box, list);
    }
    uint32_t* ids = prims + (size_t)i * max_prims;
    for (uint32_t k = 0; k < list.cap; k++) ids[k] = k < list.n ? (acc.list_get(k) ^ RT_PRIM_SPHERE_FLAG) : RT_PRIM_MISS;
    if (counts) counts[i] = rt::ov_list_count<MODE>(list);
    if (COUNT) {
        atomicAdd(&counters[RT_CNT_NODE_VISITS], (unsigned long long)acc.cnt.nodes);
        atomicAdd(&counters[RT_CNT_TRI_TESTS], (unsigned long long)acc.cnt.tris);
    }
}

template <int MODE>
void launch_mode(const DevScene& sc, const float4* boxes, uint32_t* prims, uint32_t* counts, uint32_t n, uint32_t max_prims, size_t lds,
                 unsigned long long* counters, hipStream_t stream) {
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    if (counters) hipLaunchKernelGGL((k_overlap_box<true, MODE>), grid, block, lds, stream, sc, boxes, prims, counts, n, max_prims, counters);
    else hipLaunchKernelGGL((k_overlap_box<false, MODE>), grid, block, lds, stream, sc, boxes, prims, counts, n, max_prims, counters);
}

} // namespace

namespace rt {

hipError_t launch_overlap_box(const DevScene& sc, const void* boxes, uint32_t* prims, uint32_t* counts, uint32_t n, uint32_t max_prims, int mode,
                              unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (max_prims > OV_PRIMS_MAX || (mode == OV_ANY && max_prims != 0u) || (max_prims != 0u && !prims)) return hipErrorInvalidValue;
    const size_t lds = (size_t)(sc.stack_entries / 2u + 1u) * WAVE * sizeof(uint2) + (size_t)max_prims * WAVE * sizeof(uint32_t); // stack + list
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
