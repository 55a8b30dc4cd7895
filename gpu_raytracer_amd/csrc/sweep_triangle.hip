// sweep_triangle.hip — the kernel of the triangle sweep of include/rt_hip.h (rt_sweep_triangle): for each moving triangle the caller
// supplies, the time, the normal and the separating axis of its first contact with the scene's surface.
//
// Every statement that decides a bit of the answer is in sweep_triangle_rules.h and the walk in group_walk.h, which the host check
// (tests/check_sweep_triangle.cpp) runs against a brute force; how a lane reads a node and a record and keeps its stack is LaneAccess
// of query_lane.h; this file supplies the output record.  One lane per sweep, one wave per block, the per-lane stack in LDS: the
// launch shape of k_sweep_box.
#include "sweep_triangle.h"

#include "query_lane.h"
#include "sweep_triangle_rules.h"

using namespace rtdev;

namespace {

// One rt_triangle_sweep (v0 pad | v1 pad | v2 pad | direction tmax) per lane -> one rt_triangle_sweep_hit (normal t | axis 0 prim_id
// material_id).  Through the walk a lane keeps q0, u1, u2, the bounds with their box, d and 1 / d; v1 and v2 serve the spheres, before
// the walk and for a winning sphere's normal after it.
template <bool COUNT>
__global__ __launch_bounds__(WAVE) void k_sweep_triangle(DevScene sc, const float4* __restrict__ sweeps, uint4* __restrict__ out, uint32_t n,
                                                          unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const float4 s0 = sweeps[4 * (size_t)i], s1 = sweeps[4 * (size_t)i + 1], s2 = sweeps[4 * (size_t)i + 2], s3 = sweeps[4 * (size_t)i + 3];
    const float q0[3] = {s0.x, s0.y, s0.z}, q1[3] = {s1.x, s1.y, s1.z}, q2[3] = {s2.x, s2.y, s2.z}, direction[3] = {s3.x, s3.y, s3.z};
    const rt::StQuery q = rt::st_query(q0, q1, q2, direction, s3.w);
    LaneAccess<COUNT> acc(sc, s_stack);
    uint32_t r[8];
    rt::sb_answer_miss(q.b.tmax, r);
    if (rt::st_query_valid(q0, q1, q2, direction, s3.w)) { // degenerate queries are misses without a walk
        rt::CpBest best;
        best.order = rt::sw_start(q.b.tmax);
        best.slot = 0xFFFFFFFFu;
        for (uint32_t s = 0; s < sc.n_spheres; s++) { // the spheres by brute force, in index order
            const uint64_t c = rt::cp_order(rt::st_sphere(sc.spheres[s].center, sc.spheres[s].radius, q, q1, q2), s);
            if (c < best.order) best.order = c, best.slot = s;
        }
        rt::st_walk(acc, sc.n_nodes, q, best);
        if (best.slot != 0xFFFFFFFFu) { // normal and axis from the winner's record, not carried through the walk
            if ((uint32_t)best.order & RT_PRIM_SPHERE_FLAG) { // a triangle's key
                float rec[9];
                uint32_t ids[3];
                LaneAccess<false>(sc, nullptr).record(best.slot, rec, ids);
                rt::st_answer_triangle(rec, ids[0], best.order, q, r);
            } else {
                const DevSphere& s = sc.spheres[best.slot];
                rt::st_answer_sphere(s.center, s.radius, s.material_id, best.order, q, q1, q2, r);
            }
        }
    }
    out[2 * (size_t)i] = make_uint4(r[0], r[1], r[2], r[3]);
    out[2 * (size_t)i + 1] = make_uint4(r[4], r[5], r[6], r[7]);
    if (COUNT) flush_counts(counters, acc.cnt);
}

} // namespace

namespace rt {

hipError_t launch_sweep_triangle(const DevScene& sc, const void* sweeps, void* out, uint32_t n, unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = lane_stack_bytes(sc);
    const float4* p = reinterpret_cast<const float4*>(sweeps);
    uint4* o = reinterpret_cast<uint4*>(out);
    if (counters) hipLaunchKernelGGL((k_sweep_triangle<true>), grid, block, lds, stream, sc, p, o, n, counters);
    else hipLaunchKernelGGL((k_sweep_triangle<false>), grid, block, lds, stream, sc, p, o, n, counters);
    return hipGetLastError();
}

} // namespace rt
