// sweep.hip — the kernel of the sphere sweep of include/rt_hip.h (rt_sweep_sphere): for each moving sphere the caller supplies, the
// time and the point of its first contact with the scene's surface.
//
// Every statement that decides a bit of the answer, and the walk itself, is in sweep_rules.h, which the host check
// (tests/check_sweep.cpp) runs against a brute force; this file supplies how a lane reads a node and a record, its stack and the
// output record.  One lane per sweep, one wave per block, the per-lane stack in LDS: the launch shape of k_cp_nearest.
#include "sweep.h"

#include "device_common.h"
#include "sweep_rules.h"

using namespace rtdev;

namespace {

// What sw_walk (sweep_rules.h, rule 5) asks of its caller, for one lane: k_cp_nearest's LaneAccess.
template <bool COUNT>
struct SweepAccess {
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

// One rt_sweep (origin radius | direction tmax) per lane -> one rt_sweep_hit (position | t | u v | prim_id material_id).
template <bool COUNT>
__global__ __launch_bounds__(WAVE) void k_sweep_sphere(DevScene sc, const float4* __restrict__ sweeps, uint4* __restrict__ out, uint32_t n,
                                                        unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // (DevScene::stack_entries / 2 + 1) * 64 64-bit entries
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const float4 s0 = sweeps[2 * (size_t)i], s1 = sweeps[2 * (size_t)i + 1];
    const float origin[3] = {s0.x, s0.y, s0.z}, direction[3] = {s1.x, s1.y, s1.z};
    const rt::SwQuery q = rt::sw_query(origin, s0.w, direction, s1.w);
    SweepAccess<COUNT> acc;
    acc.nodes = reinterpret_cast<const uint4*>(sc.nodes);
    acc.tris = sc.tris;
    acc.stack = s_stack + threadIdx.x;
    acc.cnt = {0u, 0u};
    uint32_t r[8];
    rt::sw_answer_miss(q.tmax, r);
    if (rt::sw_query_valid(q)) { // degenerate queries are misses without a walk
        rt::CpBest best;
        best.order = rt::sw_start(q.tmax);
        best.slot = 0xFFFFFFFFu;
        for (uint32_t s = 0; s < sc.n_spheres; s++) { // the spheres by brute force, in index order
            const uint64_t c = rt::cp_order(rt::sw_sphere(sc.spheres[s].center, sc.spheres[s].radius, q), s);
            if (c < best.order) best.order = c, best.slot = s;
        }
        rt::sw_walk(acc, sc.n_nodes, q, best);
        if (best.slot != 0xFFFFFFFFu) {
            if ((uint32_t)best.order & RT_PRIM_SPHERE_FLAG) { // a triangle's key
                float rec[9];
                uint32_t ids[3];
                SweepAccess<false>{nullptr, sc.tris, nullptr, {0u, 0u}}.record(best.slot, rec, ids);
                rt::sw_answer_triangle(rec, ids[0], best.order, q, r);
            } else {
                const DevSphere& s = sc.spheres[best.slot];
                rt::sw_answer_sphere(s.center, s.radius, s.material_id, best.order, q, r);
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

hipError_t launch_sweep_sphere(const DevScene& sc, const void* sweeps, void* out, uint32_t n, unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = (size_t)(sc.stack_entries / 2u + 1u) * WAVE * sizeof(uint2); // as launch_closest_point
    const float4* p = reinterpret_cast<const float4*>(sweeps);
    uint4* o = reinterpret_cast<uint4*>(out);
    if (counters) hipLaunchKernelGGL((k_sweep_sphere<true>), grid, block, lds, stream, sc, p, o, n, counters);
    else hipLaunchKernelGGL((k_sweep_sphere<false>), grid, block, lds, stream, sc, p, o, n, counters);
    return hipGetLastError();
}

} // namespace rt
