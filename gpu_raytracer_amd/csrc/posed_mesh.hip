// posed_mesh.hip — the kernels of the posed-mesh queries of include/rt_hip.h (rt_overlap_mesh, rt_sweep_mesh): the caller's mesh of m
// triangles, given once, at n poses; per pose the number of touching (mesh triangle, primitive) pairs with the first touching
// triangle, or the first contact of the whole body in translation.
//
// Every statement that decides a bit of the answer is in mesh_pose_rules.h (the pose, a lane's running best, the shared bound, the
// reduction), overlap_triangle_rules.h and sweep_triangle_rules.h (what is done with a posed triangle) and group_walk.h (the walk),
// which the host check (tests/check_posed_mesh.cpp) runs against a brute force; how a lane reads a node and a record and keeps its
// stack is LaneAccess / LaneKeyAccess of query_lane.h.  This file supplies the layout and the reduction across lanes.
//
// Layout: one wave per block, the per-lane stack in LDS, as the other volume queries.  A pose is served by a GROUP of G = 2^lg
// lanes (posed_mesh_group: 1 for m = 1, else the smallest power of two >= m, at most 64), a wave serves 64 / G poses, and lane g of
// a group takes the mesh triangles g, g + G, g + 2G, ... in that order: a hull of 12 - 64 triangles fills a wave with 4 - 1 poses.
// Behind the stacks lie 64 words, one per group: the sweep's shared bound, the overlap's stop flag.  No lane returns before the
// reduction: lanes beyond n or beyond m carry the neutral element, so that the cross-lane operations see the whole wave converged.
// Known limit: a pose never spans more than one wave, so few poses of a very large mesh occupy few waves (rt_hip.h says so).
#include "posed_mesh.h"

#include <type_traits>

#include "mesh_pose_rules.h"
#include "query_lane.h"

using namespace rtdev;

namespace {

// the word of a lane's group, in LDS
struct LdsWord {
    uint32_t* p;
    __device__ __forceinline__ uint32_t read() const { return *reinterpret_cast<volatile uint32_t*>(p); }
    __device__ __forceinline__ void lower(uint32_t bits) { atomicMin(p, bits); }
};

// mesh triangle j at pose P: its three posed vertices
__device__ __forceinline__ void posed_triangle(const float4* __restrict__ mesh, uint32_t j, const rt::MpPose& P, float w0[3], float w1[3], float w2[3]) {
    const float4 t0 = mesh[3 * (size_t)j], t1 = mesh[3 * (size_t)j + 1], t2 = mesh[3 * (size_t)j + 2];
    const float v0[3] = {t0.x, t0.y, t0.z}, v1[3] = {t1.x, t1.y, t1.z}, v2[3] = {t2.x, t2.y, t2.z};
    rt::mp_vertex(P, v0, w0), rt::mp_vertex(P, v1, w1), rt::mp_vertex(P, v2, w2);
}

// The pose of record i (its first two float4 of `stride`): read and turned into R again for every triangle instead of being kept
// across the walk - twelve registers the walk can use (the index goes through an empty asm so that the loads are not hoisted).
__device__ __forceinline__ bool pose_of(const float4* __restrict__ records, uint32_t stride, uint32_t i, rt::MpPose& P) {
    asm volatile("" : "+v"(i));
    const float4 p0 = records[stride * (size_t)i], p1 = records[stride * (size_t)i + 1];
    const float position[3] = {p0.x, p0.y, p0.z}, rotation[4] = {p1.x, p1.y, p1.z, p1.w};
    return rt::mp_pose(position, rotation, P);
}

// the butterfly over the 2^lg lanes of a group (aligned, so lane ^ off stays inside it); every lane of the wave takes part
__device__ __forceinline__ uint64_t group_min64(uint64_t x, uint32_t lg) {
    for (uint32_t off = (1u << lg) >> 1; off; off >>= 1) {
        const uint64_t o = ((uint64_t)__shfl_xor((uint32_t)(x >> 32), (int)off) << 32) | __shfl_xor((uint32_t)x, (int)off);
        x = o < x ? o : x;
    }
    return x;
}
__device__ __forceinline__ uint64_t group_sum64(uint64_t x, uint32_t lg) {
    for (uint32_t off = (1u << lg) >> 1; off; off >>= 1)
        x += ((uint64_t)__shfl_xor((uint32_t)(x >> 32), (int)off) << 32) | __shfl_xor((uint32_t)x, (int)off);
    return x;
}
__device__ __forceinline__ uint32_t group_min32(uint32_t x, uint32_t lg) {
    for (uint32_t off = (1u << lg) >> 1; off; off >>= 1) {
        const uint32_t o = __shfl_xor(x, (int)off);
        x = o < x ? o : x;
    }
    return x;
}

// One rt_pose (position pad | rotation) per group -> pairs[i] and, unless null, first[i].
template <bool COUNT, int MODE>
__global__ __launch_bounds__(WAVE) void k_overlap_mesh(DevScene sc, const float4* __restrict__ mesh, uint32_t m, const float4* __restrict__ poses,
                                                        uint32_t* __restrict__ pairs, uint32_t* __restrict__ first, uint32_t n, uint32_t lg,
                                                        unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries, then 64 words: a stop flag per group
    uint32_t* s_flag = reinterpret_cast<uint32_t*>(s_stack + (size_t)lane_stack_entries(sc) * WAVE);
    const uint32_t G = 1u << lg, group = threadIdx.x >> lg, g = threadIdx.x & (G - 1u);
    const uint32_t i = blockIdx.x * (WAVE >> lg) + group;
    const bool live = i < n;
    float4 p0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p1 = p0;
    if (live) p0 = poses[2 * (size_t)i], p1 = poses[2 * (size_t)i + 1];
    if (g == 0u) s_flag[group] = 0u;
    __syncthreads();
    const float position[3] = {p0.x, p0.y, p0.z}, rotation[4] = {p1.x, p1.y, p1.z, p1.w};
    LaneKeyAccess<COUNT> acc(sc, s_stack); // the list has no words: nothing is listed (cap 0)
    rt::MpPose P;
    uint64_t sum = 0ull;
    uint32_t low = rt::MP_NONE;
    if (live && rt::mp_pose(position, rotation, P)) { // an invalid pose touches nothing, without a walk
        for (uint32_t j = g; j < m; j += G) {
            if (MODE == rt::OV_ANY && *reinterpret_cast<volatile uint32_t*>(&s_flag[group])) break;
            float q0[3], q1[3], q2[3];
            posed_triangle(mesh, j, P, q0, q1, q2);
            if (!rt::ot_query_valid(q0, q1, q2)) continue; // what k_overlap_triangle<., MODE> runs for it
            rt::OvList list;
            rt::ov_list_init(list, 0u);
            rt::OtQuery q;
            rt::ot_query_init(q, q0, q1, q2);
            for (uint32_t s = 0; s < sc.n_spheres; s++) { // the spheres by brute force, in index order
                if (MODE == rt::OV_ANY && list.total) break;
                if (rt::ot_sphere(sc.spheres[s].center, sc.spheres[s].radius, q)) rt::ov_list_offer(acc, list, s);
            }
            if (MODE != rt::OV_ANY || list.total == 0u) rt::ot_walk<MODE>(acc, sc.n_nodes, q, list);
            if (list.total == 0u) continue;
            sum += list.total;
            if (low == rt::MP_NONE) low = j; // j only grows
            if (MODE == rt::OV_ANY) {
                s_flag[group] = 1u;
                break;
            }
        }
    }
    sum = group_sum64(sum, lg); // the whole wave is here
    low = group_min32(low, lg);
    if (live && g == 0u) {
        pairs[i] = MODE == rt::OV_ANY ? (sum ? 1u : 0u) : (sum < 0xFFFFFFFFull ? (uint32_t)sum : 0xFFFFFFFFu);
        if (first) first[i] = low;
    }
    if (COUNT) flush_counts(counters, acc.cnt);
}

// One rt_pose_sweep (position pad | rotation | direction tmax) per group -> one rt_mesh_sweep_hit (normal t | axis triangle prim_id
// material_id).  SHARE: the group's word carries the body's best time (mesh_pose_rules.h, rule 4).
template <bool COUNT, bool SHARE>
__global__ __launch_bounds__(WAVE) void k_sweep_mesh(DevScene sc, const float4* __restrict__ mesh, uint32_t m, const float4* __restrict__ sweeps,
                                                      uint4* __restrict__ out, uint32_t n, uint32_t lg, unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries, then 64 words: the shared bound per group
    uint32_t* s_word = reinterpret_cast<uint32_t*>(s_stack + (size_t)lane_stack_entries(sc) * WAVE);
    const uint32_t G = 1u << lg, group = threadIdx.x >> lg, g = threadIdx.x & (G - 1u);
    const uint32_t i = blockIdx.x * (WAVE >> lg) + group;
    const bool live = i < n;
    float4 p2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) p2 = sweeps[3 * (size_t)i + 2];
    const float tmax = p2.w;
    if (SHARE) {
        if (g == 0u) s_word[group] = rt::cp_bits(tmax);
        __syncthreads();
    }
    const float direction[3] = {p2.x, p2.y, p2.z};
    LaneAccess<COUNT> acc(sc, s_stack);
    rt::MpPose P;
    rt::MpBest own;
    rt::mp_best_init(own, tmax);
    if (live && pose_of(sweeps, 3u, i, P)) { // an invalid pose is a miss, without a walk
        typename std::conditional<SHARE, LdsWord, rt::MpNoShare>::type sh{};
        if constexpr (SHARE) sh.p = &s_word[group];
        rt::CpBest best{own.order, rt::MP_NONE}; // the lane's running order over all its triangles
        for (uint32_t j = g; j < m; j += G) {
            float q0[3], q1[3], q2[3];
            (void)pose_of(sweeps, 3u, i, P);
            posed_triangle(mesh, j, P, q0, q1, q2);
            if (!rt::st_query_valid(q0, q1, q2, direction, tmax)) continue; // what k_sweep_triangle runs for it
            const rt::StQuery q = rt::st_query(q0, q1, q2, direction, tmax);
            best.order = rt::mp_tighten(best.order, sh.read());
            for (uint32_t s = 0; s < sc.n_spheres; s++) // the spheres by brute force, in index order
                rt::mp_sweep_sphere(rt::cp_order(rt::st_sphere(sc.spheres[s].center, sc.spheres[s].radius, q, q1, q2), s), s, j, best, own, sh);
            rt::mp_sweep_walk(acc, sc.n_nodes, q, j, best, own, sh);
        }
    }
    const uint64_t least = group_min64(rt::mp_reduce_order(own), lg); // the whole wave is here
    const uint32_t winner = group_min32(own.j != rt::MP_NONE && own.order == least ? own.j : rt::MP_NONE, lg);
    uint32_t r[8];
    bool writes = false;
    if (live && winner == rt::MP_NONE) {
        writes = g == 0u;
        rt::mp_answer_miss(tmax, r);
    } else if (live && own.j == winner) { // normal and axis from the winner's record and its triangle posed once more
        writes = true;
        float q0[3], q1[3], q2[3];
        (void)pose_of(sweeps, 3u, i, P);
        posed_triangle(mesh, own.j, P, q0, q1, q2);
        const rt::StQuery q = rt::st_query(q0, q1, q2, direction, tmax);
        if ((uint32_t)own.order & RT_PRIM_SPHERE_FLAG) { // a triangle's key
            float rec[9];
            uint32_t ids[3];
            LaneAccess<false>(sc, nullptr).record(own.slot, rec, ids);
            rt::st_answer_triangle(rec, ids[0], own.order, q, r);
        } else {
            const DevSphere& s = sc.spheres[own.slot];
            rt::st_answer_sphere(s.center, s.radius, s.material_id, own.order, q, q1, q2, r);
        }
        r[5] = own.j;
    }
    if (writes) {
        out[2 * (size_t)i] = make_uint4(r[0], r[1], r[2], r[3]);
        out[2 * (size_t)i + 1] = make_uint4(r[4], r[5], r[6], r[7]);
    }
    if (COUNT) flush_counts(counters, acc.cnt);
}

uint32_t log2_of(uint32_t g) {
    uint32_t lg = 0u;
    while ((1u << lg) < g) lg++;
    return lg;
}

template <int MODE>
void launch_overlap_mode(const DevScene& sc, const float4* mesh, uint32_t m, const float4* poses, uint32_t* pairs, uint32_t* first, uint32_t n, uint32_t lg,
                         size_t lds, unsigned long long* counters, hipStream_t stream) {
    const uint32_t per_wave = WAVE >> lg;
    const dim3 grid((n + per_wave - 1) / per_wave), block(WAVE);
    if (counters) hipLaunchKernelGGL((k_overlap_mesh<true, MODE>), grid, block, lds, stream, sc, mesh, m, poses, pairs, first, n, lg, counters);
    else hipLaunchKernelGGL((k_overlap_mesh<false, MODE>), grid, block, lds, stream, sc, mesh, m, poses, pairs, first, n, lg, counters);
}

template <bool SHARE>
void launch_sweep_share(const DevScene& sc, const float4* mesh, uint32_t m, const float4* sweeps, uint4* out, uint32_t n, uint32_t lg, size_t lds,
                        unsigned long long* counters, hipStream_t stream) {
    const uint32_t per_wave = WAVE >> lg;
    const dim3 grid((n + per_wave - 1) / per_wave), block(WAVE);
    if (counters) hipLaunchKernelGGL((k_sweep_mesh<true, SHARE>), grid, block, lds, stream, sc, mesh, m, sweeps, out, n, lg, counters);
    else hipLaunchKernelGGL((k_sweep_mesh<false, SHARE>), grid, block, lds, stream, sc, mesh, m, sweeps, out, n, lg, counters);
}

} // namespace

namespace rt {

hipError_t launch_overlap_mesh(const DevScene& sc, const void* mesh, uint32_t m, const void* poses, uint32_t* pairs, uint32_t* first, uint32_t n, int mode,
                               unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (m == 0 || !mesh || !pairs || (mode == OV_ANY && first)) return hipErrorInvalidValue;
    const uint32_t lg = log2_of(posed_mesh_group(m));
    const size_t lds = lane_stack_bytes(sc) + WAVE * sizeof(uint32_t); // stacks + a word per group
    const float4 *t = reinterpret_cast<const float4*>(mesh), *p = reinterpret_cast<const float4*>(poses);
    switch (mode) {
    case OV_COUNT_ALL: launch_overlap_mode<OV_COUNT_ALL>(sc, t, m, p, pairs, first, n, lg, lds, counters, stream); break;
    case OV_ANY: launch_overlap_mode<OV_ANY>(sc, t, m, p, pairs, first, n, lg, lds, counters, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_sweep_mesh(const DevScene& sc, const void* mesh, uint32_t m, const void* sweeps, void* out, uint32_t n, bool share,
                             unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (m == 0 || !mesh) return hipErrorInvalidValue;
    const uint32_t lg = log2_of(posed_mesh_group(m));
    const size_t lds = lane_stack_bytes(sc) + WAVE * sizeof(uint32_t); // stacks + a word per group
    const float4 *t = reinterpret_cast<const float4*>(mesh), *p = reinterpret_cast<const float4*>(sweeps);
    uint4* o = reinterpret_cast<uint4*>(out);
    if (share) launch_sweep_share<true>(sc, t, m, p, o, n, lg, lds, counters, stream);
    else launch_sweep_share<false>(sc, t, m, p, o, n, lg, lds, counters, stream);
    return hipGetLastError();
}

} // namespace rt
