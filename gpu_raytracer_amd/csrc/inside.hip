// inside.hip — the kernel of the inside test and the signed distance of include/rt_hip.h (rt_inside, rt_signed_distance): for each
// point the caller supplies, whether it lies inside the scene's solids by a majority of crossing parities, and rt_closest_point's
// record with that sign.
//
// Nothing that decides a bit is stated here: the directions, sphere containment, the stop rule, the majority and the signing are in
// inside_rules.h; a vote is the count traverse_all (multi_hit_walk.h) gives a list of capacity 0 with COUNT_ALL, the walk of
// rt_intersect_all's pure count; the magnitude is k_cp_nearest's lane (cp_nearest_lane, query_lane.h).  One lane
// per point, one wave per block, the launch shape of k_cp_nearest; the per-lane stack in LDS serves the closest-point walk first and
// then each ray walk in turn - every walk starts and ends with an empty stack, and a lane runs them one after another.
#include "inside.h"

#include "inside_rules.h"
#include "multi_hit_walk.h"
#include "query_lane.h"

using namespace rtdev;

namespace {

// One rt_point_query (px py pz radius) per lane -> DISTANCE: one rt_nearest at out[2 i], signed; else one byte at out_inside[i]; and,
// votes != null, one byte at votes[i] = the odd votes of all `rays` rays.  counters[RT_CNT_SEGMENTS] += the rays traced.
template <bool COUNT, bool DISTANCE>
__global__ __launch_bounds__(WAVE) void k_inside(DevScene sc, const float4* __restrict__ points, void* __restrict__ out, uint8_t* __restrict__ votes,
                                                  uint32_t n, uint32_t rays, unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const float4 pq = points[i];
    const float p[3] = {pq.x, pq.y, pq.z};
    uint2* stack = s_stack + threadIdx.x;
    Counts cnt = {0u, 0u};
    const bool valid = DISTANCE ? rt::cp_query_valid(p, pq.w) : rt::inside_query_valid(p);
    bool sphere_inside = false;
    if (valid)
        for (uint32_t s = 0; s < sc.n_spheres; s++) // in index order, before any ray
            sphere_inside = sphere_inside || rt::inside_sphere(sc.spheres[s].center, sc.spheres[s].radius, p);
    uint32_t r[8];
    if (DISTANCE) { // k_cp_nearest's answer
        LaneAccess<COUNT> acc(sc, s_stack);
        cp_nearest_lane(sc, acc, p, pq.w, r); // `valid` is its own test of the query
        cnt = acc.cnt;
    }
    // the votes, in order; a lane whose votes are not asked for stops at its majority, and traces nothing inside a sphere
    uint32_t odd = 0u, traced = 0u;
    bool go = valid && (votes != nullptr || !sphere_inside);
    const V3 o = v3(p[0], p[1], p[2]);
    for (uint32_t k = 0; k < rays; k++) {
        if (!go) continue;
        float dk[3];
        rt::inside_direction(k, dk);
        HitList list;
        list.init(nullptr, 0u, INFINITY); // capacity 0: offer only counts
        traverse_all<COUNT, true>(sc, o, v3(dk[0], dk[1], dk[2]), stack, list, cnt, RT_MIN_RAY_DISTANCE, INFINITY);
        traced++;
        odd += list.total & 1u;
        if (votes == nullptr && rt::inside_decided(odd, traced - odd, rays)) go = false;
    }
    const bool inside = sphere_inside || rt::inside_majority(odd, rays);
    if (DISTANCE) {
        rt::inside_sign(r, inside);
        uint4* rec = reinterpret_cast<uint4*>(out);
        rec[2 * (size_t)i] = make_uint4(r[0], r[1], r[2], r[3]);
        rec[2 * (size_t)i + 1] = make_uint4(r[4], r[5], r[6], r[7]);
    } else {
        reinterpret_cast<uint8_t*>(out)[i] = inside ? 1u : 0u;
    }
    if (votes) votes[i] = (uint8_t)odd;
    atomicAdd(&counters[RT_CNT_SEGMENTS], (unsigned long long)traced);
    if (COUNT) flush_counts(counters, cnt);
}

} // namespace

namespace rt {

hipError_t launch_inside(const DevScene& sc, const void* points, void* out, uint8_t* votes, uint32_t n, uint32_t rays, bool distance, bool count,
                         unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!inside_rays_valid(rays) || !counters) return hipErrorInvalidValue;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = lane_stack_bytes(sc); // one stack for both walks
    const float4* p = reinterpret_cast<const float4*>(points);
    if (distance) {
        if (count) hipLaunchKernelGGL((k_inside<true, true>), grid, block, lds, stream, sc, p, out, votes, n, rays, counters);
        else hipLaunchKernelGGL((k_inside<false, true>), grid, block, lds, stream, sc, p, out, votes, n, rays, counters);
    } else {
        if (count) hipLaunchKernelGGL((k_inside<true, false>), grid, block, lds, stream, sc, p, out, votes, n, rays, counters);
        else hipLaunchKernelGGL((k_inside<false, false>), grid, block, lds, stream, sc, p, out, votes, n, rays, counters);
    }
    return hipGetLastError();
}

} // namespace rt
