// path_walk.h — the path loop of the path queries as a function: the body of ext_trace_path (kernels.hip), the nested-loop form, from
// the segment (o, tmin, d, tmax) on.  The first segment honours the caller's (tmin, tmax); every later one is a continuation as the
// frames trace it.  Every vertex is ext_light_sum with its shadow segments traced on the spot by occluded<> (ext_direct's lambda), then
// ext_leave_vertex and ext_scatter (device_common.h).  `rng` is the path's generator after whatever was drawn before the path; `stack`
// the lane's own stack in LDS.
// k_ps_trace (probe_query.hip, rt_radiance_sh) and k_ir_trace (irradiance_query.hip, rt_irradiance) call it.  k_pq_trace
// (path_query.hip, rt_radiance) holds the same statements in its own body: called from there, the same optimised IR but for the order
// of its phis came out of the register allocator with 114 VGPRs where the kernel has 101 ("Probe queries"), so it
// is left as it was.  rt_radiance_sh's and rt_irradiance's tests hold the two to the same bits.
#ifndef RT_PATH_WALK_H
#define RT_PATH_WALK_H

#include "device_common.h"

namespace rtdev {

template <bool COUNT>
__device__ __forceinline__ void walk_path(const DevScene& sc, SimpleRng rng, uint32_t max_bounces, bool shadows, V3 o, V3 d, float tmin, float tmax,
                                          uint2* stack, Counts& cnt, SegCounts& seg, V3& radiance) {
    V3 throughput = v3(1.0f, 1.0f, 1.0f);
    uint32_t channel = 3;
    for (uint32_t depth = 0;; depth++) { // the body of ext_trace_path
        if (depth == 0) seg.camera++; else seg.continuation++;
        // one walk for both kinds of segment: with (RT_MIN_RAY_DISTANCE, RT_F32_MAX) these three statements are find_closest
        Hit hit;
        hit.t = tmax;
        hit.prim = RT_PRIM_MISS;
        hit.slot = 0;
        test_spheres(sc, o, d, hit, tmin);
        traverse<COUNT, false>(sc, o, d, stack, hit, cnt, tmin);
        tmin = RT_MIN_RAY_DISTANCE, tmax = RT_F32_MAX;
        if (hit.prim == RT_PRIM_MISS) {
            radiance = radiance + RT_SKY() * throughput;
            break;
        }
        V3 point, normal;
        uint32_t material_id;
        hit_geometry(sc, hit, o, d, point, normal, material_id);
        if (material_id >= sc.n_materials) {
            radiance = radiance + RT_MAGENTA() * throughput;
            break;
        }
        const DevMaterial m = sc.materials[material_id];
        const bool terminal = depth >= max_bounces;
        const V3 lighting = ext_light_sum(sc.lights, sc.n_lights, m, point, normal, terminal, shadows, [&](uint32_t, V3 sdir, float sdist) {
            seg.shadow++; // (ext_direct)
            return !occluded<COUNT>(sc, point + normal * EXT_EPS, sdir, RT_MIN_RAY_DISTANCE, sdist, stack, cnt);
        });
        const float tf = ext_leave_vertex(m, lighting, terminal, throughput, radiance);
        if (terminal) break;
        V3 norigin, ndir;
        if (!ext_scatter(m, point, normal, d, tf, depth, rng, channel, throughput, norigin, ndir)) break;
        o = norigin;
        d = ndir;
    }
}

// One atomic per wave and counter, as flush_segment_counts: every lane of the wave gets here.
template <bool COUNT>
__device__ __forceinline__ void flush_query_counts(const SegCounts& seg, const Counts& cnt, uint32_t lane, unsigned long long* __restrict__ counters) {
    const unsigned long long c0 = wave_sum(seg.camera), c1 = wave_sum(seg.continuation), c2 = wave_sum(seg.shadow);
    const unsigned long long n0 = COUNT ? wave_sum(cnt.nodes) : 0ull, n1 = COUNT ? wave_sum(cnt.tris) : 0ull;
    if (lane == 0) {
        if (c0) atomicAdd(&counters[RT_CNT_CAMERA], c0);
        if (c1) atomicAdd(&counters[RT_CNT_CONTINUATION], c1);
        if (c2) atomicAdd(&counters[RT_CNT_SHADOW], c2);
        if (COUNT) {
            atomicAdd(&counters[RT_CNT_NODE_VISITS], n0);
            atomicAdd(&counters[RT_CNT_TRI_TESTS], n1);
        }
    }
}

} // namespace rtdev
#endif
