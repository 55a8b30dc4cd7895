// path_query.hip — the kernels of rt_radiance (include/rt_hip.h, "Path queries"): the radiance the extended mode carries back along
// rays the caller supplies.
//
// Nothing here is new arithmetic.  A path is the body of ext_trace_path (kernels.hip), the nested-loop form, with the caller's ray in
// the place of the camera's: the first segment honours the ray's own (tmin, tmax) under k_rq_trace's degeneracy rules, as k_sq_surface
// does; every vertex is ext_light_sum with its shadow segments traced on the spot by occluded<> (ext_direct's lambda), then
// ext_leave_vertex and ext_scatter (device_common.h).  One lane per path, one wave per block, the per-lane stack in LDS as in
// k_sq_surface.  A path leaves one 16-byte record; a second kernel adds a ray's records in sample order from zero - the frames' pixel
// reduction - so there is no float atomic anywhere: the order is the result.
#include "path_query.h"

#include "../../include/rt_hip.h"
#include "device_common.h"

using namespace rtdev;

namespace {

#ifndef RT_PQ_MIN_WAVES
#define RT_PQ_MIN_WAVES 4 /* waves per SIMD asked of the register allocator: 101 VGPRs without scratch (the counting variant 105); 5 (96 VGPRs)
                             spills 4 registers, 6 (80) spills 25.  k_render_extended, the same loops, takes 122 at 4 waves ("Path queries") */
#endif

// Lane g of the launch is sample g % S of ray g / S of the launch's batch, so a ray's samples sit in consecutive lanes and share
// their first segment.  `first`: the index of the batch's first ray in the caller's array (the seed's); `lanes` = rays * S <=
// RT_QUERY_CHUNK.  dst[g] = (x, segments) of path g; with S == 1 that is the ray's rt_path_result, (0 + x) / 1.
template <bool COUNT>
__global__ __launch_bounds__(WAVE, RT_PQ_MIN_WAVES) void k_pq_trace(DevScene sc, rt::PathArgs a, const float4* __restrict__ rays, uint64_t first,
                                                                                               uint32_t lanes, uint4* __restrict__ dst,
                                                                                               unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries
    const uint32_t lane = threadIdx.x;
    uint2* stack = s_stack + lane;
    const uint32_t S = a.samples;
    // the wave's first lane in 64 bits (uniform), the lane's own from there in 32: lane + its sample index stay below 64 + S
    const uint64_t gw = (uint64_t)blockIdx.x * WAVE;
    const uint64_t pw = gw / S;
    const uint32_t sw = (uint32_t)(gw - pw * S) + lane;
    const uint64_t p = pw + sw / S; // the ray's index in the batch
    const uint32_t s = sw % S;
    // every lane stays to the end (the wave sums of the counters): a lane past the batch is "no path"
    const bool live = gw + lane < lanes;
    Counts cnt = {0u, 0u};
    SegCounts seg = {0u, 0u, 0u};
    V3 radiance = v3(0.0f, 0.0f, 0.0f);
    if (live) {
        const float4 ra = rays[2 * p], rb = rays[2 * p + 1];
        V3 o = v3(ra.x, ra.y, ra.z), d = v3(rb.x, rb.y, rb.z);
        // the degeneracy rules of k_rq_trace: a degenerate ray is no path
        bool valid = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z) &&
                     !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) && !isnan(ra.w) && !isnan(rb.w);
        float tmin = fmaxf(ra.w, RT_MIN_RAY_DISTANCE), tmax = rb.w; // of the segment at hand: the ray's own for the first
        valid = valid && tmin < tmax;
        if (valid) {
            SimpleRng rng = rng_for(a.seed + (uint32_t)(first + p), a.first_sample + s);
            if (a.camera_draws) { // what a jittered camera sample spent on its jitter (ext_sample_ray)
                rng.next_f32();
                rng.next_f32();
            }
            V3 throughput = v3(1.0f, 1.0f, 1.0f);
            uint32_t channel = 3;
            const bool shadows = a.shadows != 0u;
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
                const bool terminal = depth >= a.max_bounces;
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
        if (S == 1u) { // the reduction of one sample: (0 + x) / 1
            const V3 sum = v3(0.0f, 0.0f, 0.0f) + radiance;
            radiance = v3(sum.x / 1.0f, sum.y / 1.0f, sum.z / 1.0f);
        }
        dst[gw + lane] = make_uint4(__float_as_uint(radiance.x), __float_as_uint(radiance.y), __float_as_uint(radiance.z), seg.camera + seg.continuation + seg.shadow);
    }
    // one atomic per wave and counter, as flush_segment_counts
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

// Ray r of the batch: its S records in sample order, added from zero, divided once; the segment counts added mod 2^32.
__global__ __launch_bounds__(256) void k_pq_reduce(const uint4* __restrict__ paths, uint32_t n, uint32_t S, uint4* __restrict__ out) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint4* __restrict__ rec = paths + (size_t)r * S;
    V3 sum = v3(0.0f, 0.0f, 0.0f);
    uint32_t segments = 0;
    for (uint32_t k = 0; k < S; k++) {
        const uint4 x = rec[k];
        sum = sum + v3(__uint_as_float(x.x), __uint_as_float(x.y), __uint_as_float(x.z));
        segments += x.w;
    }
    const float fs = (float)S;
    out[r] = make_uint4(__float_as_uint(sum.x / fs), __float_as_uint(sum.y / fs), __float_as_uint(sum.z / fs), segments);
}

} // namespace

namespace rt {

hipError_t launch_path_query(const DevScene& sc, const PathArgs& a, const void* rays, uint64_t first, uint32_t n, void* scratch, void* out, bool count,
                             unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t lds = lane_stack_bytes(sc);
    const uint32_t lanes = n * a.samples;                                          // <= RT_QUERY_CHUNK (the caller's chunking)
    const float4* r = reinterpret_cast<const float4*>(rays);
    uint4* o = reinterpret_cast<uint4*>(out);
    uint4* dst = a.samples == 1u ? o : reinterpret_cast<uint4*>(scratch);
    const dim3 grid((lanes + WAVE - 1) / WAVE), block(WAVE);
    if (count) hipLaunchKernelGGL((k_pq_trace<true>), grid, block, lds, stream, sc, a, r, first, lanes, dst, counters);
    else hipLaunchKernelGGL((k_pq_trace<false>), grid, block, lds, stream, sc, a, r, first, lanes, dst, counters);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.samples == 1u) return e;
    hipLaunchKernelGGL(k_pq_reduce, dim3((n + 255u) / 256u), dim3(256), 0, stream, dst, n, a.samples, o);
    return hipGetLastError();
}

} // namespace rt
