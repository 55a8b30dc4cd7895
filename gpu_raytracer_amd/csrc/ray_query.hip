// ray_query.hip — the kernels of the ray queries of include/rt_hip.h: closest hit (rt_intersect), any hit (rt_occluded) and the
// first K hits (rt_intersect_all) of rays the caller supplies, and the frames' camera rays as such records (rt_camera_rays).
// The list and the walk of rt_intersect_all are in multi_hit_walk.h, which inside.hip shares.
//
// A query ray is walked by the code the frames use (device_common.h: test_spheres, traverse, occluded), with the ray's own
// range: the walk starts from hit = (tmax, miss) and accepts tmin < t < hit.t, so the frames' strict compare and tie rule give
// the range semantics.  One lane per ray, one wave per block, the per-lane stack in LDS as in k_render_reference.
#include "ray_query.h"

#include <algorithm>

#include "device_common.h"
#include "multi_hit_walk.h"

using namespace rtdev;

namespace {

// One rt_ray (ox oy oz tmin | dx dy dz tmax) per lane -> one rt_hit (t u v prim_id) or, ANY_HIT, one byte.
template <bool COUNT, bool ANY_HIT>
__global__ __launch_bounds__(WAVE) void k_rq_trace(DevScene sc, const float4* __restrict__ rays, void* __restrict__ out, uint32_t n,
                                                    unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    uint2* stack = s_stack + threadIdx.x;
    const float4 ra = rays[2 * (size_t)i], rb = rays[2 * (size_t)i + 1];
    const V3 o = v3(ra.x, ra.y, ra.z), d = v3(rb.x, rb.y, rb.z);
    const float tmax = rb.w;
    // degenerate rays are misses without a walk: non-finite origin or direction, zero direction, NaN bounds, an empty range
    bool valid = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z) &&
                 !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) && !isnan(ra.w) && !isnan(tmax);
    const float tmin = fmaxf(ra.w, RT_MIN_RAY_DISTANCE); // the floor the box filter is conservative for
    valid = valid && tmin < tmax;
    Counts cnt = {0u, 0u};
    if (ANY_HIT) {
        const bool occ = valid && occluded<COUNT>(sc, o, d, tmin, tmax, stack, cnt);
        reinterpret_cast<uint8_t*>(out)[i] = occ ? 1u : 0u;
    } else {
        Hit hit;
        hit.t = tmax;
        hit.prim = RT_PRIM_MISS;
        hit.slot = 0;
        if (valid) {
            test_spheres(sc, o, d, hit, tmin);
            traverse<COUNT, false>(sc, o, d, stack, hit, cnt, tmin);
        }
        float uv[2] = {0.0f, 0.0f};
        if (hit.prim < RT_PRIM_SPHERE_FLAG) { // a triangle: the test that accepted it once more, for its barycentrics
            const float4* p = reinterpret_cast<const float4*>(sc.tris + hit.slot);
            const float4 q0 = p[0], q1 = p[1], q2 = p[2];
            float t;
            moller_trumbore(v3(q0.x, q0.y, q0.z), v3(q0.w, q1.x, q1.y), v3(q1.z, q1.w, q2.x), o, d, t, uv);
        }
        reinterpret_cast<uint4*>(out)[i] = make_uint4(__float_as_uint(hit.t), __float_as_uint(uv[0]), __float_as_uint(uv[1]), hit.prim);
    }
    if (COUNT) flush_counts(counters, cnt);
}

// One rt_ray per lane -> max_hits rt_hit records at out[i * max_hits ..] (the listed candidates, then misses) and, counts != null,
// counts[i] = the records listed, or COUNT_ALL: all candidates in the range.  max_hits == 0 (COUNT_ALL only): `out` is not touched.
template <bool COUNT, bool COUNT_ALL>
__global__ __launch_bounds__(WAVE) void k_rq_trace_all(DevScene sc, const float4* __restrict__ rays, uint4* __restrict__ out, uint32_t* __restrict__ counts,
                                                        uint32_t n, uint32_t max_hits, unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // the stack of k_rq_trace, then 3 * max_hits * 64 list words
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    uint2* stack = s_stack + threadIdx.x;
    const float4 ra = rays[2 * (size_t)i], rb = rays[2 * (size_t)i + 1];
    const V3 o = v3(ra.x, ra.y, ra.z), d = v3(rb.x, rb.y, rb.z);
    const float tmax = rb.w;
    // the degeneracy rules of k_rq_trace
    bool valid = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z) &&
                 !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) && !isnan(ra.w) && !isnan(tmax);
    const float tmin = fmaxf(ra.w, RT_MIN_RAY_DISTANCE);
    valid = valid && tmin < tmax;
    Counts cnt = {0u, 0u};
    HitList list;
    list.init(reinterpret_cast<uint32_t*>(s_stack + (size_t)lane_stack_entries(sc) * WAVE) + threadIdx.x, max_hits, tmax);
    if (valid) {
        for (uint32_t s = 0; s < sc.n_spheres; s++) {
            float t;
            if (sphere_candidate(sc.spheres[s], o, d, tmin, tmax, t)) list.offer(t, s, s);
        }
        traverse_all<COUNT, COUNT_ALL>(sc, o, d, stack, list, cnt, tmin, tmax);
    }
    uint4* rec = out + (size_t)i * max_hits;
    for (uint32_t k = 0; k < max_hits; k++) {
        uint4 r = make_uint4(__float_as_uint(tmax), 0u, 0u, RT_PRIM_MISS);
        if (k < list.n) {
            const uint32_t key = list.e[(3u * k + 1u) * WAVE], slot = list.e[(3u * k + 2u) * WAVE];
            float uv[2] = {0.0f, 0.0f};
            if (key & RT_PRIM_SPHERE_FLAG) { // a triangle: the test that accepted it once more, for its barycentrics
                const float4* p = reinterpret_cast<const float4*>(sc.tris + slot);
                const float4 q0 = p[0], q1 = p[1], q2 = p[2];
                float t;
                moller_trumbore(v3(q0.x, q0.y, q0.z), v3(q0.w, q1.x, q1.y), v3(q1.z, q1.w, q2.x), o, d, t, uv);
            }
            r = make_uint4(list.e[(3u * k) * WAVE], __float_as_uint(uv[0]), __float_as_uint(uv[1]), key ^ RT_PRIM_SPHERE_FLAG);
        }
        rec[k] = r;
    }
    if (counts) counts[i] = COUNT_ALL ? list.total : list.n;
    if (COUNT) flush_counts(counters, cnt);
}

// rt_camera_rays: camera_ray of the frames at the pixel centres, one lane per pixel.
__global__ __launch_bounds__(256) void k_rq_camera_rays(DevCamera cam, uint32_t width, bool wavefront, float4* __restrict__ out, uint64_t first,
                                                         uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t pix = first + i;
    const uint32_t px = (uint32_t)(pix % width), py = (uint32_t)(pix / width);
    V3 o, d;
    camera_ray(cam, (float)px + 0.5f, (float)py + 0.5f, wavefront, o, d);
    out[2 * (size_t)i] = make_float4(o.x, o.y, o.z, RT_MIN_RAY_DISTANCE);
    out[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, RT_F32_MAX);
}

} // namespace

namespace rt {

hipError_t launch_ray_query(const DevScene& sc, const void* rays, void* out, uint32_t n, bool any_hit, unsigned long long* counters,
                            hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = lane_stack_bytes(sc);
    const float4* r = reinterpret_cast<const float4*>(rays);
    if (any_hit) {
        if (counters) hipLaunchKernelGGL((k_rq_trace<true, true>), grid, block, lds, stream, sc, r, out, n, counters);
        else hipLaunchKernelGGL((k_rq_trace<false, true>), grid, block, lds, stream, sc, r, out, n, counters);
    } else {
        if (counters) hipLaunchKernelGGL((k_rq_trace<true, false>), grid, block, lds, stream, sc, r, out, n, counters);
        else hipLaunchKernelGGL((k_rq_trace<false, false>), grid, block, lds, stream, sc, r, out, n, counters);
    }
    return hipGetLastError();
}

hipError_t launch_ray_query_all(const DevScene& sc, const void* rays, void* hits, uint32_t* counts, uint32_t n, uint32_t max_hits, bool count_all,
                                unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = lane_stack_bytes(sc) + (size_t)max_hits * 3u * WAVE * sizeof(uint32_t); // stack + list
    const float4* r = reinterpret_cast<const float4*>(rays);
    uint4* h = reinterpret_cast<uint4*>(hits);
    if (count_all) {
        if (counters) hipLaunchKernelGGL((k_rq_trace_all<true, true>), grid, block, lds, stream, sc, r, h, counts, n, max_hits, counters);
        else hipLaunchKernelGGL((k_rq_trace_all<false, true>), grid, block, lds, stream, sc, r, h, counts, n, max_hits, counters);
    } else {
        if (counters) hipLaunchKernelGGL((k_rq_trace_all<true, false>), grid, block, lds, stream, sc, r, h, counts, n, max_hits, counters);
        else hipLaunchKernelGGL((k_rq_trace_all<false, false>), grid, block, lds, stream, sc, r, h, counts, n, max_hits, counters);
    }
    return hipGetLastError();
}

hipError_t launch_camera_rays(const DevCamera& cam, uint32_t width, bool wavefront, void* out, uint64_t first, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rq_camera_rays, dim3((n + 255u) / 256u), dim3(256), 0, stream, cam, width, wavefront, reinterpret_cast<float4*>(out),
                       first, n);
    return hipGetLastError();
}

} // namespace rt
