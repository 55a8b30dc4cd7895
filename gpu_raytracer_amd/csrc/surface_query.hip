// surface_query.hip — the kernels of the surface queries of include/rt_hip.h: the hit point, geometric normal and material of the
// closest hit of rays the caller supplies (rt_surface), and the ambient occlusion of such points (rt_ambient_occlusion).
//
// Both are compositions of what the frames and the ray queries already do (device_common.h): rt_surface is k_rq_trace's closest-hit
// walk followed by hit_geometry and the continuation's face-forward; an ambient-occlusion sample is the cosine lobe of ext_scatter's
// diffuse branch (rng_for, two draws, normalize(N + unit_vector)) walked by occluded<> under k_rq_trace's degeneracy rules.  One wave
// per block, the per-lane stack in LDS as in k_render_reference.
#include "surface_query.h"

#include <algorithm>

#include "device_common.h"

using namespace rtdev;

namespace {

// One rt_ray (ox oy oz tmin | dx dy dz tmax) per lane -> one rt_surface_point (px py pz prim_id | nx ny nz material_id).
template <bool COUNT>
__global__ __launch_bounds__(WAVE) void k_sq_surface(DevScene sc, const float4* __restrict__ rays, uint4* __restrict__ out, uint32_t n,
                                                      unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries
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
    Hit hit;
    hit.t = tmax;
    hit.prim = RT_PRIM_MISS;
    hit.slot = 0;
    if (valid) {
        test_spheres(sc, o, d, hit, tmin);
        traverse<COUNT, false>(sc, o, d, stack, hit, cnt, tmin);
    }
    uint4 r0 = make_uint4(0u, 0u, 0u, RT_PRIM_MISS), r1 = make_uint4(0u, 0u, 0u, 0u); // a miss
    if (hit.prim != RT_PRIM_MISS) {
        V3 point, normal;
        uint32_t material_id;
        hit_geometry(sc, hit, o, d, point, normal, material_id);
        const V3 nf = dot(normal, d) < 0.0f ? normal : -normal; // face-forwarded, the continuation's nf
        r0 = make_uint4(__float_as_uint(point.x), __float_as_uint(point.y), __float_as_uint(point.z), hit.prim);
        r1 = make_uint4(__float_as_uint(nf.x), __float_as_uint(nf.y), __float_as_uint(nf.z), material_id);
    }
    out[2 * (size_t)i] = r0;
    out[2 * (size_t)i + 1] = r1;
    if (COUNT) flush_counts(counters, cnt);
}

// One lane per (point, sample): lane g of the batch (g0 = the launch's first) is sample g % S of point g / S, so a point's samples sit
// in consecutive lanes and a wave's rays share their origins.  `points` holds the batch's records, `first` is the index of its first
// point in the caller's array (the seed's), `lanes` = points * S.  Each lane makes its ray, walks it and votes; the first lane of every
// run of one point in the wave adds the run's unoccluded samples to the point's count.
template <bool COUNT>
__global__ __launch_bounds__(WAVE) void k_sq_ao(DevScene sc, const float4* __restrict__ points, uint64_t first, uint64_t g0, uint64_t lanes,
                                                 uint32_t S, uint32_t seed, float max_distance, float bias, uint32_t* __restrict__ unoccluded,
                                                 unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[];
    uint2* stack = s_stack + threadIdx.x;
    const uint32_t lane = threadIdx.x;
    // the wave's first lane in 64 bits (uniform), the lane's own from there in 32: lane + its sample index stay below 64 + S
    const uint64_t gw = g0 + (uint64_t)blockIdx.x * WAVE;
    const uint64_t pw = gw / S;
    const uint32_t sw = (uint32_t)(gw - pw * S) + lane;
    const uint64_t p = pw + sw / S; // the point's index in the batch
    const uint32_t s = sw % S;
    const bool live = gw + lane < lanes;
    Counts cnt = {0u, 0u};
    bool open = false; // the sample exists and is not occluded
    if (live) {
        const float4 pa = points[2 * p], pb = points[2 * p + 1];
        const V3 P = v3(pa.x, pa.y, pa.z), N = v3(pb.x, pb.y, pb.z);
        // a point that is no point traces nothing: all its samples are open
        const bool point_ok = isfinite(P.x) && isfinite(P.y) && isfinite(P.z) && isfinite(N.x) && isfinite(N.y) && isfinite(N.z) &&
                              !(N.x == 0.0f && N.y == 0.0f && N.z == 0.0f);
        open = true;
        if (point_ok) {
            SimpleRng rng = rng_for(seed + (uint32_t)(first + p), s);
            const float u1 = rng.next_f32(), u2 = rng.next_f32();
            const V3 d = normalize(N + unit_vector(u1, u2)); // the cosine lobe of ext_scatter
            const V3 o = P + N * bias;
            // the ray (o, RT_MIN_RAY_DISTANCE, d, max_distance) under the degeneracy rules of k_rq_trace
            const bool valid = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z) &&
                               !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) && RT_MIN_RAY_DISTANCE < max_distance;
            open = !(valid && occluded<COUNT>(sc, o, d, RT_MIN_RAY_DISTANCE, max_distance, stack, cnt));
        }
    }
    const unsigned long long votes = __ballot(open);
    if (live && (lane == 0u || s == 0u)) { // the first lane of a run: the run ends with the point or with the wave
        const uint32_t len = min(S - s, (uint32_t)WAVE - lane);
        const unsigned long long run = (len == WAVE ? ~0ull : (1ull << len) - 1ull) << lane;
        const uint32_t c = (uint32_t)__popcll(votes & run);
        if (c) atomicAdd(&unoccluded[p], c);
    }
    if (COUNT) flush_counts(counters, cnt);
}

__global__ __launch_bounds__(256) void k_sq_ao_finish(const uint32_t* __restrict__ unoccluded, uint32_t n, float samples, float* __restrict__ visibility,
                                                       uint32_t* __restrict__ counts_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = unoccluded[i];
    if (visibility) visibility[i] = (float)c / samples;
    if (counts_out) counts_out[i] = c;
}

} // namespace

namespace rt {

hipError_t launch_surface_query(const DevScene& sc, const void* rays, void* out, uint32_t n, unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = lane_stack_bytes(sc);
    const float4* r = reinterpret_cast<const float4*>(rays);
    uint4* o = reinterpret_cast<uint4*>(out);
    if (counters) hipLaunchKernelGGL((k_sq_surface<true>), grid, block, lds, stream, sc, r, o, n, counters);
    else hipLaunchKernelGGL((k_sq_surface<false>), grid, block, lds, stream, sc, r, o, n, counters);
    return hipGetLastError();
}

hipError_t launch_ao(const DevScene& sc, const void* points, uint64_t first, uint32_t n, const AoParams& ap, uint32_t* unoccluded,
                     unsigned long long* counters, hipStream_t stream) {
    const uint64_t lanes = (uint64_t)n * ap.samples;
    const size_t lds = lane_stack_bytes(sc);
    const float4* p = reinterpret_cast<const float4*>(points);
    for (uint64_t g0 = 0; g0 < lanes; g0 += RT_AO_LAUNCH_LANES) {
        const uint64_t m = std::min<uint64_t>(RT_AO_LAUNCH_LANES, lanes - g0);
        const dim3 grid((uint32_t)((m + WAVE - 1) / WAVE)), block(WAVE);
        if (counters)
            hipLaunchKernelGGL((k_sq_ao<true>), grid, block, lds, stream, sc, p, first, g0, lanes, ap.samples, ap.seed, ap.max_distance, ap.bias,
                               unoccluded, counters);
        else
            hipLaunchKernelGGL((k_sq_ao<false>), grid, block, lds, stream, sc, p, first, g0, lanes, ap.samples, ap.seed, ap.max_distance, ap.bias,
                               unoccluded, counters);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_ao_finish(const uint32_t* unoccluded, uint32_t n, uint32_t samples, float* visibility, uint32_t* counts_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sq_ao_finish, dim3((n + 255u) / 256u), dim3(256), 0, stream, unoccluded, n, (float)samples, visibility, counts_out);
    return hipGetLastError();
}

} // namespace rt
