// irradiance_query.hip — the kernels of rt_irradiance (include/rt_hip.h, "Irradiance queries"): the cosine-weighted hemispherical gather
// at surface points the caller supplies, E = pi / S * sum of the radiance along S directions of the frames' cosine lobe.
//
// Nothing here is new arithmetic.  A sample is rt_radiance's path (walk_path, path_walk.h) along a direction the lane draws itself
// from the point's normal: the generator's first two draws through ext_scatter's diffuse branch (device_common.h), which k_sq_ao
// (surface_query.hip) restates too, from the continuation's origin P + N * EXT_EPS.  One lane per path, one wave per block, the
// per-lane stack in LDS as in k_ps_trace.  A path leaves one 16-byte record; a second kernel, one wave per point, adds the point's
// records in sample order from zero - so there is no float atomic anywhere: the order is the result.
#include "irradiance_query.h"

#include "../../include/rt_hip.h"
#include "path_walk.h"

using namespace rtdev;

namespace {

#ifndef RT_IR_MIN_WAVES
#define RT_IR_MIN_WAVES 4 /* waves per SIMD asked of the register allocator, as RT_PS_MIN_WAVES: the same loop ("Irradiance queries") */
#endif

// k_sq_ao's point_ok: a record with a non-finite component of P or N, or with N = 0, is no point.
__device__ __forceinline__ bool point_valid(float4 pa, float4 pb) {
    return isfinite(pa.x) && isfinite(pa.y) && isfinite(pa.z) && isfinite(pb.x) && isfinite(pb.y) && isfinite(pb.z) &&
           !(pb.x == 0.0f && pb.y == 0.0f && pb.z == 0.0f);
}

// Lane g of the launch is sample g % S of point g / S of the launch's batch.  `first`: the index of the batch's first point in the
// caller's array (the seed's); `lanes` = points * S <= RT_QUERY_CHUNK.  dst[g] = (x, segments) of path g: rt_radiance's result for
// the ray (P + N * EXT_EPS, RT_MIN_RAY_DISTANCE, d, FLT_MAX) with one sample (its (0 + x) / 1 changes no bit: x is never -0).
template <bool COUNT>
__global__ __launch_bounds__(WAVE, RT_IR_MIN_WAVES) void k_ir_trace(DevScene sc, rt::PathArgs a, const float4* __restrict__ points, uint64_t first,
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
    const uint64_t p = pw + sw / S; // the point's index in the batch
    const uint32_t s = sw % S;
    // every lane stays to the end (the wave sums of the counters): a lane past the batch is "no path"
    const bool live = gw + lane < lanes;
    Counts cnt = {0u, 0u};
    SegCounts seg = {0u, 0u, 0u};
    if (live) {
        V3 radiance = v3(0.0f, 0.0f, 0.0f);
        const float4 pa = points[2 * p], pb = points[2 * p + 1];
        if (point_valid(pa, pb)) {
            const V3 P = v3(pa.x, pa.y, pa.z), N = v3(pb.x, pb.y, pb.z);
            SimpleRng rng = rng_for(a.seed + (uint32_t)(first + p), a.first_sample + s);
            const float u1 = rng.next_f32(), u2 = rng.next_f32();
            V3 w = N + unit_vector(u1, u2); // the cosine lobe of ext_scatter, N as given
            if (dot(w, w) < 1e-12f) w = N;
            const V3 d = normalize(w);
            const V3 o = P + N * EXT_EPS;
            // rt_radiance's degeneracy rule for the ray (o, RT_MIN_RAY_DISTANCE, d, FLT_MAX): a large N can leave any of these
            const bool valid = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z) &&
                               !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
            if (valid) walk_path<COUNT>(sc, rng, a.max_bounces, a.shadows != 0u, o, d, RT_MIN_RAY_DISTANCE, RT_F32_MAX, stack, cnt, seg, radiance);
        }
        dst[gw + lane] = make_uint4(__float_as_uint(radiance.x), __float_as_uint(radiance.y), __float_as_uint(radiance.z), seg.camera + seg.continuation + seg.shadow);
    }
    flush_query_counts<COUNT>(seg, cnt, lane, counters);
}

// One wave per point r of the batch.  The point's S records go by in tiles of 64: lane t of the wave reads record k0 + t (one
// coalesced KiB per tile, all in flight together) and leaves its radiance in LDS; then lane c < 3 - channel c, rt_irradiance_result's
// word c - adds the tile's values to its own sum in sample order.  So every (point, channel) sum lives in one lane from zero to the
// end, then one division and one multiply.  A lane per point instead (k_pq_reduce's shape) reads 16 bytes every S * 16 and waits for
// one load per add ("Irradiance queries").  The segment counts add up mod 2^32 across the wave.  A point that is
// no point gets zeros without a look at its records.
__global__ __launch_bounds__(WAVE) void k_ir_reduce(uint32_t S, const float4* __restrict__ points, const uint4* __restrict__ paths, uint4* __restrict__ out) {
    __shared__ float s_x[3][WAVE]; // sample-minor: lane t writes column t, the three adding lanes all read column t at once
    const uint32_t lane = threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (!point_valid(points[2 * (size_t)r], points[2 * (size_t)r + 1])) { // (uniform: the whole wave is this point's)
        if (lane == 0u) out[r] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint4* __restrict__ rec = paths + (size_t)r * S;
    const uint32_t c = lane < 3u ? lane : 0u;
    float sum = 0.0f;
    uint32_t segments = 0;
    for (uint32_t k0 = 0; k0 < S; k0 += WAVE) {
        const uint32_t tile = min(S - k0, (uint32_t)WAVE);
        if (lane < tile) {
            const uint4 x = rec[k0 + lane];
            s_x[0][lane] = __uint_as_float(x.x);
            s_x[1][lane] = __uint_as_float(x.y);
            s_x[2][lane] = __uint_as_float(x.z);
            segments += x.w;
        }
        __syncthreads();
        if (lane < 3u)
            for (uint32_t t = 0; t < tile; t++) sum = sum + s_x[c][t];
        __syncthreads(); // the next tile overwrites what was just read
    }
    const uint32_t total = (uint32_t)wave_sum(segments);
    uint32_t* __restrict__ o = reinterpret_cast<uint32_t*>(out + r);
    if (lane < 3u) o[lane] = __float_as_uint(sum * (3.1415927f / (float)S));
    if (lane == 0u) o[3] = total;
}

} // namespace

namespace rt {

hipError_t launch_irradiance_query(const DevScene& sc, const PathArgs& a, const void* points, uint64_t first, uint32_t n, void* scratch, void* out, bool count,
                                   unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t lds = lane_stack_bytes(sc);
    const uint32_t lanes = n * a.samples;                                          // <= RT_QUERY_CHUNK (the caller's chunking)
    const float4* p = reinterpret_cast<const float4*>(points);
    uint4* dst = reinterpret_cast<uint4*>(scratch);
    const dim3 grid((lanes + WAVE - 1) / WAVE), block(WAVE);
    if (count) hipLaunchKernelGGL((k_ir_trace<true>), grid, block, lds, stream, sc, a, p, first, lanes, dst, counters);
    else hipLaunchKernelGGL((k_ir_trace<false>), grid, block, lds, stream, sc, a, p, first, lanes, dst, counters);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ir_reduce, dim3(n), dim3(WAVE), 0, stream, a.samples, p, dst, reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

} // namespace rt
