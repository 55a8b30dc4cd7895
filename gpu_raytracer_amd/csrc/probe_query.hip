// probe_query.hip — the kernels of rt_radiance_sh (include/rt_hip.h, "Probe queries"): the radiance field at points the caller
// supplies, as 9 real spherical-harmonic coefficients per colour channel.
//
// Nothing here is new arithmetic but the basis.  A sample is rt_radiance's path (walk_path, path_walk.h) along a direction the lane
// draws itself: the generator's first two draws through unit_vector, the two draws RT_PATH_CAMERA_DRAWS names.  One lane per path, one
// wave per block, the per-lane stack in LDS as in k_pq_trace.  A path leaves one 16-byte record; a second kernel, one lane per (probe,
// coefficient, channel), draws each direction again and adds radiance * basis in sample order from zero - so there is no float
// atomic anywhere: the order is the result.
#include "probe_query.h"

#include "../../include/rt_hip.h"
#include "path_walk.h"

using namespace rtdev;

namespace {

#ifndef RT_PS_MIN_WAVES
#define RT_PS_MIN_WAVES 4 /* waves per SIMD asked of the register allocator, as RT_PQ_MIN_WAVES: the same loop ("Probe queries") */
#endif

__device__ __forceinline__ bool probe_valid(float4 pr) { return isfinite(pr.x) && isfinite(pr.y) && isfinite(pr.z); }

// Direction k of the probe whose index in the caller's array is i, and the generator after its two draws.
__device__ __forceinline__ V3 probe_direction(const rt::PathArgs& a, uint32_t i, uint32_t k, SimpleRng& rng) {
    rng = rng_for(a.seed + i, a.first_sample + k);
    const float u1 = rng.next_f32();
    const float u2 = rng.next_f32();
    return unit_vector(u1, u2);
}

// The real SH basis to L2 (Ramamoorthi and Hanrahan 2001) as rt_hip.h writes it: every operation one f32 rounding, nothing fused.
__device__ __forceinline__ float sh_basis(uint32_t j, V3 d) {
    switch (j) {
        case 0: return 0.2820948f;
        case 1: return 0.4886025f * d.y;
        case 2: return 0.4886025f * d.z;
        case 3: return 0.4886025f * d.x;
        case 4: return 1.0925484f * (d.x * d.y);
        case 5: return 1.0925484f * (d.y * d.z);
        case 6: return 0.31539157f * (3.0f * (d.z * d.z) - 1.0f);
        case 7: return 1.0925484f * (d.x * d.z);
        default: return 0.5462742f * (d.x * d.x - d.y * d.y);
    }
}

// Lane g of the launch is sample g % S of probe g / S of the launch's batch.  `first`: the index of the batch's first probe in the
// caller's array (the seed's); `lanes` = probes * S <= RT_QUERY_CHUNK.  dst[g] = (x, segments) of path g: rt_radiance's result for
// the ray (position, RT_MIN_RAY_DISTANCE, d, FLT_MAX) with one sample (its (0 + x) / 1 changes no bit: x is never -0).
template <bool COUNT>
__global__ __launch_bounds__(WAVE, RT_PS_MIN_WAVES) void k_ps_trace(DevScene sc, rt::PathArgs a, const float4* __restrict__ probes, uint64_t first,
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
    const uint64_t p = pw + sw / S; // the probe's index in the batch
    const uint32_t s = sw % S;
    // every lane stays to the end (the wave sums of the counters): a lane past the batch is "no path"
    const bool live = gw + lane < lanes;
    Counts cnt = {0u, 0u};
    SegCounts seg = {0u, 0u, 0u};
    if (live) {
        V3 radiance = v3(0.0f, 0.0f, 0.0f);
        const float4 pr = probes[p];
        if (probe_valid(pr)) {
            SimpleRng rng;
            const V3 d = probe_direction(a, (uint32_t)(first + p), s, rng);
            // rt_radiance's degeneracy rule for the direction (its components are finite: r, z and the polynomials are)
            if (!(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f))
                walk_path<COUNT>(sc, rng, a.max_bounces, a.shadows != 0u, v3(pr.x, pr.y, pr.z), d, RT_MIN_RAY_DISTANCE, RT_F32_MAX, stack, cnt, seg, radiance);
        }
        dst[gw + lane] = make_uint4(__float_as_uint(radiance.x), __float_as_uint(radiance.y), __float_as_uint(radiance.z), seg.camera + seg.continuation + seg.shadow);
    }
    flush_query_counts<COUNT>(seg, cnt, lane, counters);
}

// One wave per probe r of the batch.  The probe's S records go by in tiles of 64: lane t of the wave draws direction k0 + t again,
// reads record k0 + t (one coalesced KiB per tile) and leaves the sample's radiance and its nine basis values in LDS; then lane l < 27
// - coefficient l / 3, channel l % 3, rt_sh9's word l - adds the tile's products to its own sum in sample order, each term one
// product.  So every (probe, coefficient, channel) sum lives in one lane from zero to the end, then one division and one multiply.
// The loads of a tile are in flight together, where a lane that draws, reads and adds sample by sample waits for one load per add
// ("Probe queries").  The segment counts add up mod 2^32 across the wave.  A probe that is no probe gets zeros without a look at its records.
__global__ __launch_bounds__(WAVE) void k_ps_project(rt::PathArgs a, const float4* __restrict__ probes, uint64_t first, const uint4* __restrict__ paths,
                                                      float* __restrict__ out) {
    __shared__ float s_x[3][WAVE], s_y[9][WAVE]; // sample-minor: lane t writes column t, the adding lanes all read column t at once
    const uint32_t lane = threadIdx.x;
    const uint32_t r = blockIdx.x;
    const uint32_t S = a.samples;
    float* __restrict__ o = out + (size_t)r * 28u;
    if (!probe_valid(probes[r])) { // (uniform: the whole wave is this probe's)
        if (lane < 28u) o[lane] = 0.0f;
        return;
    }
    const uint4* __restrict__ rec = paths + (size_t)r * S;
    const uint32_t i = (uint32_t)(first + r);
    const uint32_t j = lane / 3u, c = lane - j * 3u;
    float sum = 0.0f;
    uint32_t segments = 0;
    for (uint32_t k0 = 0; k0 < S; k0 += WAVE) {
        const uint32_t tile = min(S - k0, (uint32_t)WAVE);
        if (lane < tile) {
            SimpleRng rng;
            const V3 d = probe_direction(a, i, k0 + lane, rng);
            const uint4 x = rec[k0 + lane];
            s_x[0][lane] = __uint_as_float(x.x);
            s_x[1][lane] = __uint_as_float(x.y);
            s_x[2][lane] = __uint_as_float(x.z);
            segments += x.w;
#pragma unroll
            for (uint32_t q = 0; q < 9u; q++) s_y[q][lane] = sh_basis(q, d);
        }
        __syncthreads();
        if (lane < 27u)
            for (uint32_t t = 0; t < tile; t++) sum = sum + s_x[c][t] * s_y[j][t];
        __syncthreads(); // the next tile overwrites what was just read
    }
    const uint32_t total = (uint32_t)wave_sum(segments);
    if (lane < 27u) o[lane] = sum * (12.566371f / (float)S);
    if (lane == 0u) reinterpret_cast<uint32_t*>(o)[27] = total;
}

} // namespace

namespace rt {

hipError_t launch_probe_query(const DevScene& sc, const PathArgs& a, const void* probes, uint64_t first, uint32_t n, void* scratch, void* out, bool count,
                              unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t lds = lane_stack_bytes(sc);
    const uint32_t lanes = n * a.samples;                                          // <= RT_QUERY_CHUNK (the caller's chunking)
    const float4* p = reinterpret_cast<const float4*>(probes);
    uint4* dst = reinterpret_cast<uint4*>(scratch);
    const dim3 grid((lanes + WAVE - 1) / WAVE), block(WAVE);
    if (count) hipLaunchKernelGGL((k_ps_trace<true>), grid, block, lds, stream, sc, a, p, first, lanes, dst, counters);
    else hipLaunchKernelGGL((k_ps_trace<false>), grid, block, lds, stream, sc, a, p, first, lanes, dst, counters);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ps_project, dim3(n), dim3(WAVE), 0, stream, a, p, first, dst, reinterpret_cast<float*>(out));
    return hipGetLastError();
}

} // namespace rt
