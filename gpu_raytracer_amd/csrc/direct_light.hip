// direct_light.hip — the kernel of rt_direct_light (include/rt_hip.h, "Direct-light queries"): the light the scene's lights deliver to
// points the caller supplies, with shadows.
//
// Nothing here is new arithmetic.  The radiance is ext_light_sum (device_common.h), the statement the frames' path vertex uses; a
// shadow segment is shadow_segment's direction and length from P + N * bias, under k_rq_trace's degeneracy rules; it is answered by
// the light's triangle list (shadow_grid_walk.h: grid_segment_head, grid_walk_on - the walk of k_wf_shadow_grid) when the device holds
// grids and the point is one the lists are supersets for, and by occluded<> (the walk of rt_occluded) otherwise and whenever a list
// hands the segment on.  "Is any triangle accepted" does not depend on which superset of the accepted triangles is tested, so both
// give the same bit.  One lane per point, one wave per block, the per-lane stack in LDS as in k_rq_trace, the lights and the grid
// table staged behind it; the wave goes through the lights together, as k_wf_shadow_grid does, and then walks what is left to the
// tree densely, a segment per lane.
#include "direct_light.h"

#include "device_common.h"
#include "shadow_grid_walk.h"

using namespace rtdev;

namespace {

__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// The degeneracy rules of k_rq_trace for the segment (o, RT_MIN_RAY_DISTANCE, d, dist).
__device__ __forceinline__ bool segment_valid(V3 o, V3 d, float dist) {
    return finite3(o) && finite3(d) && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) && RT_MIN_RAY_DISTANCE < dist;
}

#ifndef RT_DL_MIN_WAVES
#define RT_DL_MIN_WAVES 6 /* waves per SIMD asked of the register allocator: 80 VGPRs without scratch; 7 (72 VGPRs) spills 13 registers.  The
                             counting variant carries five more counters and spills at 6, so it asks for two waves less (97 VGPRs; at 5 it still spills 6) */
#endif
// One rt_surface_point (px py pz prim_id | nx ny nz material_id) per lane -> one rt_lighting (r g b lit_mask).
template <bool COUNT>
__global__ __launch_bounds__(WAVE, COUNT ? RT_DL_MIN_WAVES - 2 : RT_DL_MIN_WAVES) void k_dl_direct(DevScene sc, rt::DirectLightArgs a, const float4* __restrict__ points, uint4* __restrict__ out,
                                                     uint32_t n, unsigned long long* __restrict__ counters) {
    // lane_stack_entries * 64 64-bit stack entries, then n_lights DevLight, then (a.grids) n_lights DevShadowGrid
    extern __shared__ uint2 s_stack[];
    __shared__ uint32_t s_upto[WAVE], s_occ[WAVE];
    const uint32_t lane = threadIdx.x;
    uint2* stack = s_stack + lane;
    DevLight* s_lights = reinterpret_cast<DevLight*>(s_stack + (size_t)lane_stack_entries(sc) * WAVE);
    DevShadowGrid* s_grids = reinterpret_cast<DevShadowGrid*>(s_lights + sc.n_lights);
    stage_lights(s_lights, sc);
    if (a.grids) {
        const uint32_t words = sc.n_lights * (uint32_t)(sizeof(DevShadowGrid) / 4);
        const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(a.grids);
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_grids);
        for (uint32_t k = lane; k < words; k += WAVE) dst[k] = src[k];
        __syncthreads();
    }
    // every lane stays to the end (the wave sums of the counters): a lane past the batch is "not a point"
    const uint32_t i = blockIdx.x * WAVE + lane;
    float4 pa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pb = pa;
    if (i < n) {
        pa = points[2 * (size_t)i], pb = points[2 * (size_t)i + 1];
        RT_KEEP4(pa);
        RT_KEEP4(pb);
    }
    const V3 P = v3(pa.x, pa.y, pa.z), N = v3(pb.x, pb.y, pb.z);
    const uint32_t material_id = __float_as_uint(pb.w);
    const bool is_point = i < n && finite3(P) && finite3(N) && !(N.x == 0.0f && N.y == 0.0f && N.z == 0.0f);
    const bool shade = is_point && material_id < sc.n_materials;
    DevMaterial m = {};
    if (shade) m = sc.materials[material_id];
    const bool shadows = a.shadows != 0u;
    // the lists are supersets for unit normals and points in the widened box only (direct_light.h); the host has checked the bias
    const bool eligible = a.grids != nullptr && shade && fabsf(dot(N, N) - 1.0f) <= 1.0e-5f && P.x >= a.lo[0] && P.x <= a.hi[0] && P.y >= a.lo[1] &&
                          P.y <= a.hi[1] && P.z >= a.lo[2] && P.z <= a.hi[2];
    const V3 o = P + N * a.bias;
    uint32_t nonzero = 0, occ = 0, walk = 0; // per light: its contribution is not zero / its segment is occluded / ... is left to the tree
    uint32_t n_tests = 0, n_entries = 0, n_answered = 0;
    Counts cnt = {0u, 0u};
    for (uint32_t li = 0; li < sc.n_lights; li++) {
        V3 sdir = v3(0.0f, 0.0f, 0.0f);
        float sdist = 0.0f;
        bool nz = false;
        if (shade) nz = needs_shadow_segment(light_contribution(s_lights[li], m, P, N, sdir, sdist));
        if (nz) nonzero |= 1u << li;
        const bool mine = nz && shadows;
        if (!eligible) { // (without grids the loop ends here for the whole wave)
            if (mine) walk |= 1u << li;
            continue;
        }
        if (__ballot(mine) == 0ull) continue;
        if (mine && segment_valid(o, sdir, sdist)) { // (a degenerate segment is not occluded)
            GridPending pd = {};
            uint32_t outcome = grid_segment_head<COUNT>(sc, s_lights[li], s_grids[li], P, N, pd, n_tests, n_entries);
            if (outcome == GRID_PENDING) outcome = grid_walk_on<COUNT>(s_grids[li], pd, RT_WF_GRID_WALK, n_tests, n_entries);
            if (COUNT && outcome <= GRID_OCCLUDED) n_answered++;
            if (outcome == GRID_OCCLUDED) occ |= 1u << li;
            if (outcome >= GRID_FORWARD) walk |= 1u << li;
        }
    }
    // The segments left to the tree, densely: a point has segments toward some of the lights only (three of five on the sponza-like
    // scene), so a wave that walked them light by light would keep its lanes 60 % busy and wait for each light's longest walk.  Segment s
    // of the wave (points in lane order, a point's lights in index order - the order of a caller's composed batch) goes to lane s % 64 of
    // round s / 64: the lane finds its point by the wave's running segment count, fetches it by shuffle and sets the light's bit in the
    // point's word.
    {
        uint32_t upto = (uint32_t)__popc(walk); // segments of the lanes up to and including this one
        for (uint32_t off = 1; off < WAVE; off <<= 1) {
            const uint32_t t = __shfl_up(upto, off, WAVE);
            if (lane >= off) upto += t;
        }
        const uint32_t total = __shfl(upto, WAVE - 1, WAVE);
        if (total) { // (wave-uniform)
            s_upto[lane] = upto;
            s_occ[lane] = 0u;
            __syncthreads();
            for (uint32_t first = 0; first < total; first += WAVE) {
                const uint32_t s = first + lane;
                uint32_t src = 0; // the first lane whose count exceeds s (63 for a lane without a segment in this round)
                for (uint32_t step = WAVE / 2; step; step >>= 1)
                    if (s_upto[src + step - 1u] <= s) src += step;
                uint32_t rest = __shfl(walk, src, WAVE);
                const V3 sp = v3(__shfl(P.x, src, WAVE), __shfl(P.y, src, WAVE), __shfl(P.z, src, WAVE));
                const V3 so = v3(__shfl(o.x, src, WAVE), __shfl(o.y, src, WAVE), __shfl(o.z, src, WAVE));
                if (s < total) {
                    for (uint32_t k = s - (src ? s_upto[src - 1u] : 0u); k; k--) rest &= rest - 1u; // drop the point's earlier segments
                    const uint32_t li = (uint32_t)__ffs(rest) - 1u;
                    V3 sdir;
                    float sdist;
                    shadow_segment(s_lights[li], sp, sdir, sdist);
                    if (segment_valid(so, sdir, sdist) && occluded<COUNT>(sc, so, sdir, RT_MIN_RAY_DISTANCE, sdist, stack, cnt)) atomicOr(&s_occ[src], 1u << li);
                }
            }
            __syncthreads();
            occ |= s_occ[lane];
        }
    }
    uint4 r = make_uint4(0u, 0u, 0u, 0u); // not a point
    if (shade) {
        const V3 rad = ext_light_sum(s_lights, sc.n_lights, m, P, N, a.ambient != 0u, shadows, [&](uint32_t li, V3, float) { return ((occ >> li) & 1u) == 0u; });
        r = make_uint4(__float_as_uint(rad.x), __float_as_uint(rad.y), __float_as_uint(rad.z), nonzero & ~occ);
    } else if (is_point) { // an invalid material id: what the frames show for it
        const V3 c = RT_MAGENTA();
        r = make_uint4(__float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(c.z), 0u);
    }
    if (i < n) out[i] = r;
    const unsigned long long segments = wave_sum(shadows ? (uint32_t)__popc(nonzero) : 0u);
    if (lane == 0 && segments) atomicAdd(&counters[RT_CNT_SHADOW], segments);
    if (COUNT) {
        const unsigned long long n0 = wave_sum(cnt.nodes), n1 = wave_sum(cnt.tris + n_tests), ga = wave_sum(n_answered), ge = wave_sum(n_entries);
        if (lane == 0) {
            atomicAdd(&counters[RT_CNT_NODE_VISITS], n0);
            atomicAdd(&counters[RT_CNT_TRI_TESTS], n1);
            atomicAdd(&counters[RT_CNT_DL_GRID_ANSWERED], ga);
            atomicAdd(&counters[RT_CNT_DL_GRID_ENTRIES], ge);
        }
    }
}

} // namespace

namespace rt {

hipError_t launch_direct_light(const DevScene& sc, const DirectLightArgs& a, const void* points, void* out, uint32_t n, bool count,
                               unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    const size_t lds = lane_stack_bytes(sc)
                       + (size_t)sc.n_lights * (sizeof(DevLight) + (a.grids ? sizeof(DevShadowGrid) : 0));
    const float4* p = reinterpret_cast<const float4*>(points);
    uint4* o = reinterpret_cast<uint4*>(out);
    if (count) hipLaunchKernelGGL((k_dl_direct<true>), grid, block, lds, stream, sc, a, p, o, n, counters);
    else hipLaunchKernelGGL((k_dl_direct<false>), grid, block, lds, stream, sc, a, p, o, n, counters);
    return hipGetLastError();
}

} // namespace rt
