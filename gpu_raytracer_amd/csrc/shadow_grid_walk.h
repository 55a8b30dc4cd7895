// shadow_grid_walk.h — the device side of the light grids (shadow_grid.h): how a shadow segment looks up its cell and walks the cell's
// list, stated once for the two kernels that do it: k_wf_shadow_grid (wavefront.hip: the frames' path vertices) and k_dl_direct
// (direct_light.hip: rt_direct_light's points).  Also the staging of the lights in LDS that both share with the shading stages.
#ifndef RT_SHADOW_GRID_WALK_H
#define RT_SHADOW_GRID_WALK_H

#include "device_common.h"
#include "shadow_grid.h"

namespace rtdev {

// The shading stages are bound by memory latency, not arithmetic (22 % VALU busy, 83 % of the wave time in s_waitcnt):
// what counts is the number of DEPENDENT round trips per path.  Lights come from LDS (staged once per block), and
// each group of per-path loads is issued together: RT_KEEP4 pins the loaded values at one point so the
// compiler cannot split a record by first use and sink the later words behind a branch (each a further round trip).
#define RT_KEEP4(v) asm volatile("" : "+v"((v).x), "+v"((v).y), "+v"((v).z), "+v"((v).w))
__device__ __forceinline__ void stage_lights(DevLight* __restrict__ s_lights, const DevScene& sc) {
    const uint32_t words = sc.n_lights * (uint32_t)(sizeof(DevLight) / 4);
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(sc.lights);
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_lights);
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

#ifndef RT_WF_GRID_WALK
#define RT_WF_GRID_WALK 31 /* entries a segment looks at before it is handed on (12 while a long walk held its whole wave up: rounds 2-3) */
#endif
static_assert(EXT_EPS == RT_SG_EXT_EPS, "the light grids' dilation is derived from the shadow segments' origin offset");
static_assert(RT_WF_GRID_WALK < RT_SG_SORTED_PREFIX, "a walk may only look at the ordered part of a list");
// One shadow segment (vertex `point` / `normal` toward light li) against the head of its cell's list: what the cell's own 128-byte block
// holds (header, two entries, the key of the third).  Outcome GRID_VISIBLE / GRID_OCCLUDED / GRID_FORWARD (left to the BVH), or
// GRID_PENDING: the list goes on beyond the block and the segment has not met its occluder or its end yet - `pend` is then what the
// second part of the walk (grid_walk_on) needs.
enum : uint32_t { GRID_VISIBLE = 0u, GRID_OCCLUDED = 1u, GRID_FORWARD = 2u, GRID_PENDING = 3u };
struct GridPending {
    V3 o, d;
    float dist, limit;
    uint32_t at;    // the next entry, as an index into the grid's overflow array
    uint32_t i, count; // ... which is entry i of `count`
};
static_assert(RT_SG_BLOCK_ENTRIES == 2u, "grid_segment_head tests the block's two entries by name");
// The grids' arrays are reached through pointers that come from the table staged in LDS, so the compiler cannot tell their address space
// and would read them with flat loads (each waited for with the LDS counter as well); they are device allocations: global loads.
typedef uint32_t sg_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 sg_ldg4(const uint4* p) {
    const sg_u32x4 v = *reinterpret_cast<const __attribute__((address_space(1))) sg_u32x4*>(reinterpret_cast<uintptr_t>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
template <bool COUNT>
__device__ __forceinline__ uint32_t grid_segment_head(const DevScene& sc, const DevLight& light, const DevShadowGrid& g, V3 point, V3 normal, GridPending& pend,
                                                      uint32_t& n_tests, uint32_t& n_entries) {
    V3 d;
    float dist;
    shadow_segment(light, point, d, dist);
    const V3 o = point + normal * EXT_EPS;
    Hit hit;
    hit.t = dist;
    hit.prim = RT_PRIM_MISS;
    hit.slot = 0;
    test_spheres(sc, o, d, hit, RT_MIN_RAY_DISTANCE);
    if (hit.prim != RT_PRIM_MISS) return GRID_OCCLUDED; // by a sphere: nothing left to do
    const uint32_t kind = g.kind;
    uint32_t cell = 0xFFFFFFFFu; // no cell: an empty list
    float limit = 0.0f;
    if (kind == RT_SG_KIND_CUBE) {
        // the direction from the light toward the vertex picks the face (largest component) and the cell (the other two over it)
        const float wx = -d.x, wy = -d.y, wz = -d.z;
        const float ax = fabsf(wx), ay = fabsf(wy), az = fabsf(wz);
        const uint32_t a = (ax >= ay && ax >= az) ? 0u : (ay >= az ? 1u : 2u);
        const float wa = a == 0u ? wx : (a == 1u ? wy : wz), wb_ = a == 0u ? wy : (a == 1u ? wz : wx), wc = a == 0u ? wz : (a == 1u ? wx : wy);
        const float inv = __builtin_amdgcn_rcpf(fabsf(wa)); // (an ulp either way is far inside the lists' margin)
        const float fu = (wb_ * inv + 1.0f) * g.scale, fv = (wc * inv + 1.0f) * g.scale;
        const uint32_t top = g.res - 1u;
        const uint32_t ix = min((uint32_t)max((int)floorf(fu), 0), top), iy = min((uint32_t)max((int)floorf(fv), 0), top);
        cell = ((2u * a + (wa < 0.0f ? 1u : 0u)) * g.res + iy) * g.res + ix;
        limit = dist + g.limit_margin;
    } else if (kind == RT_SG_KIND_ORTHO) {
        const float fu = (dot(o, ld3(g.axis_u)) - g.u0) * g.scale, fv = (dot(o, ld3(g.axis_v)) - g.v0) * g.scale;
        const float r = (float)g.res;
        if (fu >= 0.0f && fu < r && fv >= 0.0f && fv < r) cell = (uint32_t)fv * g.res + (uint32_t)fu; // outside: nothing projects there
        limit = (g.key_top - dot(o, ld3(g.axis_w))) + g.limit_margin;
    } else {
        return GRID_FORWARD; // a light without a grid
    }
    // the cell's block: header and the list's first entry in the first half of its 128-byte line, the second entry in the other half
    if (cell == 0xFFFFFFFFu && g.near_begin == g.near_end) return GRID_VISIBLE;
    uint4 hd = make_uint4(0u, 0u, 0x7F800000u, 0u), q0 = hd, q1 = hd, q2 = hd;
    const uint4* __restrict__ blk = g.blocks + (size_t)(cell == 0xFFFFFFFFu ? 0u : cell) * RT_SG_BLOCK_QUADS;
    if (cell != 0xFFFFFFFFu) {
        hd = sg_ldg4(blk);
        q0 = sg_ldg4(blk + 1), q1 = sg_ldg4(blk + 2), q2 = sg_ldg4(blk + 3);
        RT_KEEP4(hd);
        RT_KEEP4(q0);
        RT_KEEP4(q1);
        RT_KEEP4(q2);
    }
    const uint32_t count = hd.x;
    if (count > g.heavy) return GRID_FORWARD;
    const uint4* __restrict__ ovf = g.overflow; // 48-byte entries: {key, v0} {e1, e2.x} {e2.yz, record, 0}
    // triangles too close to the light for a bounded dilation: tested by every segment of the light (normally none)
    for (uint32_t k = g.near_begin; k < g.near_end; k++) {
        const uint4 n0 = sg_ldg4(ovf + 3 * (size_t)k), n1 = sg_ldg4(ovf + 3 * (size_t)k + 1), n2 = sg_ldg4(ovf + 3 * (size_t)k + 2);
        if (COUNT) n_tests++;
        float t;
        if (moller_trumbore(v3(__uint_as_float(n0.y), __uint_as_float(n0.z), __uint_as_float(n0.w)), v3(__uint_as_float(n1.x), __uint_as_float(n1.y), __uint_as_float(n1.z)),
                            v3(__uint_as_float(n1.w), __uint_as_float(n2.x), __uint_as_float(n2.y)), o, d, t) &&
            t > RT_MIN_RAY_DISTANCE && t < dist)
            return GRID_OCCLUDED;
    }
    // entries come nearest to the light first: a key beyond the segment's own end means every later triangle lies beyond it too
    if (count == 0u || !(__uint_as_float(q0.x) < limit)) return GRID_VISIBLE;
    float t;
    if (COUNT) n_entries++, n_tests++;
    // the acceptance of test_triangle for a segment that has hit nothing yet: 1e-5 < t < its length
    if (moller_trumbore(v3(__uint_as_float(q0.y), __uint_as_float(q0.z), __uint_as_float(q0.w)), v3(__uint_as_float(q1.x), __uint_as_float(q1.y), __uint_as_float(q1.z)),
                        v3(__uint_as_float(q1.w), __uint_as_float(q2.x), __uint_as_float(q2.y)), o, d, t) &&
        t > RT_MIN_RAY_DISTANCE && t < dist)
        return GRID_OCCLUDED;
    if (count == 1u) return GRID_VISIBLE;
    q0 = sg_ldg4(blk + 4), q1 = sg_ldg4(blk + 5), q2 = sg_ldg4(blk + 6);
    if (!(__uint_as_float(q0.x) < limit)) return GRID_VISIBLE;
    if (COUNT) n_entries++, n_tests++;
    if (moller_trumbore(v3(__uint_as_float(q0.y), __uint_as_float(q0.z), __uint_as_float(q0.w)), v3(__uint_as_float(q1.x), __uint_as_float(q1.y), __uint_as_float(q1.z)),
                        v3(__uint_as_float(q1.w), __uint_as_float(q2.x), __uint_as_float(q2.y)), o, d, t) &&
        t > RT_MIN_RAY_DISTANCE && t < dist)
        return GRID_OCCLUDED;
    if (count == 2u || !(__uint_as_float(hd.z) < limit)) return GRID_VISIBLE; // (the third entry's key travels in the header)
    pend.o = o, pend.d = d, pend.dist = dist, pend.limit = limit;
    pend.at = hd.y, pend.i = 2u, pend.count = count;
    return GRID_PENDING;
}
// ... and the list beyond the block, at most `trips` entries further: entries 2, 3, ... follow each other in the overflow array, each is
// fetched when the one before it has decided nothing.  GRID_PENDING again: `pend` has moved on.
template <bool COUNT>
__device__ __forceinline__ uint32_t grid_walk_on(const DevShadowGrid& g, GridPending& pend, uint32_t trips, uint32_t& n_tests, uint32_t& n_entries) {
    const uint4* __restrict__ ovf = g.overflow;
    for (uint32_t k = 0; k < trips; k++) {
        const size_t at = 3 * (size_t)pend.at;
        uint4 q0 = sg_ldg4(ovf + at), q1 = sg_ldg4(ovf + at + 1), q2 = sg_ldg4(ovf + at + 2);
        RT_KEEP4(q0);
        RT_KEEP4(q1);
        RT_KEEP4(q2);
        if (!(__uint_as_float(q0.x) < pend.limit)) return GRID_VISIBLE;
        if (COUNT) n_entries++, n_tests++;
        float t;
        if (moller_trumbore(v3(__uint_as_float(q0.y), __uint_as_float(q0.z), __uint_as_float(q0.w)), v3(__uint_as_float(q1.x), __uint_as_float(q1.y), __uint_as_float(q1.z)),
                            v3(__uint_as_float(q1.w), __uint_as_float(q2.x), __uint_as_float(q2.y)), pend.o, pend.d, t) &&
            t > RT_MIN_RAY_DISTANCE && t < pend.dist)
            return GRID_OCCLUDED;
        pend.at++;
        pend.i++;
        if (pend.i >= pend.count) return GRID_VISIBLE;
        if (pend.i >= RT_WF_GRID_WALK) return GRID_FORWARD;
    }
    return GRID_PENDING;
}

} // namespace rtdev
#endif
