// multi_hit_walk.h — the walk that offers every candidate along a ray to a list, stated once for the two kernels that use it:
// k_rq_trace_all (ray_query.hip: rt_intersect_all's first K hits and crossing counts) and k_inside (inside.hip: the parity rays of
// rt_inside and rt_signed_distance, which count triangles with a list of capacity 0).
#ifndef RT_MULTI_HIT_WALK_H
#define RT_MULTI_HIT_WALK_H

#include "device_common.h"

namespace rtdev {

// ------------------------------------------------------------------------------------
// rt_intersect_all: the first max_hits candidates along each ray, in the order rt_intersect's rules would pick them.
// ------------------------------------------------------------------------------------
// One sphere against the ray's own range: the arithmetic of test_spheres (device_common.h) for one sphere, without its "closest so
// far".  true: `t` is the sphere's single candidate (t1 if t1 > tmin, else t2) and lies in (tmin, tmax).
__device__ __forceinline__ bool sphere_candidate(const DevSphere& s, V3 o, V3 d, float tmin, float tmax, float& t) {
    V3 oc = o - ld3(s.center);
    float a = dot(d, d);
    float b = 2.0f * dot(oc, d);
    float c = dot(oc, oc) - s.radius * s.radius;
    float disc = b * b - 4.0f * a * c;
    if (disc < 0.0f) return false;
    float sq = sqrtf(disc);
    float t1 = (-b - sq) / (2.0f * a);
    float t2 = (-b + sq) / (2.0f * a);
    t = (t1 > tmin) ? t1 : t2;
    return t > tmin && t < tmax;
}

// A lane's sorted list of its first max_hits candidates, in LDS behind the stack, lane-interleaved like it: word f of entry k of
// this lane at e[(3 * k + f) * WAVE]; the words are the bits of t, the ordering key and the record slot (DevScene::tris index, or
// the sphere index).  Key = prim_id ^ RT_PRIM_SPHERE_FLAG: sphere i -> i, triangle p -> 0x80000000 | p, so that at equal t spheres
// come before triangles and each kind is in index order.  Every candidate has t > tmin > 0, so (t bits, key) as one 64-bit unsigned
// number orders the list, and equal t means equal bits.
struct HitList {
    uint32_t* e;
    uint32_t cap, n;     // max_hits, entries held
    uint32_t total;      // candidates offered
    unsigned long long bound; // a candidate enters the list when it is below this: (tmax, 0) until the list is full, then its last entry

    __device__ __forceinline__ void init(uint32_t* lane_words, uint32_t max_hits, float tmax) {
        e = lane_words;
        cap = max_hits;
        n = total = 0u;
        bound = (unsigned long long)__float_as_uint(tmax) << 32;
    }
    // the distance the walk culls by: nothing at or beyond it can enter the list any more (at it: visit_node8's limit is above)
    __device__ __forceinline__ float bound_t() const { return __uint_as_float((uint32_t)(bound >> 32)); }
    // a candidate in (tmin, tmax): counted, and put in its place when it is among the first `cap` so far (the tail moves up by one,
    // the last entry of a full list falls out)
    __device__ __forceinline__ void offer(float t, uint32_t key, uint32_t slot) {
        total++;
        const unsigned long long c = ((unsigned long long)__float_as_uint(t) << 32) | key;
        if (cap == 0u || !(c < bound)) return;
        uint32_t j = n < cap ? n : cap - 1u;
        while (j > 0u) {
            const uint32_t pt = e[(3u * j - 3u) * WAVE], pk = e[(3u * j - 2u) * WAVE];
            if (!(c < (((unsigned long long)pt << 32) | pk))) break;
            e[(3u * j) * WAVE] = pt;
            e[(3u * j + 1u) * WAVE] = pk;
            e[(3u * j + 2u) * WAVE] = e[(3u * j - 1u) * WAVE];
            j--;
        }
        e[(3u * j) * WAVE] = __float_as_uint(t);
        e[(3u * j + 1u) * WAVE] = key;
        e[(3u * j + 2u) * WAVE] = slot;
        if (n < cap) n++;
        if (n == cap) bound = ((unsigned long long)e[(3u * cap - 3u) * WAVE] << 32) | e[(3u * cap - 2u) * WAVE];
    }
};

// The walk of traverse (device_common.h) with a list instead of one closest hit: the same groups, stack and visiting order, the
// leaves' triangles offered to the list.  The boxes are culled by the list's bound; COUNT_ALL: by tmax throughout, since every
// candidate in the range has to be counted.  A triangle has one record in the tree and a leaf one parent, so none is offered twice.
template <bool COUNT, bool COUNT_ALL>
__device__ __forceinline__ void traverse_all(const DevScene& sc, V3 o, V3 d, uint2* __restrict__ stack, HitList& list, Counts& cnt, float tmin,
                                             float tmax) {
    if (sc.n_nodes == 0) return;
    const FilterRay fr = make_filter_ray(o, d);
    const uint32_t oct = ray_octant(fr);
    const uint4* __restrict__ nodes = reinterpret_cast<const uint4*>(sc.nodes);
    uint32_t g_base = 0, g_bits = 1u | (1u << 8); // the root as the only child of a group
    int sp = 0;
    for (;;) {
        if ((g_bits & 0xFFu) == 0u) {
            if (sp == 0) break;
            sp--;
            const uint2 e = stack[sp * WAVE];
            g_base = e.x;
            g_bits = e.y;
        }
        const uint32_t i = first_slot(g_bits, oct);
        g_bits ^= 1u << i;
        const uint32_t node = g_base + (uint32_t)__popc(__builtin_amdgcn_ubfe(g_bits, 8u, i)); // inner slots below i
        if (g_bits & 0xFFu) {
            stack[sp * WAVE] = make_uint2(g_base, g_bits);
            sp++;
        }
        uint32_t cb, tb, im, lm;
        const uint32_t hm = visit_node8<COUNT>(nodes, node, fr, COUNT_ALL ? tmax : list.bound_t(), cnt, cb, tb, im, lm);
        uint32_t t = hm & lm;
        while (t) {
            const uint32_t sl = first_slot(t, oct);
            t ^= 1u << sl;
            const uint32_t first = tb + RT_DEV_LEAF_STRIDE * (uint32_t)__popc(lm & ((1u << sl) - 1u));
            uint32_t len = 1;
            for (uint32_t x = 0; x < len; x++) {
                if (COUNT) cnt.tris++;
                const float4* p = reinterpret_cast<const float4*>(sc.tris + first + x);
                float4 q0 = p[0], q1 = p[1], q2 = p[2]; // the record in three loads issued together, as test_triangle
                asm volatile("" : "+v"(q0.x), "+v"(q0.y), "+v"(q0.z), "+v"(q0.w), "+v"(q1.x), "+v"(q1.y), "+v"(q1.z), "+v"(q1.w), "+v"(q2.x), "+v"(q2.y), "+v"(q2.z), "+v"(q2.w));
                if (x == 0) len = __float_as_uint(q2.w);
                float tt;
                if (!moller_trumbore(v3(q0.x, q0.y, q0.z), v3(q0.w, q1.x, q1.y), v3(q1.z, q1.w, q2.x), o, d, tt)) continue;
                if (tt > tmin && tt < tmax) list.offer(tt, __float_as_uint(q2.z) ^ RT_PRIM_SPHERE_FLAG, first + x);
            }
        }
        g_base = cb;
        g_bits = (hm & im) | (im << 8);
    }
}

} // namespace rtdev
#endif
