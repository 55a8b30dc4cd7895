// ray_query.hip — the kernels of the ray queries of include/rt_hip.h: closest hit (rt_intersect), any hit (rt_occluded) and the
// first K hits (rt_intersect_all) of rays the caller supplies, and the frames' camera rays as such records (rt_camera_rays).
//
// A query ray is walked by the code the frames use (device_common.h: test_spheres, traverse, occluded), with the ray's own
// range: the walk starts from hit = (tmax, miss) and accepts tmin < t < hit.t, so the frames' strict compare and tie rule give
// the range semantics.  One lane per ray, one wave per block, the per-lane stack in LDS as in k_render_reference.
#include "ray_query.h"

#include <algorithm>

#include "device_common.h"

using namespace rtdev;

namespace {

// One rt_ray (ox oy oz tmin | dx dy dz tmax) per lane -> one rt_hit (t u v prim_id) or, ANY_HIT, one byte.
template <bool COUNT, bool ANY_HIT>
__global__ __launch_bounds__(WAVE) void k_rq_trace(DevScene sc, const float4* __restrict__ rays, void* __restrict__ out, uint32_t n,
                                                    unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // (DevScene::stack_entries / 2 + 1) * 64 64-bit entries
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
    if (COUNT) {
        atomicAdd(&counters[RT_CNT_NODE_VISITS], (unsigned long long)cnt.nodes);
        atomicAdd(&counters[RT_CNT_TRI_TESTS], (unsigned long long)cnt.tris);
    }
}

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
    list.init(reinterpret_cast<uint32_t*>(s_stack + (size_t)(sc.stack_entries / 2u + 1u) * WAVE) + threadIdx.x, max_hits, tmax);
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
    if (COUNT) {
        atomicAdd(&counters[RT_CNT_NODE_VISITS], (unsigned long long)cnt.nodes);
        atomicAdd(&counters[RT_CNT_TRI_TESTS], (unsigned long long)cnt.tris);
    }
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
    const size_t lds = (size_t)(sc.stack_entries / 2u + 1u) * WAVE * sizeof(uint2); // one entry per level, as lds_bytes in kernels.hip
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
    const size_t lds = (size_t)(sc.stack_entries / 2u + 1u) * WAVE * sizeof(uint2) + (size_t)max_hits * 3u * WAVE * sizeof(uint32_t); // stack + list
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
