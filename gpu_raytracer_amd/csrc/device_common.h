// device_common.h — device-side building blocks shared by kernels.hip (megakernels) and wavefront.hip
// (queue-based pipeline): vector math in the reference's operation order, ray generation, sphere and
// Möller–Trumbore tests, the quantised 8-wide BVH visit and group walk, the reference's shading, and the extended mode's
// RNG / sampling helpers and the ONE statement of its path vertex (ext_sample_ray, ext_light_sum, ext_leave_vertex, ext_scatter)
// that its three implementations call.  Everything is __forceinline__; both translation units are compiled with
// -ffp-contract=off so the arithmetic that decides hits and colours is identical in all kernels.
#ifndef RT_DEVICE_COMMON_H
#define RT_DEVICE_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_layout.h"

namespace rtdev {

#define RT_MIN_RAY_DISTANCE 0.00001f
#define RT_F32_MAX 3.402823466e+38f
#define RT_PI 3.14159265358979323846f
#define WAVE 64


struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 ld3(const float* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
// glam scalar-math order: (x*x + y*y) + z*z
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return v3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y);
}
__device__ __forceinline__ float length(V3 a) { return sqrtf(dot(a, a)); }
__device__ __forceinline__ V3 normalize(V3 a) { return a * (1.0f / length(a)); }

// The two colours every mode shares: what a segment that leaves the scene sees (process_wavefront_ray, wavefront.rs:146-151) and
// what a hit with a material index out of range shows (lib.rs:307-309).
__device__ __forceinline__ V3 RT_SKY() { return v3(0.1f, 0.2f, 0.3f); }
__device__ __forceinline__ V3 RT_MAGENTA() { return v3(1.0f, 0.0f, 1.0f); }

// IEEE half round trip, round-to-nearest-even (shader/src/lighting.rs:125-127)
__device__ __forceinline__ float f16_round_trip(float v) {
    _Float16 h = (_Float16)v; // v_cvt_f16_f32, RNE in the default mode
    return (float)h;
}

struct Hit {
    float t;
    uint32_t prim; // RT_PRIM_MISS, RT_PRIM_SPHERE_FLAG | i, or original triangle index
    uint32_t slot; // index into DevScene::tris for triangle hits
};

struct Counts {
    uint32_t nodes, tris;
};
// a lane's walk counts into the query counters
__device__ __forceinline__ void flush_counts(unsigned long long* counters, const Counts& cnt) {
    atomicAdd(&counters[RT_CNT_NODE_VISITS], (unsigned long long)cnt.nodes);
    atomicAdd(&counters[RT_CNT_TRI_TESTS], (unsigned long long)cnt.tris);
}

// The per-lane stack of the one-wave-per-block kernels, in dynamic LDS, lane-interleaved.  The one-ray-per-lane walks and the volume
// queries' group_walk park only the group of siblings still to visit (a node's leaves are tested right after its visit), one entry
// per level: half of DevScene::stack_entries, which is sized for the queue pipeline's walk (it also parks postponed leaf groups).  At
// 512 bytes per entry and wave this decides how many waves fit a CU: depth 11 -> 6 KB, 26 waves per CU.  What a kernel keeps behind
// the stack (a hit list, the lights) starts lane_stack_entries * WAVE entries in.
__host__ __device__ __forceinline__ uint32_t lane_stack_entries(const DevScene& sc) { return sc.stack_entries / 2u + 1u; }
__host__ __device__ __forceinline__ size_t lane_stack_bytes(const DevScene& sc) { return (size_t)lane_stack_entries(sc) * WAVE * sizeof(uint2); }

// ------------------------------------------------------------------------------------
// Ray generation.  Ray::from_screen_coordinates (shader/src/ray.rs:22-53) for mode 0,
// generate_camera_ray (shader/src/wavefront.rs:75-112) for mode 1.  fov_scale / aspect /
// right / true_up are per-frame constants computed on the host in the same order.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void camera_ray(const DevCamera& cam, float sx, float sy, bool wavefront, V3& o, V3& d) {
    float u = sx / cam.width_f;
    float v = sy / cam.height_f;
    float cx = (u * 2.0f - 1.0f) * cam.aspect * cam.fov_scale;
    float cy = (1.0f - v * 2.0f) * cam.fov_scale;
    V3 dir = ld3(cam.forward) + ld3(cam.right) * cx + ld3(cam.true_up) * cy;
    V3 n = normalize(dir);
    o = ld3(cam.origin);
    d = wavefront ? n : normalize(n); // Ray::new normalises a second time (ray.rs:14-19)
}

// ------------------------------------------------------------------------------------
// Spheres: test_sphere_intersections (shader/src/lib.rs:252-269) +
// test_sphere_intersection (shader/src/intersection.rs:52-87).  Linear, wave-uniform loop.
// Accepts tmin < t < hit.t; the frames pass tmin = RT_MIN_RAY_DISTANCE, the ray queries (ray_query.hip) the ray's own.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void test_spheres(const DevScene& sc, V3 o, V3 d, Hit& hit, float tmin) {
    for (uint32_t i = 0; i < sc.n_spheres; i++) {
        const DevSphere& s = sc.spheres[i];
        V3 oc = o - ld3(s.center);
        float a = dot(d, d);
        float b = 2.0f * dot(oc, d);
        float c = dot(oc, oc) - s.radius * s.radius;
        float disc = b * b - 4.0f * a * c;
        if (disc < 0.0f) continue;
        float sq = sqrtf(disc);
        float t1 = (-b - sq) / (2.0f * a);
        float t2 = (-b + sq) / (2.0f * a);
        float t = (t1 > tmin) ? t1 : t2;
        if (t > tmin && t < hit.t) {
            hit.t = t;
            hit.prim = RT_PRIM_SPHERE_FLAG | i;
            hit.slot = i;
        }
    }
}

// ------------------------------------------------------------------------------------
// Möller–Trumbore, test_triangle_intersection_direct (shader/src/intersection.rs:91-138),
// on a pre-gathered DevTri.  Accept 1e-5 < t < closest (strict).  The reference keeps the
// first triangle found among equal t; its visiting order is its own BVH's.  Here equal t
// is resolved toward the LOWER original triangle index, which is what the reference's
// chunked BVH (> 100k triangles, mesh-order leaves visited left to right,
// src/bvh.rs:154-247) and its brute-force path (shader/src/lib.rs:283) do, and makes the
// result independent of our own topology.
// ------------------------------------------------------------------------------------
// The arithmetic of TriangleIntersector::ray_triangle_intersect (shader/src/intersection.rs:91-138) up to the distance: false when
// the ray is parallel (|a| < 1e-5) or passes outside (u, v); `t` is the distance along d otherwise (the callers apply the range).
// One statement for the leaves of the BVH and for the light grids' lists (wavefront.hip), so both accept exactly the same rays.
// `uv` (optional): the barycentrics the test accepted (weights of v1 and v2), which the ray queries report.
__device__ __forceinline__ bool moller_trumbore(V3 v0, V3 e1, V3 e2, V3 o, V3 d, float& t, float* uv = nullptr) {
    V3 h = cross(d, e2);
    float a = dot(e1, h);
    if (fabsf(a) < RT_MIN_RAY_DISTANCE) return false;
    float f = 1.0f / a;
    V3 s = o - v0;
    float u = f * dot(s, h);
    if (u < 0.0f || u > 1.0f) return false;
    V3 q = cross(s, e1);
    float v = f * dot(d, q);
    if (v < 0.0f || u + v > 1.0f) return false;
    t = f * dot(e2, q);
    if (uv) {
        uv[0] = u;
        uv[1] = v;
    }
    return true;
}

// Returns the record's leaf_count word (the run length when `slot` is the first triangle of a leaf).
// Accepts tmin < t, and t < hit.t or the tie below.
__device__ __forceinline__ uint32_t test_triangle(const DevTri* __restrict__ tris, uint32_t slot, V3 o, V3 d, Hit& hit, float tmin) {
    const float4* p = reinterpret_cast<const float4*>(tris + slot);
    float4 q0 = p[0], q1 = p[1], q2 = p[2];
    // one 48-byte record = three 16-byte loads issued together (otherwise the compiler splits them by first use
    // and sinks the later words behind the early-outs: more, and dependent, fetches)
    asm volatile("" : "+v"(q0.x), "+v"(q0.y), "+v"(q0.z), "+v"(q0.w), "+v"(q1.x), "+v"(q1.y), "+v"(q1.z), "+v"(q1.w), "+v"(q2.x), "+v"(q2.y), "+v"(q2.z), "+v"(q2.w));
    const uint32_t leaf_count = __float_as_uint(q2.w);
    V3 v0 = v3(q0.x, q0.y, q0.z);
    V3 e1 = v3(q0.w, q1.x, q1.y);
    V3 e2 = v3(q1.z, q1.w, q2.x);
    float t;
    if (!moller_trumbore(v0, e1, e2, o, d, t)) return leaf_count;
    uint32_t prim = __float_as_uint(q2.z);
    // equal t: the lower index wins among TRIANGLES only; against a sphere hit or the segment's own limit (prim = MISS, shadow
    // segments) the comparison stays strict, as in find_closest_intersection (lib.rs:214-248: the sphere is kept unless the
    // triangle is strictly closer)
    if (t > tmin && (t < hit.t || (t == hit.t && prim < hit.prim && hit.prim < RT_PRIM_SPHERE_FLAG))) {
        hit.t = t;
        hit.prim = prim;
        hit.slot = slot;
    }
    return leaf_count;
}

// All triangles of the leaf `ref`.  ANY_HIT: stop at the first accepted one and return true.
template <bool COUNT, bool ANY_HIT>
__device__ __forceinline__ bool test_leaf(const DevTri* __restrict__ tris, uint32_t ref, V3 o, V3 d, Hit& hit, Counts& cnt, float tmin) {
    const uint32_t start = ref & RT_DEV_LEAF_START_MASK;
    uint32_t n = 1;
    for (uint32_t i = 0; i < n; i++) {
        if (COUNT) cnt.tris++;
        const uint32_t lc = test_triangle(tris, start + i, o, d, hit, tmin);
        if (i == 0) n = lc;
        if (ANY_HIT && hit.prim != RT_PRIM_MISS) return true;
    }
    return false;
}

// ------------------------------------------------------------------------------------
// BVH traversal.  Replaces BvhTraverser::traverse_and_intersect (shader/src/bvh.rs:18-88) and
// ray_aabb_intersect (shader/src/intersection.rs:151-164): per-lane depth-first walk over the
// 8-wide quantised tree of device_layout.h.  A visit fetches one 80-byte node (5 x dwordx4) and
// slab-tests its (up to) eight children; the result is an 8-bit mask of the slots the ray enters.
// Children whose entry distance exceeds the closest hit are skipped (the reference's slab test
// ignores the closest hit and so visits a superset: result-neutral).  The children entered are
// visited in increasing (slot XOR ray octant) - the builder puts a child into the slot that names
// the corner of the node it lies toward - so there is no distance sort, and what remains of a node
// is a (base, mask) GROUP: one 64-bit stack entry per visit.
//
// The boxes are FILTERS only — which primitive is hit is decided by the reference's
// Möller–Trumbore arithmetic — so they may be conservative but must never be too small, and "too
// small" is judged against what the FLOAT triangle test accepts, not against exact geometry: a ray
// that grazes an edge can be accepted by the triangle test while missing the exact box by rounding.
// The quantised planes are rounded outward by the builder; the float evaluation here is widened:
// with a = scale/d, b = (org - o)/d the plane distances are fma(q, a, b), whose own absolute error
// is below (2^-22 + 2^-23) * (|org - o| + 255 * scale) / |d| (one rounding each in org - o, a, b and the
// fma, one ulp in v_rcp_f32).  Near planes are moved back and far planes forward by RT_FILTER_SLACK
// (1e-5, 28 times that bound) times the same magnitude; the margin is there for the triangle test's
// own rounding: Möller–Trumbore accepts rays that pass a few 1e-7 of their distance OUTSIDE a
// triangle's exact box (a grazed edge whose triangle defines the node's face gets no help from the
// quantisation).  Round 1's 1e-6 was too tight by a hair: at one ray in 2*10^9 of the headline frame the
// result depended on the tree (found in round 2 when a second builder produced other boxes).  With 1e-5
// every builder gives the same frame, the one the reference's brute-force path gives - the reference's
// own BVH walk, whose slab test has no margin at all, misses that triangle (tests/test_oracle_extended.py
// pins the pixel).  The wider margin costs nothing measurable (it is far below the quantisation step).
// ------------------------------------------------------------------------------------
#ifndef RT_FILTER_SLACK
#define RT_FILTER_SLACK 1.0e-5f
#endif
#ifndef RT_FILTER_RCP
#define RT_FILTER_RCP 1 /* round 2: -1 % on the headline frame; the error bound above includes its one ulp */
#endif
struct FilterRay { // per-segment constants of the box filter
    V3 o, inv;     // inv = 1/d with |d| clamped away from zero (a filter may do that; the triangle test uses the real d)
};
__device__ __forceinline__ FilterRay make_filter_ray(V3 o, V3 d) {
    FilterRay f;
    f.o = o;
    float dx = fabsf(d.x) < 1e-30f ? copysignf(1e-30f, d.x) : d.x;
    float dy = fabsf(d.y) < 1e-30f ? copysignf(1e-30f, d.y) : d.y;
    float dz = fabsf(d.z) < 1e-30f ? copysignf(1e-30f, d.z) : d.z;
#if RT_FILTER_RCP
    f.inv = v3(__builtin_amdgcn_rcpf(dx), __builtin_amdgcn_rcpf(dy), __builtin_amdgcn_rcpf(dz));
#else
    f.inv = v3(1.0f / dx, 1.0f / dy, 1.0f / dz);
#endif
    return f;
}
// (dx < 0) | (dy < 0) << 1 | (dz < 0) << 2: children are visited in increasing (slot XOR octant)
__device__ __forceinline__ uint32_t ray_octant(const FilterRay& f) {
    return (f.inv.x < 0.0f ? 1u : 0u) | (f.inv.y < 0.0f ? 2u : 0u) | (f.inv.z < 0.0f ? 4u : 0u);
}
// The set slot of the 8-bit mask m (!= 0) with the smallest (slot XOR oct): permute the mask so that bit j holds slot
// j XOR oct (three conditional swaps), take the lowest set bit.  The persistent kernels of wavefront.hip read the same
// function from a 2 KB table in LDS instead (tests compare the kernels bit for bit).
__device__ __forceinline__ uint32_t first_slot(uint32_t m, uint32_t oct) {
    uint32_t p = m & 0xFFu;
    if (oct & 1u) p = ((p & 0x55u) << 1) | ((p >> 1) & 0x55u);
    if (oct & 2u) p = ((p & 0x33u) << 2) | ((p >> 2) & 0x33u);
    if (oct & 4u) p = ((p & 0x0Fu) << 4) | (p >> 4);
    return ((uint32_t)__ffs((int)p) - 1u) ^ oct;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// One visit of the 8-wide node `idx` (DevNode8, device_layout.h): the conservative quantised-box filter for eight slots.
// Returns the 8-bit mask of the slots the ray enters (bit s = slot s), already restricted to occupied slots.
template <bool COUNT>
__device__ __forceinline__ uint32_t visit_node8(const uint4* __restrict__ nodes, uint32_t idx, const FilterRay& fr, float closest_t, Counts& cnt,
                                                uint32_t& child_base, uint32_t& tri_base, uint32_t& imask, uint32_t& lmask) {
    const uint4* n = nodes + (size_t)idx * 5;
    const uint4 w0 = n[0], w1 = n[1], w2 = n[2], w3 = n[3], w4 = n[4];
    // keep the node's loads together: the words that are only used after the box tests would otherwise be fetched there
    uint32_t w1x = w1.x, w1y = w1.y, w1z = w1.z;
    asm volatile("" : "+v"(w1x), "+v"(w1y), "+v"(w1z));
    if (COUNT) cnt.nodes++;
    const float ax = ldexpf(fr.inv.x, (int)(int8_t)(w0.w & 0xFFu)), ay = ldexpf(fr.inv.y, (int)(int8_t)((w0.w >> 8) & 0xFFu)),
                az = ldexpf(fr.inv.z, (int)(int8_t)((w0.w >> 16) & 0xFFu));
    const float dox = __uint_as_float(w0.x) - fr.o.x, doy = __uint_as_float(w0.y) - fr.o.y, doz = __uint_as_float(w0.z) - fr.o.z;
    const float bx = dox * fr.inv.x, by = doy * fr.inv.y, bz = doz * fr.inv.z;
    const float ex = fmaf(255.0f, fabsf(ax), fabsf(bx)) * RT_FILTER_SLACK;
    const float ey = fmaf(255.0f, fabsf(ay), fabsf(by)) * RT_FILTER_SLACK;
    const float ez = fmaf(255.0f, fabsf(az), fabsf(bz)) * RT_FILTER_SLACK;
    const f32x2 pm = {-1.0f, 1.0f};
    const f32x2 bx2 = __builtin_elementwise_fma((f32x2){ex, ex}, pm, (f32x2){bx, bx});
    const f32x2 by2 = __builtin_elementwise_fma((f32x2){ey, ey}, pm, (f32x2){by, by});
    const f32x2 bz2 = __builtin_elementwise_fma((f32x2){ez, ez}, pm, (f32x2){bz, bz});
    const f32x2 ax2 = {ax, ax}, ay2 = {ay, ay}, az2 = {az, az};
    const bool px = fr.inv.x >= 0.0f, py = fr.inv.y >= 0.0f, pz = fr.inv.z >= 0.0f;
    // [half]: w2 = qlo_x[0], qlo_x[1], qlo_y[0], qlo_y[1]; w3 = qlo_z[0], qlo_z[1], qhi_x[0], qhi_x[1]; w4 = qhi_y[0], qhi_y[1], qhi_z[0], qhi_z[1]
    const uint32_t nxw[2] = {px ? w2.x : w3.z, px ? w2.y : w3.w}, fxw[2] = {px ? w3.z : w2.x, px ? w3.w : w2.y};
    const uint32_t nyw[2] = {py ? w2.z : w4.x, py ? w2.w : w4.y}, fyw[2] = {py ? w4.x : w2.z, py ? w4.y : w2.w};
    const uint32_t nzw[2] = {pz ? w3.x : w4.z, pz ? w3.y : w4.w}, fzw[2] = {pz ? w4.z : w3.x, pz ? w4.w : w3.y};
    const float limit = closest_t * 1.0000153f;
    uint32_t miss = 0; // bit s: the ray does NOT enter slot s (sign bits of tmax - tmin, shifted in one per slot)
#pragma unroll
    for (int h = 1; h >= 0; h--) {
#pragma unroll
        for (int i = 3; i >= 0; i--) {
            const f32x2 qx = {(float)((nxw[h] >> (8 * i)) & 0xFFu), (float)((fxw[h] >> (8 * i)) & 0xFFu)};
            const f32x2 qy = {(float)((nyw[h] >> (8 * i)) & 0xFFu), (float)((fyw[h] >> (8 * i)) & 0xFFu)};
            const f32x2 qz = {(float)((nzw[h] >> (8 * i)) & 0xFFu), (float)((fzw[h] >> (8 * i)) & 0xFFu)};
            const f32x2 tx = __builtin_elementwise_fma(qx, ax2, bx2);
            const f32x2 ty = __builtin_elementwise_fma(qy, ay2, by2);
            const f32x2 tz = __builtin_elementwise_fma(qz, az2, bz2);
            const float tmin = fmaxf(fmaxf(tx.x, ty.x), fmaxf(tz.x, 0.0f));
            const float tmax = fminf(fminf(tx.y, ty.y), fminf(tz.y, limit));
            // entered <=> tmin <= tmax <=> tmax - tmin >= +0 (all finite): v_alignbit shifts the sign bit in; slot 4h+i ends up in bit 4h+i
            miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(tmax - tmin), 31);
        }
    }
    child_base = w1x;
    tri_base = w1y;
    lmask = w1z & 0xFFu;
    imask = w0.w >> 24;
    return ~miss & (imask | lmask);
}

// The walk of one lane on its own (reference-mode kernel, nested-loop megakernel): groups on a per-lane stack of 64-bit
// entries (lane-interleaved: entry k of this lane at stack[k * 64]), a node's leaves tested right after its visit, before its
// inner children (their hits cull the children's subtrees).  ANY_HIT (shadow segments of the extended mode): return at the
// first accepted triangle.  Triangles are accepted in (tmin, hit.t); the boxes filter by [0, hit.t] only (conservative for any tmin >= 0).
template <bool COUNT, bool ANY_HIT>
__device__ __forceinline__ void traverse(const DevScene& sc, V3 o, V3 d, uint2* __restrict__ stack, Hit& hit, Counts& cnt, float tmin) {
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
        const uint32_t hm = visit_node8<COUNT>(nodes, node, fr, hit.t, cnt, cb, tb, im, lm);
        uint32_t t = hm & lm;
        while (t) {
            const uint32_t sl = first_slot(t, oct);
            t ^= 1u << sl;
            const uint32_t first = tb + RT_DEV_LEAF_STRIDE * (uint32_t)__popc(lm & ((1u << sl) - 1u));
            if (test_leaf<COUNT, ANY_HIT>(sc.tris, RT_DEV_LEAF_FLAG | first, o, d, hit, cnt, tmin)) return;
        }
        g_base = cb;
        g_bits = (hm & im) | (im << 8);
    }
}

// find_closest_intersection (shader/src/lib.rs:174-249): spheres first, then triangles with
// max_t = sphere t; a triangle is only accepted strictly closer, so it wins when both hit.
// (k_pq_trace, path_query.hip, writes these statements out with the segment's own (tmin, tmax): a change here is a change there.)
template <bool COUNT>
__device__ __forceinline__ Hit find_closest(const DevScene& sc, V3 o, V3 d, uint2* stack, Counts& cnt) {
    Hit hit;
    hit.t = RT_F32_MAX; // f32::MAX - 2.0 == f32::MAX
    hit.prim = RT_PRIM_MISS;
    hit.slot = 0;
    test_spheres(sc, o, d, hit, RT_MIN_RAY_DISTANCE);
    traverse<COUNT, false>(sc, o, d, stack, hit, cnt, RT_MIN_RAY_DISTANCE);
    return hit;
}

// any hit in (tmin, tmax)?  Spheres first, then the BVH with early exit.
template <bool COUNT>
__device__ __forceinline__ bool occluded(const DevScene& sc, V3 o, V3 d, float tmin, float tmax, uint2* stack, Counts& cnt) {
    Hit h;
    h.t = tmax;
    h.prim = RT_PRIM_MISS;
    h.slot = 0;
    test_spheres(sc, o, d, h, tmin);
    if (h.prim != RT_PRIM_MISS) return true;
    traverse<COUNT, true>(sc, o, d, stack, h, cnt, tmin);
    return h.prim != RT_PRIM_MISS;
}

// ------------------------------------------------------------------------------------
// Shading: calculate_shading (shader/src/lib.rs:300-338), LightingCalculator
// (shader/src/lighting.rs:20-139), MaterialEvaluator (shader/src/material.rs:16-83).
// Returns the colour of all three channel passes at once: component c is what the
// channel-c dispatch would have kept (filter_color_by_channel, lib.rs:342-349).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ V3 evaluate_brdf(const DevMaterial& m, float intensity) {
    V3 albedo = ld3(m.albedo);
    V3 diffuse = albedo / RT_PI;
    float is_metallic = (m.metallic > 0.5f) ? 1.0f : 0.0f;
    V3 metallic_contrib = albedo * intensity * 0.5f;
    V3 dielectric_contrib = diffuse * intensity;
    return metallic_contrib * is_metallic + dielectric_contrib * (1.0f - is_metallic);
}

// calculate_light_contribution (lighting.rs:50-94) for one light.  Also returns the direction and
// length of the segment toward the light (used by the extended mode's shadow rays).
__device__ __forceinline__ V3 light_contribution(const DevLight& L, const DevMaterial& m, V3 point, V3 normal, V3& to_light_dir,
                                                 float& to_light_dist) {
    V3 dir_light_dir = ld3(L.neg_ndir); // -normalize(direction), lighting.rs:103 (per-light constant, DevLight)
    float dir_intensity = fmaxf(dot(normal, dir_light_dir), 0.0f) * L.intensity;
    V3 to_light = ld3(L.position) - point; // lighting.rs:120-122
    float distance = length(to_light);
    V3 pld = normalize(to_light);
    float att = f16_round_trip(1.0f / (1.0f + distance * distance * 0.01f)); // :125-127
    float point_intensity = fmaxf(dot(normal, pld), 0.0f) * L.intensity * att;
    float spot_factor = fmaxf(dot(dir_light_dir, pld), 0.0f); // :132 (the same -normalize(direction))
    float spot_intensity = point_intensity * spot_factor;
    float is_dir = (L.light_type == 0) ? 1.0f : 0.0f;
    float is_point = (L.light_type == 1) ? 1.0f : 0.0f;
    float is_spot = (L.light_type == 2) ? 1.0f : 0.0f;
    float final_i = dir_intensity * is_dir + point_intensity * is_point + spot_intensity * is_spot;
    V3 brdf = evaluate_brdf(m, final_i);
    float valid = (final_i > 0.0f) ? 1.0f : 0.0f; // index_valid is always 1 inside the loop
    to_light_dir = (L.light_type == 0) ? dir_light_dir : pld;
    to_light_dist = (L.light_type == 0) ? RT_F32_MAX : distance;
    return brdf * ld3(L.color) * valid;
}

__device__ __forceinline__ V3 calculate_lighting(const DevScene& sc, const DevMaterial& m, V3 point, V3 normal) {
    V3 total = v3(0.0f, 0.0f, 0.0f);
    total = total + ld3(m.albedo) * 0.1f; // ambient, lighting.rs:30-31
    for (uint32_t li = 0; li < sc.n_lights; li++) {
        V3 sd;
        float st;
        total = total + light_contribution(sc.lights[li], m, point, normal, sd, st);
    }
    return total + ld3(m.emission);
}

// hit -> (point, geometric normal, material id)
// geometric normal and material at a hit point: `sphere` selects DevScene::spheres[slot], else DevScene::tris[slot]
__device__ __forceinline__ void surface_at(const DevScene& sc, bool sphere, uint32_t slot, V3 point, V3& normal, uint32_t& material_id) {
    if (sphere) {
        const DevSphere& s = sc.spheres[slot];
        normal = normalize(point - ld3(s.center)); // intersection.rs:80
        material_id = s.material_id;
    } else {
        const float4* p = reinterpret_cast<const float4*>(sc.tris + slot);
        float4 q0 = p[0], q1 = p[1], q2 = p[2];
        asm volatile("" : "+v"(q0.w), "+v"(q1.x), "+v"(q1.y), "+v"(q1.z), "+v"(q1.w), "+v"(q2.x), "+v"(q2.y)); // one round trip for the record
        V3 e1 = v3(q0.w, q1.x, q1.y);
        V3 e2 = v3(q1.z, q1.w, q2.x);
        normal = normalize(cross(e1, e2)); // geometric, winding dependent, never flipped (intersection.rs:132)
        material_id = __float_as_uint(q2.y);
    }
}
__device__ __forceinline__ void hit_geometry(const DevScene& sc, const Hit& hit, V3 o, V3 d, V3& point, V3& normal, uint32_t& material_id) {
    point = o + d * hit.t; // Ray::at, ray.rs:56-58
    surface_at(sc, (hit.prim & RT_PRIM_SPHERE_FLAG) != 0, hit.slot, point, normal, material_id);
}

// The transmission mix of calculate_shading (lib.rs:323-337) for all three channel passes at once.
__device__ __forceinline__ V3 transmission_mix(const DevMaterial& m, V3 lighting, float tf) {
    // per channel c: ior_c = ior + {-0.018, 0, +0.035}[c]; disp = (ior_c - 1) / (ior - 1)   (material.rs:42-58, lib.rs:326-334)
    float disp_r = ((m.ior + -0.018f) - 1.0f) / (m.ior - 1.0f);
    float disp_g = ((m.ior + 0.0f) - 1.0f) / (m.ior - 1.0f);
    float disp_b = ((m.ior + 0.035f) - 1.0f) / (m.ior - 1.0f);
    float keep = 1.0f - tf;
    return v3(lighting.x * keep + (0.2f * disp_r) * tf, lighting.y * keep + (0.2f * disp_g) * tf,
              lighting.z * keep + (0.3f * disp_b) * tf);
}

__device__ __forceinline__ V3 shade_hit(const DevScene& sc, const Hit& hit, V3 o, V3 d) {
    V3 point, normal;
    uint32_t material_id;
    hit_geometry(sc, hit, o, d, point, normal, material_id);
    if (material_id >= sc.n_materials) return RT_MAGENTA();
    const DevMaterial m = sc.materials[material_id];
    V3 lighting = calculate_lighting(sc, m, point, normal);
    float tf = fminf(fmaxf(m.transmission, 0.0f), 1.0f); // lib.rs:323
    if (tf > 0.0f) return transmission_mix(m, lighting, tf);
    return lighting;
}

// Rgba8Unorm store conversion: clamp, scale, round half up; NaN -> 0.
__device__ __forceinline__ uint32_t unorm8(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 1.0f) return 255u;
    return (uint32_t)floorf(v * 255.0f + 0.5f);
}

// Block -> pixel mapping shared by the kernels: one wave per 8x8 block of an owned tile.
struct PixelCoord {
    uint32_t x, y;
    bool valid;
};
__device__ __forceinline__ PixelCoord block_pixel_at(const DevFrame& fr, uint32_t block, uint32_t lane) {
    uint32_t ox, oy, tw, th, blk;
    const uint32_t bpt_x = (fr.tile_size + 7u) >> 3;
    if (fr.single_tile) {
        ox = fr.tile_off_x; oy = fr.tile_off_y; tw = fr.tile_w; th = fr.tile_h;
        blk = block;
    } else {
        const uint32_t bpt = bpt_x * bpt_x;
        uint32_t k = block / bpt;
        blk = block - k * bpt;
        uint32_t tile = fr.tile_first + k * fr.tile_stride;
        uint32_t ty = tile / fr.tiles_x, tx = tile - ty * fr.tiles_x;
        ox = tx * fr.tile_size; oy = ty * fr.tile_size;
        tw = min(fr.tile_size, fr.width - ox); // calculate_tile_dimensions, src/compute.rs:194-209
        th = min(fr.tile_size, fr.height - oy);
    }
    uint32_t by = blk / bpt_x, bx = blk - by * bpt_x;
    uint32_t idx = bx * 8u + (lane & 7u), idy = by * 8u + (lane >> 3);
    PixelCoord pc;
    pc.x = ox + idx;
    pc.y = oy + idy;
    // is_pixel_in_bounds, shader/src/lib.rs:152-163
    pc.valid = idx < tw && idy < th && pc.x < fr.width && pc.y < fr.height;
    return pc;
}
__device__ __forceinline__ PixelCoord block_pixel(const DevFrame& fr) { return block_pixel_at(fr, blockIdx.x, threadIdx.x); }

// ====================================================================================
// Extended mode (RT_MODE_EXTENDED): jittered samples, shadow rays and real bounces, built on
// the reference's declared-but-stub wavefront API (SimpleRng wavefront.rs:46-72, pixel seed
// lib.rs:103-105, generate_camera_ray wavefront.rs:75-112, WavefrontRay types and epsilon
// shared/src/lib.rs:833-956, apply_russian_roulette shared/src/lib.rs:969-978).  The rules are
// stated in DESIGN.md "Extended mode" (the test suite holds an executable CPU statement of them);
// this is the same arithmetic in the same order.
// ====================================================================================
struct SimpleRng {
    uint32_t seed;
    __device__ __forceinline__ uint32_t next_u32() {
        seed = seed * 1664525u + 1013904223u;
        return seed;
    }
    __device__ __forceinline__ float next_f32() { return (float)(next_u32() >> 8) / 16777216.0f; }
};

__device__ __forceinline__ SimpleRng rng_for(uint32_t pixel_seed, uint32_t sample) {
    uint32_t h = pixel_seed + sample * 0x9E3779B9u;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return SimpleRng{h};
}

// Progressive accumulation (RT_FLAG_ACCUMULATE): a pixel's sum starts from the samples earlier calls left in
// DevTargets::run_sum (zero for a closed frame or the first call of an accumulation) and goes back there with this launch's samples added,
// in sample order, so that the image equals one frame of all the samples.
__device__ __forceinline__ V3 run_sum_start(const DevFrame& fr, const DevTargets& tg, size_t pix) {
    if (!tg.run_sum || fr.sample_base == 0) return v3(0.0f, 0.0f, 0.0f);
    const float4 a = reinterpret_cast<const float4*>(tg.run_sum)[pix];
    return v3(a.x, a.y, a.z);
}
__device__ __forceinline__ void run_sum_keep(const DevTargets& tg, size_t pix, V3 sum) {
    if (tg.run_sum) reinterpret_cast<float4*>(tg.run_sum)[pix] = make_float4(sum.x, sum.y, sum.z, 0.0f);
}

// The image of a pixel from its sum over n samples: the float target and the three rgba8 channel textures.  Every kernel that ends a
// pixel's samples stores through this one function (the frame kernels, k_wf_resolve, k_ad_image), so their bits cannot drift apart.
__device__ __forceinline__ void store_image(const DevTargets& tg, size_t pix, V3 sum, float n) {
    const V3 color = v3(sum.x / n, sum.y / n, sum.z / n);
    if (tg.rgba32f) reinterpret_cast<float4*>(tg.rgba32f)[pix] = make_float4(color.x, color.y, color.z, 1.0f);
    if (tg.chan[0]) reinterpret_cast<uint32_t*>(tg.chan[0])[pix] = unorm8(color.x) | 0xFF000000u;
    if (tg.chan[1]) reinterpret_cast<uint32_t*>(tg.chan[1])[pix] = (unorm8(color.y) << 8) | 0xFF000000u;
    if (tg.chan[2]) reinterpret_cast<uint32_t*>(tg.chan[2])[pix] = (unorm8(color.z) << 16) | 0xFF000000u;
}

// Adaptive sampling (rt_render_adaptive).  A pixel of an adaptive running image keeps n (its samples, run_sum w), S
// (their sum, run_sum xyz) and H (the sum of its odd-indexed samples, run_odd xyz).  A new image (DevFrame::sample_base 0) has none.
struct AdPixel {
    V3 s, h;
    uint32_t n;
};
__device__ __forceinline__ AdPixel ad_load(const DevFrame& fr, const DevTargets& tg, size_t pix) {
    AdPixel a;
    a.s = a.h = v3(0.0f, 0.0f, 0.0f);
    a.n = 0u;
    if (fr.sample_base == 0u) return a;
    const float4 s = reinterpret_cast<const float4*>(tg.run_sum)[pix], h = reinterpret_cast<const float4*>(tg.run_odd)[pix];
    a.s = v3(s.x, s.y, s.z);
    a.h = v3(h.x, h.y, h.z);
    a.n = (uint32_t)s.w;
    return a;
}
__device__ __forceinline__ void ad_keep(const DevTargets& tg, size_t pix, V3 s, V3 h, uint32_t n) {
    reinterpret_cast<float4*>(tg.run_sum)[pix] = make_float4(s.x, s.y, s.z, (float)n);
    reinterpret_cast<float4*>(tg.run_odd)[pix] = make_float4(h.x, h.y, h.z, 0.0f);
}
// The rule's error, in exactly this order (rt_hip.h): I = S / n, A = (H + H) / n, d = |I - A| summed r, g, b, e = d / (1e-4 + sqrt(I.r + I.g + I.b)).
__device__ __forceinline__ float ad_error(V3 s, V3 h, uint32_t n_samples) {
    const float n = (float)n_samples;
    const V3 i = v3(s.x / n, s.y / n, s.z / n);
    const V3 a = v3((h.x + h.x) / n, (h.y + h.y) / n, (h.z + h.z) / n);
    const float d = fabsf(i.x - a.x) + fabsf(i.y - a.y) + fabsf(i.z - a.z);
    return d / (1e-4f + sqrtf(i.x + i.y + i.z));
}
// Whether the pixel takes samples this call: too few samples so far, or an error at or above the threshold (a NaN error: converged).
__device__ __forceinline__ bool ad_active(const AdPixel& a, float threshold, uint32_t min_samples) {
    return a.n < min_samples || ad_error(a.s, a.h, a.n) >= threshold;
}
// Whether lane `lane` of owned block `block` takes samples this call (k_ad_select's mask).
__device__ __forceinline__ bool ad_lane_active(const DevFrame& fr, uint32_t block, uint32_t lane) { return (fr.ad_mask[block] >> lane) & 1ull; }

// sin/cos(2*pi*u) as explicit-fma polynomials: identical bits on the host oracle and here.
__device__ __forceinline__ void sincos_2pi(float u, float& s_out, float& c_out) {
    float f4 = u * 4.0f;
    float qf = floorf(f4);
    int q = (int)qf;
    float x = (f4 - qf) * 1.57079632679489661923f;
    float x2 = x * x;
    float sp = __builtin_fmaf(x2, -2.50521083854417187751e-8f, 2.75573192239858906526e-6f);
    sp = __builtin_fmaf(x2, sp, -1.98412698412698412698e-4f);
    sp = __builtin_fmaf(x2, sp, 8.33333333333333333333e-3f);
    sp = __builtin_fmaf(x2, sp, -1.66666666666666666667e-1f);
    sp = __builtin_fmaf(x2, sp, 1.0f);
    float sn = x * sp;
    float cp = __builtin_fmaf(x2, 2.08767569878680989792e-9f, -2.75573192239858906526e-7f);
    cp = __builtin_fmaf(x2, cp, 2.48015873015873015873e-5f);
    cp = __builtin_fmaf(x2, cp, -1.38888888888888888889e-3f);
    cp = __builtin_fmaf(x2, cp, 4.16666666666666666667e-2f);
    cp = __builtin_fmaf(x2, cp, -0.5f);
    float cs = __builtin_fmaf(x2, cp, 1.0f);
    switch (q & 3) {
        case 0: s_out = sn; c_out = cs; break;
        case 1: s_out = cs; c_out = -sn; break;
        case 2: s_out = -sn; c_out = -cs; break;
        default: s_out = -cs; c_out = sn; break;
    }
}

__device__ __forceinline__ V3 unit_vector(float u1, float u2) {
    float z = 1.0f - 2.0f * u1;
    float r = sqrtf(fmaxf(0.0f, 1.0f - z * z));
    float sn, cs;
    sincos_2pi(u2, sn, cs);
    return v3(r * cs, r * sn, z);
}

// ------------------------------------------------------------------------------------
// The extended mode's path vertex, stated once for its three implementations: the queue pipeline
// (wavefront.hip), the state-machine megakernel and the nested-loop megakernel (kernels.hip).  The tests hold the three to the same
// bits and to the CPU statement, so every expression here, and the order of the rng draws, is part of the result.
// ------------------------------------------------------------------------------------
#define EXT_EPS 0.001f /* WavefrontRay::t_min (shared/src/lib.rs:854) as the origin offset of shadow and continuation segments */

struct SegCounts {
    uint32_t camera, continuation, shadow;
};

__device__ __forceinline__ unsigned long long wave_sum(uint32_t v) {
    unsigned long long s = v;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, WAVE);
    return s;
}

// The megakernels' epilogue.  Segment counts are part of the result (rt_stats.rays): one atomic per wave and counter.
template <bool COUNT>
__device__ __forceinline__ void flush_segment_counts(const DevTargets& tg, const SegCounts& seg, const Counts& cnt) {
    unsigned long long c0 = wave_sum(seg.camera), c1 = wave_sum(seg.continuation), c2 = wave_sum(seg.shadow);
    unsigned long long n0 = COUNT ? wave_sum(cnt.nodes) : 0ull, n1 = COUNT ? wave_sum(cnt.tris) : 0ull;
    if (threadIdx.x == 0 && tg.counters) {
        atomicAdd(&tg.counters[RT_CNT_SEGMENTS], c0 + c1 + c2);
        atomicAdd(&tg.counters[RT_CNT_CAMERA], c0);
        atomicAdd(&tg.counters[RT_CNT_CONTINUATION], c1);
        atomicAdd(&tg.counters[RT_CNT_SHADOW], c2);
        if (COUNT) {
            atomicAdd(&tg.counters[RT_CNT_NODE_VISITS], n0);
            atomicAdd(&tg.counters[RT_CNT_TRI_TESTS], n1);
        }
    }
}

// The camera ray of global sample `sample` (DevFrame::sample_base + k, or the pixel's own n + k in an adaptive call) of pixel (px, py):
// the pixel's seed (lib.rs:103-105), two draws under `jitter`, else the pixel centre.  Returns the rng in the state the path continues
// from; a caller that only wants the ray drops it, and the seed is then computed under `jitter` alone.
__device__ __forceinline__ SimpleRng ext_sample_ray(const DevCamera& cam, uint32_t width, uint32_t frame_seed, uint32_t jitter, uint32_t px, uint32_t py,
                                                    uint32_t sample, bool wavefront, V3& o, V3& d) {
    SimpleRng rng = rng_for(frame_seed + px + py * width, sample);
    float jx = 0.5f, jy = 0.5f;
    if (jitter) {
        jx = rng.next_f32();
        jy = rng.next_f32();
    }
    camera_ray(cam, (float)px + jx, (float)py + jy, wavefront, o, d);
    return rng;
}

// Step 2.  A light whose contribution is not zero is gated by a shadow segment.
__device__ __forceinline__ bool needs_shadow_segment(V3 contrib) { return contrib.x != 0.0f || contrib.y != 0.0f || contrib.z != 0.0f; }
// The ordered light sum: the 0.1 albedo ambient term at the terminal vertex only, the lights in index order (lighting.rs:33-43) with
// the occluded ones skipped, emission last.  `visible(li, dir, dist)` is asked only about lights that need a segment, in that order.
__device__ __forceinline__ V3 light_sum_begin(const DevMaterial& m, bool terminal) {
    V3 total = v3(0.0f, 0.0f, 0.0f);
    if (terminal) total = total + ld3(m.albedo) * 0.1f;
    return total;
}
__device__ __forceinline__ V3 light_sum_end(V3 total, const DevMaterial& m) { return total + ld3(m.emission); }
template <class Visible>
__device__ __forceinline__ V3 ext_light_sum(const DevLight* lights, uint32_t n_lights, const DevMaterial& m, V3 point, V3 normal, bool terminal,
                                            bool shadows, Visible visible) {
    V3 total = light_sum_begin(m, terminal);
    for (uint32_t li = 0; li < n_lights; li++) {
        V3 sdir;
        float sdist;
        const V3 contrib = light_contribution(lights[li], m, point, normal, sdir, sdist);
        if (needs_shadow_segment(contrib) && shadows && !visible(li, sdir, sdist)) continue;
        total = total + contrib;
    }
    return light_sum_end(total, m);
}

// Step 3.  Leaving a vertex with its light sum: the terminal one adds the reference's calculate_shading (transmission mix included),
// any other the part that is not transmitted.  Returns T = clamp(transmission, 0, 1), which the continuation draws against.
__device__ __forceinline__ float ext_leave_vertex(const DevMaterial& m, V3 lighting, bool terminal, V3 throughput, V3& radiance) {
    const float tf = fminf(fmaxf(m.transmission, 0.0f), 1.0f); // lib.rs:323
    if (terminal) {
        V3 out = lighting;
        if (tf > 0.0f) out = transmission_mix(m, lighting, tf);
        radiance = radiance + out * throughput;
    } else {
        radiance = radiance + (lighting * (1.0f - tf)) * throughput;
    }
    return tf;
}

// Steps 4 and 5.  The continuation from a non-terminal vertex at `point` (geometric normal `normal`, never flipped; `din` the incoming
// direction; `depth` the vertex's index on the path).  Updates the rng, the hero channel (3: none yet) and the throughput, gives the
// next segment, and returns false when the path is absorbed (rng, channel and throughput are then of no further use).
// One exit with an `absorbed` flag, not early returns: with those k_wf_finish takes 89 VGPRs instead of 79 and loses a wave per SIMD.
__device__ __forceinline__ bool ext_scatter(const DevMaterial& m, V3 point, V3 normal, V3 din, float tf, uint32_t depth, SimpleRng& rng,
                                            uint32_t& channel, V3& throughput, V3& norigin, V3& ndir) {
    const bool front = dot(normal, din) < 0.0f;
    const V3 nf = front ? normal : -normal; // face-forwarded
    bool transmit = false;
    if (tf > 0.0f) transmit = rng.next_f32() < tf;
    bool absorbed = false;
    if (transmit) {
        if (channel == 3) { // the hero channel, chosen once per path
            const uint32_t c = (uint32_t)(rng.next_f32() * 3.0f);
            channel = c < 2 ? c : 2;
            throughput = v3(channel == 0 ? throughput.x * 3.0f : 0.0f, channel == 1 ? throughput.y * 3.0f : 0.0f,
                            channel == 2 ? throughput.z * 3.0f : 0.0f);
        }
        const float offs = channel == 0 ? -0.018f : (channel == 1 ? 0.0f : 0.035f); // dispersion, material.rs:47-52
        const float ior_c = m.ior + offs;
        const float eta = front ? (1.0f / ior_c) : ior_c;
        const float cos_i = -dot(nf, din);
        const float sin2_t = eta * eta * (1.0f - cos_i * cos_i);
        if (sin2_t > 1.0f) { // total internal reflection: stays on the incoming side
            ndir = din - nf * (2.0f * dot(din, nf));
            norigin = point + nf * EXT_EPS;
        } else {
            const float cos_t = sqrtf(1.0f - sin2_t);
            ndir = din * eta + nf * (eta * cos_i - cos_t);
            norigin = point - nf * EXT_EPS;
        }
        ndir = normalize(ndir);
        throughput = throughput * ld3(m.albedo);
    } else if (m.metallic > 0.5f) {
        const float u1 = rng.next_f32(), u2 = rng.next_f32();
        const V3 r = din - nf * (2.0f * dot(din, nf));
        ndir = normalize(r + unit_vector(u1, u2) * m.roughness);
        absorbed = !(dot(ndir, nf) > 0.0f); // a lobe direction below the surface
        norigin = point + nf * EXT_EPS;
        if (!absorbed) throughput = throughput * ld3(m.albedo);
    } else {
        const float u1 = rng.next_f32(), u2 = rng.next_f32();
        V3 w = nf + unit_vector(u1, u2); // cosine-weighted
        if (dot(w, w) < 1e-12f) w = nf;
        ndir = normalize(w);
        norigin = point + nf * EXT_EPS;
        throughput = throughput * ld3(m.albedo);
    }
    if (!absorbed && depth >= 2) { // apply_russian_roulette (shared/src/lib.rs:969-978) from the third vertex on
        const float p = fminf(fmaxf(fmaxf(fmaxf(throughput.x, throughput.y), throughput.z), 0.05f), 1.0f);
        if (rng.next_f32() > p) absorbed = true;
        else throughput = v3(throughput.x / p, throughput.y / p, throughput.z / p);
    }
    return !absorbed;
}

// Direction and length of the shadow segment toward light L from `point`: the same expressions
// light_contribution evaluates (lighting.rs:103, 120-122), so both produce the same bits.
__device__ __forceinline__ void shadow_segment(const DevLight& L, V3 point, V3& dir, float& dist) {
    if (L.light_type == 0) {
        dir = ld3(L.neg_ndir);
        dist = RT_F32_MAX;
    } else {
        V3 to_light = ld3(L.position) - point;
        dist = length(to_light);
        dir = normalize(to_light);
    }
}

// Wave-aggregated queue append: one atomicAdd per wave, slots handed out by ballot + prefix count.
__device__ __forceinline__ void wave_append(uint32_t* __restrict__ queue, uint32_t* __restrict__ counter, bool pred, uint32_t value) {
    const unsigned long long m = __ballot(pred);
    if (m == 0ull) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader, WAVE);
    if (pred) queue[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = value;
}

} // namespace rtdev

#endif
