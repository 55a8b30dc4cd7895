// contact_triangle.hip — the kernel of the triangle contact query of include/rt_hip.h (rt_contact_triangle): for each resting
// triangle the caller supplies, the max_contacts nearest primitives of the scene whose distance from the triangle is below its
// margin, nearest first - their points, distances and the triangle's own weights at the closest pair - their number, or only whether
// there is one.
//
// Every statement that decides a bit of the answer is in contact_triangle_rules.h (and through it contact_capsule_rules.h,
// sweep_capsule_rules.h and closest_point_all_rules.h) and the walk in group_walk.h, which the host check
// (tests/check_contact_triangle.cpp) runs against a brute-force sort; how a lane reads a node and a record, its stack and where its
// list lives are LaneListAccess of query_lane.h; this file supplies the output records.  One lane per triangle, one wave per block,
// the per-lane stack in LDS and the list behind it: the launch shape of k_contact_capsule.
#include "contact_triangle.h"

#include "contact_triangle_rules.h"
#include "query_lane.h"

using namespace rtdev;

namespace {

// One rt_triangle_contact_query (v0 margin | v1 pad | v2 pad) per lane -> max_contacts rt_triangle_contact records at out[i *
// max_contacts ..] (the listed primitives, then misses) and, counts != null, counts[i] = cc_list_count.  max_contacts == 0: `out` is
// not touched.
template <bool COUNT, int MODE>
__global__ __launch_bounds__(WAVE) void k_contact_triangle(DevScene sc, const float4* __restrict__ triangles, uint4* __restrict__ out,
                                                            uint32_t* __restrict__ counts, uint32_t n, uint32_t max_contacts,
                                                            unsigned long long* __restrict__ counters) {
    extern __shared__ uint2 s_stack[]; // the stack of k_cp_nearest, then 3 * max_contacts * 64 list words
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    const float4 c0 = triangles[3 * (size_t)i], c1 = triangles[3 * (size_t)i + 1], c2 = triangles[3 * (size_t)i + 2];
    const float v0[3] = {c0.x, c0.y, c0.z}, v1[3] = {c1.x, c1.y, c1.z}, v2[3] = {c2.x, c2.y, c2.z};
    const rt::CtQuery q = rt::ct_query(v0, v1, v2, c0.w);
    LaneListAccess<COUNT> acc(sc, s_stack);
    rt::CpList list;
    rt::cp_list_init(list, MODE == rt::CC_ANY ? 0u : (max_contacts < rt::CT_CONTACT_MAX ? max_contacts : rt::CT_CONTACT_MAX), q.box.r); // the launch's list words hold no more
    if (rt::ct_query_valid(q)) { // degenerate queries list nothing, without a walk
        bool done = false;
        for (uint32_t s = 0; s < sc.n_spheres && !done; s++) { // the spheres by brute force, in index order
            float qu, qv;
            done = rt::cc_offer_sphere<MODE>(acc, list, rt::cp_order(rt::ct_sphere(sc.spheres[s].center, sc.spheres[s].radius, q, qu, qv), s), s);
        }
        if (!done) rt::ct_walk<MODE>(acc, sc.n_nodes, q, list);
    }
    uint4* rec = out + 2 * (size_t)i * max_contacts;
    LaneAccess<false> plain(sc, nullptr); // the records once more, uncounted
    for (uint32_t k = 0; k < list.cap; k++) {
        uint32_t r[8];
        rt::cp_answer_miss(q.box.r, r);
        if (k < list.n) {
            uint32_t d2, key, slot;
            acc.list_get(k, d2, key, slot);
            const uint64_t order = ((uint64_t)d2 << 32) | key;
            if (key & RT_PRIM_SPHERE_FLAG) { // a triangle's key
                float t[9];
                uint32_t ids[3];
                plain.record(slot, t, ids);
                rt::ct_answer_triangle(t, ids[0], order, q, r);
            } else {
                const DevSphere& s = sc.spheres[slot];
                rt::ct_answer_sphere(s.center, s.radius, s.material_id, order, q, r);
            }
        }
        rec[2 * k] = make_uint4(r[0], r[1], r[2], r[3]);
        rec[2 * k + 1] = make_uint4(r[4], r[5], r[6], r[7]);
    }
    if (counts) counts[i] = rt::cc_list_count<MODE>(list);
    if (COUNT) flush_counts(counters, acc.cnt);
}

template <int MODE>
void launch_mode(const DevScene& sc, const float4* triangles, uint4* out, uint32_t* counts, uint32_t n, uint32_t max_contacts, size_t lds,
                 unsigned long long* counters, hipStream_t stream) {
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    if (counters) hipLaunchKernelGGL((k_contact_triangle<true, MODE>), grid, block, lds, stream, sc, triangles, out, counts, n, max_contacts, counters);
    else hipLaunchKernelGGL((k_contact_triangle<false, MODE>), grid, block, lds, stream, sc, triangles, out, counts, n, max_contacts, counters);
}

} // namespace

namespace rt {

hipError_t launch_contact_triangle(const DevScene& sc, const void* triangles, void* out, uint32_t* counts, uint32_t n, uint32_t max_contacts, int mode,
                                   unsigned long long* counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (max_contacts > CT_CONTACT_MAX || (mode == CC_ANY && max_contacts != 0u) || (max_contacts != 0u && !out)) return hipErrorInvalidValue;
    const size_t lds = lane_stack_bytes(sc) + (size_t)max_contacts * 3u * WAVE * sizeof(uint32_t); // stack + list
    const float4* c = reinterpret_cast<const float4*>(triangles);
    uint4* o = reinterpret_cast<uint4*>(out);
    switch (mode) {
    case CC_LIST: launch_mode<CC_LIST>(sc, c, o, counts, n, max_contacts, lds, counters, stream); break;
    case CC_COUNT_ALL: launch_mode<CC_COUNT_ALL>(sc, c, o, counts, n, max_contacts, lds, counters, stream); break;
    case CC_ANY: launch_mode<CC_ANY>(sc, c, o, counts, n, max_contacts, lds, counters, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace rt
