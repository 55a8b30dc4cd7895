// Host check of the overlap query (gpu_raytracer_amd/csrc/overlap_rules.h), built by tests/test_overlap_abi.py with AddressSanitizer +
// UBSan.  It builds trees with bvh_builder.cpp on check_closest_point's inputs and asks about boxes centred on check_closest_point's
// points - half extents (1, 0.5, 1.5) x {0.02, 0.08, 0.25, 0.6} by index, then flat boxes, segments, points, a box around the whole
// scene and degenerate queries - the way the kernel does: ov_sphere for the spheres, ov_walk for the tree, with a host-side stack and
// list whose every index is checked against what the kernel's launch provides, for K in {1, 4, 32} with and without COUNT_ALL and in
// ANY mode, and compares every id and count with a brute force over all records and spheres by the same rules.  A child box culled
// with a touching triangle under it, a key lost across the K-th place, a primitive counted twice, a non-finite triangle listed, or a
// list or stack that outgrows its words shows here, before any kernel runs.
// usage: check_overlap <n_triangles> <seed> <kind> [method]   as check_closest_point
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "bvh_builder.h"
#include "host_access.h"
#include "overlap_rules.h"

using namespace rt;

namespace {

int g_fail = 0;
const uint32_t K_MAX = 32u; // RT_OVERLAP_MAX

struct Sphere {
    float centre[3], radius;
};

struct Query {
    float c[3], h[3];
    bool small; // one of the two small sizes on an ordinary centre: what the culling figure is taken over
};

// what k_overlap_box does for one lane: K ids and the count
template <int MODE>
uint32_t kernel_lane(HostKeyAccess& acc, const std::vector<Sphere>& spheres, const Query& q, uint32_t K, uint32_t* out) {
    acc.list.assign((size_t)K, 0xDEADBEEFu);
    OvList list;
    ov_list_init(list, MODE == OV_ANY ? 0u : K);
    if (ov_query_valid(q.c, q.h)) {
        OvBox box;
        ov_box_init(box, q.c, q.h);
        for (uint32_t s = 0; s < spheres.size(); s++) {
            if (MODE == OV_ANY && list.total) break;
            if (ov_list_wants<MODE>(list, s) && ov_sphere(spheres[s].centre, spheres[s].radius, q.c, q.h)) ov_list_offer(acc, list, s);
        }
        if (MODE != OV_ANY || list.total == 0u) ov_walk<MODE>(acc, (uint32_t)acc.b->nodes.size(), box, list);
    }
    for (uint32_t k = 0; k < list.cap; k++) out[k] = k < list.n ? (acc.list_get(k) ^ RT_PRIM_SPHERE_FLAG) : RT_PRIM_MISS;
    return ov_list_count<MODE>(list);
}

} // namespace

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atoll(argv[1]) : 1000;
    const uint32_t seed = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 1;
    const int kind = argc > 3 ? std::atoi(argv[3]) : 0;
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<BuildTri> tris(n);
    for (size_t i = 0; i < n; i++) { // check_bvh's inputs
        BuildTri& t = tris[i];
        t.material_id = (uint32_t)(i % 5);
        t.prim_id = (uint32_t)i;
        float c[3] = {u(rng) * 10, u(rng) * 10, u(rng) * 10}, s = 0.3f;
        if (kind == 1) c[2] = -3.0f;
        if (kind == 2) c[0] = c[1] = c[2] = 1.25f, s = 0.0f;
        if (kind == 3) c[0] = std::pow(1.001f, (float)i), c[1] = 0.0f, c[2] = 0.0f, s = 1e-3f;
        if (kind == 4) s = (i % 97 == 0) ? 1e5f : 1e-4f;
        for (int a = 0; a < 3; a++) {
            t.v0[a] = c[a] + u(rng) * s;
            t.v1[a] = c[a] + u(rng) * s;
            t.v2[a] = c[a] + u(rng) * s;
            if (kind == 1 && a == 2) t.v0[a] = t.v1[a] = t.v2[a] = -3.0f;
        }
        if (kind == 5 && i % 7 == 0) t.v1[i % 3] = (i % 14 == 0) ? std::numeric_limits<float>::quiet_NaN() : std::numeric_limits<float>::infinity();
    }
    BvhBuild b;
    BvhBuildOptions opt;
    opt.method = argc > 4 ? std::atoi(argv[4]) : 0;
    build_bvh(tris.data(), tris.size(), opt, b);
    const std::vector<Sphere> spheres = {{{2.0f, 1.0f, -1.0f}, 0.75f}, {{-4.0f, 0.5f, 3.0f}, 1.5f}, {{2.0f, 1.0f, -1.0f}, 0.75f}};

    // the leaves' records: padding records are not triangles
    std::vector<uint32_t> recs;
    for (size_t first = 0; first + RT_DEV_LEAF_STRIDE <= b.tris.size(); first += RT_DEV_LEAF_STRIDE)
        for (uint32_t x = 0; x < b.tris[first].leaf_count && x < RT_DEV_LEAF_STRIDE; x++) recs.push_back((uint32_t)(first + x));

    // boxes on check_closest_point's points: near surfaces, on vertices and on surfaces, scattered, far outside, with coordinates
    // around 1e4, on and in a sphere; then flat boxes, segments and points on vertices, a box around everything, degenerate queries
    std::vector<Query> qs;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float extent[3] = {1.0f, 0.5f, 1.5f}, sizes[4] = {0.02f, 0.08f, 0.25f, 0.6f};
    auto sized = [&](Query& q, size_t k, bool ordinary) {
        for (int a = 0; a < 3; a++) q.h[a] = extent[a] * sizes[k % 4];
        q.small = ordinary && k % 4 < 2;
    };
    const size_t n_each = 96;
    for (size_t k = 0; k < n_each && !recs.empty(); k++) {
        const DevTri& t = b.tris[recs[rng() % recs.size()]];
        const float bu = 0.5f * (u(rng) + 1.0f) * 0.5f, bv = 0.5f * (u(rng) + 1.0f) * 0.5f;
        Query near, vert, surf, flat;
        for (int a = 0; a < 3; a++) {
            surf.c[a] = t.v0[a] + (t.e1[a] * bu + t.e2[a] * bv);
            near.c[a] = surf.c[a] + u(rng) * 0.05f;
            vert.c[a] = k % 3 == 0 ? t.v0[a] : k % 3 == 1 ? t.v0[a] + t.e1[a] : t.v0[a] + t.e2[a];
        }
        sized(near, k, true), sized(vert, k + 1, true), sized(surf, k + 2, true);
        flat = vert; // a slab, a segment, a point on a vertex, by index
        flat.small = false;
        for (int a = 0; a < 3; a++) flat.h[a] = ((k + (size_t)a) % 4 < 1 + k % 3) ? 0.0f : 0.2f;
        qs.push_back(near), qs.push_back(vert), qs.push_back(surf), qs.push_back(flat);
    }
    for (size_t k = 0; k < n_each; k++) {
        Query scat, far, big;
        for (int a = 0; a < 3; a++) scat.c[a] = u(rng) * 12.0f, far.c[a] = u(rng) * 3000.0f, big.c[a] = 1e4f + u(rng) * 50.0f;
        sized(scat, k, true), sized(far, k, false), sized(big, k, false);
        qs.push_back(scat), qs.push_back(far), qs.push_back(big);
    }
    qs.push_back({{2.0f, 1.0f, -1.0f}, {0.1f, 0.1f, 0.1f}, false});      // wholly inside the coincident spheres: not touched
    qs.push_back({{2.0f, 1.0f, -1.0f}, {0.5f, 0.5f, 0.5f}, false});      // its corners pass through their surface
    qs.push_back({{2.75f, 1.0f, -1.0f}, {0.0f, 0.0f, 0.0f}, false});     // a point on it
    qs.push_back({{0.0f, 0.0f, 0.0f}, {2.0e5f, 2.0e5f, 2.0e5f}, false}); // around everything finite
    qs.push_back({{0.0f, 0.0f, 0.0f}, {3.0e38f, 3.0e38f, 3.0e38f}, false}); // c + h stays finite, the products overflow
    qs.push_back({{nan, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}, false});        // degenerate: nothing, without a walk
    qs.push_back({{0.0f, inf, 0.0f}, {1.0f, 1.0f, 1.0f}, false});
    qs.push_back({{0.0f, 0.0f, 0.0f}, {1.0f, nan, 1.0f}, false});
    qs.push_back({{0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, inf}, false});
    qs.push_back({{0.0f, 0.0f, 0.0f}, {1.0f, -1.0f, 1.0f}, false});
    const size_t n_degenerate = 5;

    const uint32_t Ks[3] = {1u, 4u, K_MAX};
    HostKeyAccess acc[3][2], any;
    for (auto& row : acc)
        for (HostKeyAccess& a : row) a.init(b);
    any.init(b);
    size_t listed[3] = {0, 0, 0}, overfull[3] = {0, 0, 0}, n_small = 0, touched = 0;
    unsigned long long small_nodes = 0, small_tris = 0;
    int fails[3][2] = {{0, 0}, {0, 0}, {0, 0}}, any_fails = 0, nonfinite_listed = 0;
    std::vector<uint32_t> keys; // every touching primitive's key
    for (size_t k = 0; k < qs.size(); k++) {
        const Query& q = qs[k];
        const bool ok = ov_query_valid(q.c, q.h);
        keys.clear();
        if (ok) {
            for (uint32_t s = 0; s < spheres.size(); s++)
                if (ov_sphere(spheres[s].centre, spheres[s].radius, q.c, q.h)) keys.push_back(s);
            for (uint32_t r : recs) {
                const DevTri& t = b.tris[r];
                if (ov_triangle(t.v0, t.e1, t.e2, q.c, q.h)) keys.push_back(t.prim_id ^ RT_PRIM_SPHERE_FLAG);
            }
            for (const BuildTri& t : tris) { // a triangle with a non-finite vertex is never listed, wherever it is stored
                bool finite = true;
                float e1[3], e2[3];
                for (int a = 0; a < 3; a++) {
                    finite = finite && std::isfinite(t.v0[a]) && std::isfinite(t.v1[a]) && std::isfinite(t.v2[a]);
                    e1[a] = t.v1[a] - t.v0[a], e2[a] = t.v2[a] - t.v0[a];
                }
                if (!finite && ov_triangle(t.v0, e1, e2, q.c, q.h)) nonfinite_listed++;
            }
        } else if (k + n_degenerate < qs.size()) {
            std::printf("FAIL: box %zu is degenerate\n", k);
            g_fail++;
        }
        std::sort(keys.begin(), keys.end());
        const uint32_t total = (uint32_t)keys.size();
        touched += total > 0;
        for (int ki = 0; ki < 3; ki++)
            for (int all = 0; all < 2; all++) {
                const uint32_t K = Ks[ki];
                HostKeyAccess& a = acc[ki][all];
                uint32_t got[K_MAX], want[K_MAX];
                const unsigned long long n1 = a.nodes, t1 = a.tris;
                const uint32_t got_count = all ? kernel_lane<OV_COUNT_ALL>(a, spheres, q, K, got) : kernel_lane<OV_LIST>(a, spheres, q, K, got);
                const uint32_t written = total < K ? total : K;
                for (uint32_t j = 0; j < K; j++) want[j] = j < written ? (keys[j] ^ RT_PRIM_SPHERE_FLAG) : RT_PRIM_MISS;
                const uint32_t want_count = all ? total : written;
                if (!all) listed[ki] += written, overfull[ki] += total > K;
                if (all && K == K_MAX && q.small) n_small++, small_nodes += a.nodes - n1, small_tris += a.tris - t1;
                bool bad = std::memcmp(got, want, (size_t)K * 4) != 0 || got_count != want_count;
                if (!ok) bad = bad || a.nodes != n1 || a.tris != t1; // no walk
                if (bad) {
                    if (g_fail < 20) {
                        uint32_t j = 0;
                        while (j + 1 < K && got[j] == want[j]) j++;
                        std::printf("FAIL: box %zu (%.9g %.9g %.9g | %.9g %.9g %.9g) K %u all %d: count %u, brute force %u; first difference at %u: prim %08x, "
                                    "brute force %08x; visits %llu tests %llu\n",
                                    k, q.c[0], q.c[1], q.c[2], q.h[0], q.h[1], q.h[2], K, all, got_count, want_count, j, got[j], want[j], a.nodes - n1, a.tris - t1);
                    }
                    g_fail++, fails[ki][all]++;
                }
            }
        uint32_t none[1];
        const unsigned long long n1 = any.nodes;
        const uint32_t got_any = kernel_lane<OV_ANY>(any, spheres, q, 0u, none);
        if (got_any != (total ? 1u : 0u) || (!ok && any.nodes != n1)) {
            if (g_fail < 20) std::printf("FAIL: box %zu ANY: %u, brute force total %u\n", k, got_any, total);
            g_fail++, any_fails++;
        }
    }
    if (nonfinite_listed) {
        std::printf("FAIL: %d triangles with a non-finite vertex pass the statement\n", nonfinite_listed);
        g_fail++;
    }
    const double nq = (double)qs.size();
    for (int ki = 0; ki < 3; ki++)
        for (int all = 0; all < 2; all++)
            std::printf("K %2u%s: %d failed, %.1f node visits and %.1f triangle tests per box, stack %d of %zu%s\n", Ks[ki], all ? " COUNT_ALL" : "          ",
                        fails[ki][all], (double)acc[ki][all].nodes / nq, (double)acc[ki][all].tris / nq, acc[ki][all].max_sp, acc[ki][all].stack.size(),
                        all ? "" : (", " + std::to_string(listed[ki]) + " ids listed, " + std::to_string(overfull[ki]) + " boxes with more").c_str());
    std::printf("ANY           : %d failed, %.1f node visits and %.1f triangle tests per box, stack %d of %zu, %zu of the boxes touched\n", any_fails,
                (double)any.nodes / nq, (double)any.tris / nq, any.max_sp, any.stack.size(), touched);
    std::printf("small boxes   : %.1f node visits and %.1f triangle tests per box over %zu boxes (brute force %zu)\n",
                n_small ? (double)small_nodes / (double)n_small : 0.0, n_small ? (double)small_tris / (double)n_small : 0.0, n_small, recs.size());
    std::printf("kind %d n %zu method %d: %zu nodes depth %u, %zu boxes x K {1, 4, 32} x {listed, COUNT_ALL} and ANY, %d failures\n", kind, n, opt.method,
                b.nodes.size(), b.depth, qs.size(), g_fail);
    return g_fail ? 1 : 0;
}
