// Host check of the nearest-K query (gpu_raytracer_amd/csrc/closest_point_all_rules.h), built by tests/test_closest_point_all_abi.py
// with AddressSanitizer + UBSan.  It builds trees with bvh_builder.cpp on check_closest_point's inputs and asks about
// check_closest_point's points (a quarter of the on-surface ones with a radius of 1.5, which holds a handful), plus degenerate
// queries, the way the kernel does - cp_list_offer for the spheres, cp_walk_all for the tree, the listed
// primitives' records once more for the answers - with a host-side stack and list whose every index is checked against what the
// kernel's launch provides, for K in {1, 4, 16} with and without COUNT_ALL, and compares every record's and count's bytes with a
// brute-force sort over all records and spheres by the same rules.  COUNT_ALL runs with finite radii only: a query whose radius is
// infinite gets COUNT_ALL_RADIUS there.  At K = 1 the records, node visits and triangle tests must also be cp_walk's, query by query.
// A bound that culls a box holding one of the K, a tie across the K-th place that is lost, a candidate counted twice, or a list or
// stack that outgrows its words shows here, before any kernel runs.
// usage: check_closest_point_all <n_triangles> <seed> <kind> [method]   as check_closest_point
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "bvh_builder.h"
#include "closest_point_all_rules.h"
#include "host_access.h"

using namespace rt;

namespace {

int g_fail = 0;
const float COUNT_ALL_RADIUS = 2.0f;

struct Sphere {
    float centre[3], radius;
    uint32_t material;
};

struct Query {
    float p[3], radius;
};

// the record of the primitive `slot` with candidate `order`, alone
void answer(const BvhBuild& b, const std::vector<Sphere>& spheres, uint64_t order, uint32_t slot, const float p[3], uint32_t out[8]) {
    if ((uint32_t)order & RT_PRIM_SPHERE_FLAG) {
        const DevTri& t = b.tris[slot];
        float q[9];
        for (int a = 0; a < 3; a++) q[a] = t.v0[a], q[3 + a] = t.e1[a], q[6 + a] = t.e2[a];
        cp_answer_triangle(q, t.material_id, order, p, out);
    } else {
        const Sphere& s = spheres[slot];
        cp_answer_sphere(s.centre, s.radius, s.material, order, p, out);
    }
}

// what k_cp_nearest_all does for one lane: K records and the count
template <bool COUNT_ALL>
uint32_t kernel_lane(HostListAccess& acc, const std::vector<Sphere>& spheres, const Query& q, uint32_t K, uint32_t* out) {
    acc.list.assign((size_t)3 * K, 0xDEADBEEFu);
    CpList list;
    cp_list_init(list, K, q.radius);
    if (cp_query_valid(q.p, q.radius)) {
        for (uint32_t s = 0; s < spheres.size(); s++) {
            float pos[3];
            cp_list_offer<COUNT_ALL>(acc, list, cp_order(cp_sphere(spheres[s].centre, spheres[s].radius, q.p, pos), s), s);
        }
        cp_walk_all<COUNT_ALL>(acc, (uint32_t)acc.b->nodes.size(), q.p, list);
    }
    for (uint32_t k = 0; k < list.cap; k++) {
        cp_answer_miss(q.radius, out + 8 * k);
        if (k < list.n) {
            uint32_t d2, key, slot;
            acc.list_get(k, d2, key, slot);
            answer(*acc.b, spheres, ((uint64_t)d2 << 32) | key, slot, q.p, out + 8 * k);
        }
    }
    return cp_list_count<COUNT_ALL>(list);
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
    const std::vector<Sphere> spheres = {{{2.0f, 1.0f, -1.0f}, 0.75f, 1u}, {{-4.0f, 0.5f, 3.0f}, 1.5f, 2u}, {{2.0f, 1.0f, -1.0f}, 0.75f, 3u}};

    // the leaves' records: padding records are not triangles
    std::vector<uint32_t> recs;
    for (size_t first = 0; first + RT_DEV_LEAF_STRIDE <= b.tris.size(); first += RT_DEV_LEAF_STRIDE)
        for (uint32_t x = 0; x < b.tris[first].leaf_count && x < RT_DEV_LEAF_STRIDE; x++) recs.push_back((uint32_t)(first + x));

    // check_closest_point's points: near surfaces, on vertices and on surfaces, far outside, with coordinates around 1e4, inside and at
    // the centre of a sphere; then degenerate queries
    std::vector<Query> qs;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const size_t n_each = 96;
    for (size_t k = 0; k < n_each && !recs.empty(); k++) {
        const DevTri& t = b.tris[recs[rng() % recs.size()]];
        const float bu = 0.5f * (u(rng) + 1.0f) * 0.5f, bv = 0.5f * (u(rng) + 1.0f) * 0.5f;
        Query near, vert, surf;
        for (int a = 0; a < 3; a++) {
            surf.p[a] = t.v0[a] + (t.e1[a] * bu + t.e2[a] * bv);
            near.p[a] = surf.p[a] + u(rng) * 0.05f;
            vert.p[a] = k % 3 == 0 ? t.v0[a] : k % 3 == 1 ? t.v0[a] + t.e1[a] : t.v0[a] + t.e2[a];
        }
        near.radius = vert.radius = surf.radius = inf;
        if (k % 4 == 3) near.radius = 0.04f; // some within a finite radius, some not
        if (k % 4 == 2) surf.radius = 1.5f;  // ... and some that hold a handful
        qs.push_back(near), qs.push_back(vert), qs.push_back(surf);
    }
    for (size_t k = 0; k < n_each; k++) {
        Query scat, far, big;
        for (int a = 0; a < 3; a++) scat.p[a] = u(rng) * 30.0f, far.p[a] = u(rng) * 3000.0f, big.p[a] = 1e4f + u(rng) * 50.0f;
        scat.radius = k % 2 ? inf : 6.0f;
        far.radius = inf;
        big.radius = k % 2 ? inf : 2.0e4f;
        qs.push_back(scat), qs.push_back(far), qs.push_back(big);
    }
    qs.push_back({{2.0f, 1.0f, -1.0f}, inf});    // a sphere's centre (two coincident spheres: both listed, the lower index first)
    qs.push_back({{2.1f, 1.2f, -0.9f}, inf});    // inside it
    qs.push_back({{2.1f, 1.2f, -0.9f}, 1e-3f});  // ... and too far for this radius
    qs.push_back({{0.0f, 0.0f, 0.0f}, 3.0e38f}); // radius * radius overflows to +inf: every finite distance is in range
    qs.push_back({{nan, 0.0f, 0.0f}, inf});      // degenerate: misses and a count of 0 without a walk
    qs.push_back({{0.0f, inf, 0.0f}, 1.0f});
    qs.push_back({{0.0f, 0.0f, 0.0f}, nan});
    qs.push_back({{0.0f, 0.0f, 0.0f}, 0.0f});
    qs.push_back({{0.0f, 0.0f, 0.0f}, -1.0f});

    const uint32_t Ks[3] = {1u, 4u, 16u};
    HostListAccess acc[3][2];
    HostAccess single;
    for (auto& row : acc)
        for (HostListAccess& a : row) a.init(b);
    single.init(b);
    size_t listed[3] = {0, 0, 0}, overfull[3] = {0, 0, 0};
    int fails[3][2] = {{0, 0}, {0, 0}, {0, 0}};
    std::vector<std::pair<uint64_t, uint32_t>> cand; // (order, slot), every record and sphere
    for (size_t k = 0; k < qs.size(); k++) {
        const Query& q = qs[k];
        cand.clear();
        for (uint32_t s = 0; s < spheres.size(); s++) {
            float pos[3];
            cand.push_back({cp_order(cp_sphere(spheres[s].centre, spheres[s].radius, q.p, pos), s), s});
        }
        for (uint32_t r : recs) {
            const DevTri& t = b.tris[r];
            float v, w;
            cand.push_back({cp_order(cp_triangle(t.v0, t.e1, t.e2, q.p, v, w), t.prim_id ^ RT_PRIM_SPHERE_FLAG), r});
        }
        std::sort(cand.begin(), cand.end());
        // rt_closest_point's own walk
        uint32_t one[8];
        const unsigned long long n0 = single.nodes, t0 = single.tris;
        cp_answer_miss(q.radius, one);
        if (cp_query_valid(q.p, q.radius)) {
            CpBest best{cp_start(q.radius), 0xFFFFFFFFu};
            for (uint32_t s = 0; s < spheres.size(); s++) {
                float pos[3];
                const uint64_t c = cp_order(cp_sphere(spheres[s].centre, spheres[s].radius, q.p, pos), s);
                if (c < best.order) best.order = c, best.slot = s;
            }
            cp_walk(single, (uint32_t)b.nodes.size(), q.p, best);
            if (best.slot != 0xFFFFFFFFu) answer(b, spheres, best.order, best.slot, q.p, one);
        }
        for (int ki = 0; ki < 3; ki++)
            for (int all = 0; all < 2; all++) {
                const uint32_t K = Ks[ki];
                Query qq = q;
                if (all && std::isinf(q.radius)) qq.radius = COUNT_ALL_RADIUS;
                HostListAccess& a = acc[ki][all];
                uint32_t got[16 * 8], want[16 * 8];
                const unsigned long long n1 = a.nodes, t1 = a.tris;
                const uint32_t got_count = all ? kernel_lane<true>(a, spheres, qq, K, got) : kernel_lane<false>(a, spheres, qq, K, got);
                uint32_t total = 0;
                if (cp_query_valid(qq.p, qq.radius))
                    while (total < cand.size() && cand[total].first < cp_start(qq.radius)) total++; // sorted: the ones in range come first
                const uint32_t written = total < K ? total : K;
                for (uint32_t j = 0; j < K; j++) {
                    cp_answer_miss(qq.radius, want + 8 * j);
                    if (j < written) answer(b, spheres, cand[j].first, cand[j].second, qq.p, want + 8 * j);
                }
                const uint32_t want_count = all ? total : written;
                if (!all) listed[ki] += written, overfull[ki] += total > K;
                bool bad = std::memcmp(got, want, (size_t)K * 32) != 0 || got_count != want_count;
                if (K == 1 && !all) // and rt_closest_point's bytes and work
                    bad = bad || std::memcmp(got, one, 32) != 0 || a.nodes - n1 != single.nodes - n0 || a.tris - t1 != single.tris - t0;
                if (bad) {
                    if (g_fail < 20) {
                        uint32_t j = 0;
                        while (j + 1 < K && std::memcmp(got + 8 * j, want + 8 * j, 32) == 0) j++;
                        std::printf("FAIL: query %zu (%.9g %.9g %.9g r %.9g) K %u all %d: count %u, brute force %u; first difference at record %u: prim %08x "
                                    "dist %.9g, brute force prim %08x dist %.9g; visits %llu tests %llu, cp_walk %llu %llu\n",
                                    k, qq.p[0], qq.p[1], qq.p[2], qq.radius, K, all, got_count, want_count, j, got[8 * j + 6], cp_float(got[8 * j + 3]),
                                    want[8 * j + 6], cp_float(want[8 * j + 3]), a.nodes - n1, a.tris - t1, single.nodes - n0, single.tris - t0);
                    }
                    g_fail++, fails[ki][all]++;
                }
            }
    }
    const double nq = (double)qs.size();
    std::printf("rt_closest_point: %.1f node visits and %.1f triangle tests per query (brute force %zu)\n", (double)single.nodes / nq, (double)single.tris / nq,
                recs.size());
    for (int ki = 0; ki < 3; ki++)
        for (int all = 0; all < 2; all++)
            std::printf("K %2u%s: %d failed, %.1f node visits and %.1f triangle tests per query, stack %d of %zu%s\n", Ks[ki], all ? " COUNT_ALL" : "          ",
                        fails[ki][all], (double)acc[ki][all].nodes / nq, (double)acc[ki][all].tris / nq, acc[ki][all].max_sp, acc[ki][all].stack.size(),
                        all ? "" : (", " + std::to_string(listed[ki]) + " records listed, " + std::to_string(overfull[ki]) + " queries with more in range").c_str());
    std::printf("kind %d n %zu method %d: %zu nodes depth %u, %zu queries x K {1, 4, 16} x {listed, COUNT_ALL}, %d failures\n", kind, n, opt.method, b.nodes.size(),
                b.depth, qs.size(), g_fail);
    return g_fail ? 1 : 0;
}
