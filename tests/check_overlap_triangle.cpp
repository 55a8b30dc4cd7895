// Host check of the triangle query (gpu_raytracer_amd/csrc/overlap_triangle_rules.h), built by tests/test_overlap_triangle_abi.py with
// AddressSanitizer + UBSan.  It builds trees with bvh_builder.cpp on check_closest_point's inputs and asks about triangles of four
// sizes - vertices within 0.03, 0.12, 0.4 and 1.0 of a centre, by index - centred near surfaces, on vertices and on surfaces,
// scattered and far outside, then segments and points on scene vertices, triangles that touch a primitive only at a corner of that
// primitive's bounds (one query vertex is a vertex of the record, the rest points away from it), a triangle around everything, one
// whose products overflow and non-finite ones - the way the kernel does: ot_sphere for the spheres, ot_walk for the tree, with a
// host-side stack and list whose every index is checked against what the kernel's launch provides, for K in {1, 4, 32} with and
// without COUNT_ALL and in ANY mode, and compares every id and count with a brute force over all records and spheres by the same
// rules.  A child box culled with a touching triangle under it, a key lost across the K-th place, a primitive counted twice, a
// non-finite triangle listed, or a list or stack that outgrows its words shows here, before any kernel runs.
// usage: check_overlap_triangle <n_triangles> <seed> <kind> [method]   as check_closest_point
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "bvh_builder.h"
#include "host_access.h"
#include "overlap_triangle_rules.h"

using namespace rt;

namespace {

int g_fail = 0;
const uint32_t K_MAX = 32u; // RT_OVERLAP_MAX

struct Sphere {
    float centre[3], radius;
};

struct Query {
    float v[3][3];
    bool small;          // one of the two small sizes on an ordinary centre: what the culling figure is taken over
    bool corner = false; // made on a corner of a record's bounds: it touches that record at least
};

// what k_overlap_triangle does for one lane: K ids and the count
template <int MODE>
uint32_t kernel_lane(HostKeyAccess& acc, const std::vector<Sphere>& spheres, const Query& t, uint32_t K, uint32_t* out) {
    acc.list.assign((size_t)K, 0xDEADBEEFu);
    OvList list;
    ov_list_init(list, MODE == OV_ANY ? 0u : K);
    if (ot_query_valid(t.v[0], t.v[1], t.v[2])) {
        OtQuery q;
        ot_query_init(q, t.v[0], t.v[1], t.v[2]);
        for (uint32_t s = 0; s < spheres.size(); s++) {
            if (MODE == OV_ANY && list.total) break;
            if (ov_list_wants<MODE>(list, s) && ot_sphere(spheres[s].centre, spheres[s].radius, q)) ov_list_offer(acc, list, s);
        }
        if (MODE != OV_ANY || list.total == 0u) ot_walk<MODE>(acc, (uint32_t)acc.b->nodes.size(), q, list);
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

    std::vector<Query> qs;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float sizes[4] = {0.03f, 0.12f, 0.4f, 1.0f};
    auto around = [&](const float c[3], size_t k, bool ordinary) { // a triangle with its vertices within sizes[k % 4] of c
        Query q;
        for (int j = 0; j < 3; j++)
            for (int a = 0; a < 3; a++) q.v[j][a] = c[a] + u(rng) * sizes[k % 4];
        q.small = ordinary && k % 4 < 2;
        return q;
    };
    auto record_vertex = [](const DevTri& t, int j, float out[3]) { // s_j, as the statement computes it
        for (int a = 0; a < 3; a++) out[a] = j == 0 ? t.v0[a] : j == 1 ? t.v0[a] + t.e1[a] : t.v0[a] + t.e2[a];
    };
    const size_t n_each = 96;
    size_t n_corner = 0;
    for (size_t k = 0; k < n_each && !recs.empty(); k++) {
        const DevTri& t = b.tris[recs[rng() % recs.size()]];
        const float bu = 0.5f * (u(rng) + 1.0f) * 0.5f, bv = 0.5f * (u(rng) + 1.0f) * 0.5f;
        float surf[3], near[3], vert[3];
        record_vertex(t, (int)(k % 3), vert);
        for (int a = 0; a < 3; a++) {
            surf[a] = t.v0[a] + (t.e1[a] * bu + t.e2[a] * bv);
            near[a] = surf[a] + u(rng) * 0.05f;
        }
        qs.push_back(around(near, k, true)), qs.push_back(around(vert, k + 1, true)), qs.push_back(around(surf, k + 2, true));
        Query flat; // a segment from a vertex, a segment along an edge, a point on a vertex, by index
        flat.small = false;
        float other[3];
        record_vertex(t, (int)((k + 1) % 3), other);
        for (int a = 0; a < 3; a++) {
            flat.v[0][a] = vert[a];
            flat.v[1][a] = k % 3 == 0 ? vert[a] + u(rng) * 0.2f : k % 3 == 1 ? other[a] : vert[a];
            flat.v[2][a] = k % 2 == 0 ? flat.v[1][a] : flat.v[0][a];
        }
        qs.push_back(flat);
        // touching at a corner of the record's bounds only: the record's lowest vertex on axis k % 3 is the query's q0, and the other
        // two query vertices lie away from the record on every axis on which q0 is the record's lowest or highest
        const int ax = (int)(k % 3);
        float s[3][3];
        for (int j = 0; j < 3; j++) record_vertex(t, j, s[j]);
        bool finite = true;
        for (int j = 0; j < 3; j++)
            for (int a = 0; a < 3; a++) finite = finite && std::isfinite(s[j][a]);
        if (!finite) continue;
        int j0 = 0;
        for (int j = 1; j < 3; j++)
            if (s[j][ax] < s[j0][ax]) j0 = j;
        Query corner;
        corner.small = false, corner.corner = true;
        for (int a = 0; a < 3; a++) {
            const float lo = std::min(std::min(s[0][a], s[1][a]), s[2][a]), hi = std::max(std::max(s[0][a], s[1][a]), s[2][a]);
            const float away = s[j0][a] == lo ? -1.0f : s[j0][a] == hi ? 1.0f : (u(rng) < 0.0f ? -1.0f : 1.0f);
            corner.v[0][a] = s[j0][a];
            corner.v[1][a] = s[j0][a] + away * (0.01f + 0.2f * std::fabs(u(rng)));
            corner.v[2][a] = s[j0][a] + away * (0.01f + 0.2f * std::fabs(u(rng)));
        }
        qs.push_back(corner), n_corner++;
    }
    for (size_t k = 0; k < n_each; k++) {
        float scat[3], far[3], big[3];
        for (int a = 0; a < 3; a++) scat[a] = u(rng) * 12.0f, far[a] = u(rng) * 3000.0f, big[a] = 1e4f + u(rng) * 50.0f;
        qs.push_back(around(scat, k, true)), qs.push_back(around(far, k, false)), qs.push_back(around(big, k, false));
    }
    qs.push_back({{{2.0f, 1.0f, -1.0f}, {2.1f, 1.0f, -1.0f}, {2.0f, 1.1f, -1.1f}}, false});   // wholly inside the coincident spheres: not touched
    qs.push_back({{{2.0f, 1.0f, -1.0f}, {3.0f, 1.0f, -1.0f}, {2.0f, 1.2f, -1.0f}}, false});   // one vertex outside: passes through their surface
    qs.push_back({{{2.75f, 1.0f, -1.0f}, {2.75f, 1.0f, -1.0f}, {2.75f, 1.0f, -1.0f}}, false}); // a point on it
    qs.push_back({{{-4.0e5f, -3.0e5f, 1.0f}, {4.0e5f, -3.0e5f, -2.0f}, {0.5f, 5.0e5f, 0.25f}}, false}); // around everything finite
    qs.push_back({{{-3.0e38f, -3.0e38f, 0.0f}, {3.0e38f, -3.0e38f, 0.0f}, {0.0f, 3.0e38f, 1.0f}}, false}); // finite vertices, the edges and products overflow
    qs.push_back({{{nan, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}}, false});       // non-finite: nothing, without a walk
    qs.push_back({{{0.0f, 0.0f, 0.0f}, {1.0f, inf, 0.0f}, {0.0f, 1.0f, 0.0f}}, false});
    qs.push_back({{{0.0f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, -inf}}, false});
    qs.push_back({{{0.0f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f}, {0.0f, nan, 0.0f}}, false});
    const size_t n_degenerate = 4;

    const uint32_t Ks[3] = {1u, 4u, K_MAX};
    HostKeyAccess acc[3][2], any;
    for (auto& row : acc)
        for (HostKeyAccess& a : row) a.init(b);
    any.init(b);
    size_t listed[3] = {0, 0, 0}, overfull[3] = {0, 0, 0}, n_small = 0, touched = 0, corner_touch = 0;
    unsigned long long small_nodes = 0, small_tris = 0;
    int fails[3][2] = {{0, 0}, {0, 0}, {0, 0}}, any_fails = 0, nonfinite_listed = 0;
    std::vector<uint32_t> keys; // every touching primitive's key
    for (size_t k = 0; k < qs.size(); k++) {
        const Query& t = qs[k];
        const bool ok = ot_query_valid(t.v[0], t.v[1], t.v[2]);
        keys.clear();
        if (ok) {
            OtQuery q;
            ot_query_init(q, t.v[0], t.v[1], t.v[2]);
            for (uint32_t s = 0; s < spheres.size(); s++)
                if (ot_sphere(spheres[s].centre, spheres[s].radius, q)) keys.push_back(s);
            for (uint32_t r : recs) {
                const DevTri& rec = b.tris[r];
                if (ot_triangle(rec.v0, rec.e1, rec.e2, q)) keys.push_back(rec.prim_id ^ RT_PRIM_SPHERE_FLAG);
            }
            for (const BuildTri& bt : tris) { // a triangle with a non-finite vertex is never listed, wherever it is stored
                bool finite = true;
                float e1[3], e2[3];
                for (int a = 0; a < 3; a++) {
                    finite = finite && std::isfinite(bt.v0[a]) && std::isfinite(bt.v1[a]) && std::isfinite(bt.v2[a]);
                    e1[a] = bt.v1[a] - bt.v0[a], e2[a] = bt.v2[a] - bt.v0[a];
                }
                if (!finite && ot_triangle(bt.v0, e1, e2, q)) nonfinite_listed++;
            }
        } else if (k + n_degenerate < qs.size()) {
            std::printf("FAIL: triangle %zu is not finite\n", k);
            g_fail++;
        }
        std::sort(keys.begin(), keys.end());
        const uint32_t total = (uint32_t)keys.size();
        touched += total > 0;
        corner_touch += t.corner && total > 0;
        for (int ki = 0; ki < 3; ki++)
            for (int all = 0; all < 2; all++) {
                const uint32_t K = Ks[ki];
                HostKeyAccess& a = acc[ki][all];
                uint32_t got[K_MAX], want[K_MAX];
                const unsigned long long n1 = a.nodes, t1 = a.tris;
                const uint32_t got_count = all ? kernel_lane<OV_COUNT_ALL>(a, spheres, t, K, got) : kernel_lane<OV_LIST>(a, spheres, t, K, got);
                const uint32_t written = total < K ? total : K;
                for (uint32_t j = 0; j < K; j++) want[j] = j < written ? (keys[j] ^ RT_PRIM_SPHERE_FLAG) : RT_PRIM_MISS;
                const uint32_t want_count = all ? total : written;
                if (!all) listed[ki] += written, overfull[ki] += total > K;
                if (all && K == K_MAX && t.small) n_small++, small_nodes += a.nodes - n1, small_tris += a.tris - t1;
                bool bad = std::memcmp(got, want, (size_t)K * 4) != 0 || got_count != want_count;
                if (!ok) bad = bad || a.nodes != n1 || a.tris != t1; // no walk
                if (bad) {
                    if (g_fail < 20) {
                        uint32_t j = 0;
                        while (j + 1 < K && got[j] == want[j]) j++;
                        std::printf("FAIL: triangle %zu (%.9g %.9g %.9g | %.9g %.9g %.9g | %.9g %.9g %.9g) K %u all %d: count %u, brute force %u; first "
                                    "difference at %u: prim %08x, brute force %08x; visits %llu tests %llu\n",
                                    k, t.v[0][0], t.v[0][1], t.v[0][2], t.v[1][0], t.v[1][1], t.v[1][2], t.v[2][0], t.v[2][1], t.v[2][2], K, all, got_count,
                                    want_count, j, got[j], want[j], a.nodes - n1, a.tris - t1);
                    }
                    g_fail++, fails[ki][all]++;
                }
            }
        uint32_t none[1];
        const unsigned long long n1 = any.nodes;
        const uint32_t got_any = kernel_lane<OV_ANY>(any, spheres, t, 0u, none);
        if (got_any != (total ? 1u : 0u) || (!ok && any.nodes != n1)) {
            if (g_fail < 20) std::printf("FAIL: triangle %zu ANY: %u, brute force total %u\n", k, got_any, total);
            g_fail++, any_fails++;
        }
    }
    if (corner_touch != n_corner) { // its q0 is a record's s_j bit for bit, so every span of that pair holds 0 on both sides
        std::printf("FAIL: %zu of the %zu corner queries touch nothing\n", n_corner - corner_touch, n_corner);
        g_fail++;
    }
    if (nonfinite_listed) {
        std::printf("FAIL: %d triangles with a non-finite vertex pass the statement\n", nonfinite_listed);
        g_fail++;
    }
    const double nq = (double)qs.size();
    for (int ki = 0; ki < 3; ki++)
        for (int all = 0; all < 2; all++)
            std::printf("K %2u%s: %d failed, %.1f node visits and %.1f triangle tests per triangle, stack %d of %zu%s\n", Ks[ki], all ? " COUNT_ALL" : "          ",
                        fails[ki][all], (double)acc[ki][all].nodes / nq, (double)acc[ki][all].tris / nq, acc[ki][all].max_sp, acc[ki][all].stack.size(),
                        all ? "" : (", " + std::to_string(listed[ki]) + " ids listed, " + std::to_string(overfull[ki]) + " triangles with more").c_str());
    std::printf("ANY           : %d failed, %.1f node visits and %.1f triangle tests per triangle, stack %d of %zu, %zu of the triangles touched\n", any_fails,
                (double)any.nodes / nq, (double)any.tris / nq, any.max_sp, any.stack.size(), touched);
    std::printf("small queries : %.1f node visits and %.1f triangle tests per triangle over %zu triangles (brute force %zu)\n",
                n_small ? (double)small_nodes / (double)n_small : 0.0, n_small ? (double)small_tris / (double)n_small : 0.0, n_small, recs.size());
    std::printf("corner queries: %zu made, %zu of them touch\n", n_corner, corner_touch);
    std::printf("kind %d n %zu method %d: %zu nodes depth %u, %zu triangles x K {1, 4, 32} x {listed, COUNT_ALL} and ANY, %d failures\n", kind, n, opt.method,
                b.nodes.size(), b.depth, qs.size(), g_fail);
    return g_fail ? 1 : 0;
}
