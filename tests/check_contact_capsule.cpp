// Host check of the contact query (gpu_raytracer_amd/csrc/contact_capsule_rules.h), built by tests/test_contact_capsule_abi.py with
// AddressSanitizer + UBSan.  It builds trees with bvh_builder.cpp on check_bvh's inputs and asks about resting capsules - near
// surfaces with axes that are zero, parallel to an edge, in a triangle's plane, upright and diagonal; lying on a surface; piercing a
// triangle; scattered, far outside, with coordinates around 1e4; around, across and inside the spheres; degenerate - the way the
// kernel does: cc_offer_sphere for the spheres, cc_walk for the tree, the listed primitives' records once more for the answers, with a
// host-side stack and list whose every index is checked against what the kernel's launch provides, for K in {1, 4, 16} with and
// without COUNT_ALL and in ANY mode, and compares every record's and count's bytes with a brute-force sort over all records and
// spheres by the same rules.  COUNT_ALL and ANY run with finite radii only: a query whose radius is infinite gets COUNT_ALL_RADIUS
// there.  A capsule with a zero axis must also give cp_walk_all's records, count, node visits and triangle tests.  A bound that culls
// a box holding one of the K, a tie across the K-th place that is lost, a candidate counted twice, or a list or stack that outgrows
// its words shows here, before any kernel runs.
// usage: check_contact_capsule <n_triangles> <seed> <kind> [method]   as check_closest_point_all
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
#include "contact_capsule_rules.h"
#include "host_access.h"

using namespace rt;

namespace {

int g_fail = 0;
const float COUNT_ALL_RADIUS = 2.0f;

struct Sphere {
    float centre[3], radius;
    uint32_t material;
};

struct Capsule {
    float A[3], r, ax[3];
    bool small; // a small capsule near a surface: what the culling figure is taken over
};

void answer(const BvhBuild& b, const std::vector<Sphere>& spheres, uint64_t order, uint32_t slot, const CcQuery& q, uint32_t out[8]) {
    if ((uint32_t)order & RT_PRIM_SPHERE_FLAG) {
        const DevTri& t = b.tris[slot];
        float rec[9];
        for (int a = 0; a < 3; a++) rec[a] = t.v0[a], rec[3 + a] = t.e1[a], rec[6 + a] = t.e2[a];
        cc_answer_triangle(rec, t.material_id, order, q, out);
    } else {
        const Sphere& s = spheres[slot];
        cc_answer_sphere(s.centre, s.radius, s.material, order, q, out);
    }
}

// what k_contact_capsule does for one lane: K records and the count
template <int MODE>
uint32_t kernel_lane(HostListAccess& acc, const std::vector<Sphere>& spheres, const CcQuery& q, uint32_t K, uint32_t* out) {
    acc.list.assign((size_t)3 * K, 0xDEADBEEFu);
    CpList list;
    cp_list_init(list, MODE == CC_ANY ? 0u : K, q.r);
    if (cc_query_valid(q)) {
        bool done = false;
        for (uint32_t s = 0; s < spheres.size() && !done; s++) {
            float place;
            done = cc_offer_sphere<MODE>(acc, list, cp_order(cc_sphere(spheres[s].centre, spheres[s].radius, q, place), s), s);
        }
        if (!done) cc_walk<MODE>(acc, (uint32_t)acc.b->nodes.size(), q, list);
    }
    for (uint32_t k = 0; k < list.cap; k++) {
        cp_answer_miss(q.r, out + 8 * k);
        if (k < list.n) {
            uint32_t d2, key, slot;
            acc.list_get(k, d2, key, slot);
            answer(*acc.b, spheres, ((uint64_t)d2 << 32) | key, slot, q, out + 8 * k);
        }
    }
    return cc_list_count<MODE>(list);
}

// rt_closest_point_all's lane for the same point and radius (check_closest_point_all's kernel_lane, list mode)
uint32_t point_lane(HostListAccess& acc, const std::vector<Sphere>& spheres, const float p[3], float radius, uint32_t K, uint32_t* out) {
    acc.list.assign((size_t)3 * K, 0xDEADBEEFu);
    CpList list;
    cp_list_init(list, K, radius);
    if (cp_query_valid(p, radius)) {
        for (uint32_t s = 0; s < spheres.size(); s++) {
            float pos[3];
            cp_list_offer<false>(acc, list, cp_order(cp_sphere(spheres[s].centre, spheres[s].radius, p, pos), s), s);
        }
        cp_walk_all<false>(acc, (uint32_t)acc.b->nodes.size(), p, list);
    }
    for (uint32_t k = 0; k < list.cap; k++) {
        cp_answer_miss(radius, out + 8 * k);
        if (k < list.n) {
            uint32_t d2, key, slot;
            acc.list_get(k, d2, key, slot);
            const uint64_t order = ((uint64_t)d2 << 32) | key;
            if (key & RT_PRIM_SPHERE_FLAG) {
                const DevTri& t = acc.b->tris[slot];
                float rec[9];
                for (int a = 0; a < 3; a++) rec[a] = t.v0[a], rec[3 + a] = t.e1[a], rec[6 + a] = t.e2[a];
                cp_answer_triangle(rec, t.material_id, order, p, out + 8 * k);
            } else {
                cp_answer_sphere(spheres[slot].centre, spheres[slot].radius, spheres[slot].material, order, p, out + 8 * k);
            }
        }
    }
    return cp_list_count<false>(list);
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

    std::vector<Capsule> qs;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const size_t n_each = 64;
    auto axis_of = [&](Capsule& c, const DevTri* t, size_t k, float len) { // by k mod 5: zero, along an edge, in the plane, upright, diagonal
        float x[3] = {u(rng), u(rng), u(rng)};
        const size_t kind5 = k % 5;
        if (kind5 == 1 && t)
            for (int a = 0; a < 3; a++) x[a] = t->e1[a];
        if (kind5 == 2 && t) {
            const float p = u(rng), q2 = u(rng);
            for (int a = 0; a < 3; a++) x[a] = t->e1[a] * p + t->e2[a] * q2;
        }
        if (kind5 == 3) x[0] = 0.0f, x[1] = 1.0f, x[2] = 0.0f;
        const float l = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        for (int a = 0; a < 3; a++) c.ax[a] = kind5 == 0 || !(l > 0.0f) || !std::isfinite(l) ? 0.0f : x[a] / l * len;
    };
    auto place = [&](Capsule& c, const float at[3], float where) { // the axis point at `where` lies at `at`
        for (int a = 0; a < 3; a++) c.A[a] = at[a] - c.ax[a] * where;
    };
    for (size_t k = 0; k < n_each && !recs.empty(); k++) {
        const DevTri& t = b.tris[recs[rng() % recs.size()]];
        const float bu = 0.5f * (u(rng) + 1.0f) * 0.5f, bv = 0.5f * (u(rng) + 1.0f) * 0.5f;
        float surf[3], at[3];
        for (int a = 0; a < 3; a++)
            surf[a] = k % 4 == 0 ? t.v0[a] : k % 4 == 1 ? t.v0[a] + t.e1[a] * bu : t.v0[a] + (t.e1[a] * bu + t.e2[a] * bv); // vertex, edge, face
        Capsule small, wide, lying, pierce, open;
        small.small = true, wide.small = lying.small = pierce.small = open.small = false;
        // a small capsule near the surface: short lists
        small.r = 0.05f;
        axis_of(small, &t, k, 0.3f);
        for (int a = 0; a < 3; a++) at[a] = surf[a] + u(rng) * 0.04f;
        place(small, at, 0.5f * (u(rng) + 1.0f));
        // a radius that holds a handful: lists that overflow K = 1 and 4
        wide.r = 1.5f;
        axis_of(wide, &t, k + 1, 0.2f + 0.5f * (u(rng) + 1.0f));
        for (int a = 0; a < 3; a++) at[a] = surf[a] + u(rng) * 0.3f;
        place(wide, at, 0.5f * (u(rng) + 1.0f));
        // on the surface: distance 0 without piercing (an axis in the plane, or an end on the point)
        lying.r = 0.1f;
        axis_of(lying, &t, k + 2, 0.25f);
        place(lying, surf, k % 2 ? 0.0f : 0.5f * (u(rng) + 1.0f));
        // through the triangle's interior, both ends farther than the radius from it
        float nrm[3];
        sw_cross(t.e1, t.e2, nrm);
        const float nl = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
        pierce.r = 0.02f;
        for (int a = 0; a < 3; a++) {
            pierce.ax[a] = nl > 0.0f && std::isfinite(nl) ? nrm[a] / nl * 0.3f + u(rng) * 0.03f : 0.0f;
            at[a] = t.v0[a] + (t.e1[a] * 0.3f + t.e2[a] * 0.3f);
        }
        place(pierce, at, 0.5f);
        // an infinite radius: the K nearest of the whole scene
        open.r = inf;
        axis_of(open, &t, k + 3, 0.5f);
        for (int a = 0; a < 3; a++) at[a] = surf[a] + u(rng) * 0.5f;
        place(open, at, 0.5f);
        qs.push_back(small), qs.push_back(wide), qs.push_back(lying), qs.push_back(pierce), qs.push_back(open);
    }
    for (size_t k = 0; k < n_each; k++) {
        Capsule scat, far, big;
        scat.small = far.small = big.small = false;
        float at[3];
        for (int a = 0; a < 3; a++) at[a] = u(rng) * 12.0f;
        scat.r = k % 2 ? 6.0f : 0.5f;
        axis_of(scat, nullptr, k, k % 3 ? 0.6f : 8.0f); // some long ones: the loose bound of a diagonal capsule
        place(scat, at, 0.5f);
        for (int a = 0; a < 3; a++) at[a] = u(rng) * 3000.0f;
        far.r = k % 2 ? inf : 100.0f;
        axis_of(far, nullptr, k + 1, 1.0f);
        place(far, at, 0.5f);
        for (int a = 0; a < 3; a++) at[a] = 1e4f + u(rng) * 50.0f;
        big.r = k % 2 ? inf : 2.0e4f;
        axis_of(big, nullptr, k + 2, k % 2 ? 3.0f : 0.1f);
        place(big, at, 0.5f);
        qs.push_back(scat), qs.push_back(far), qs.push_back(big);
    }
    auto add = [&](float x, float y, float z, float r, float ax, float ay, float az) { qs.push_back({{x, y, z}, r, {ax, ay, az}, false}); };
    add(2.0f, 1.0f, -1.0f, inf, 0.0f, 0.0f, 0.0f);     // a sphere's centre, zero axis (two coincident spheres: both listed, the lower index first)
    add(2.0f, 1.0f, -1.0f, inf, 0.0f, 0.2f, 0.0f);     // from the centre, wholly inside: end B is the farther
    add(2.1f, 1.2f, -0.9f, inf, 0.1f, 0.0f, 0.0f);     // inside it
    add(2.1f, 1.2f, -0.9f, 1e-3f, 0.1f, 0.0f, 0.0f);   // ... and too far for this radius
    add(2.0f, 1.0f, -1.0f, 1.0f, 0.0f, 2.0f, 0.0f);    // from the centre through the surface: the upper root
    add(1.0f, 1.0f, -1.0f, 0.5f, 2.0f, 0.0f, 0.0f);    // through it, both ends outside: the lower root
    add(2.0f, 1.75f, -1.0f, 0.5f, 0.0f, 0.0f, 0.0f);   // on the surface with a zero axis
    add(2.0f, 1.75f, -1.0f, 0.5f, 0.0f, 1.0f, 0.0f);   // end A on the surface, outward
    add(9.0f, 0.0f, 3.0f, 20.0f, 0.0f, 1.0f, 0.0f);    // outside the other: the foot inside the axis
    add(-4.0f, 3.0f, 3.0f, 2.0f, 0.0f, 1.0f, 0.0f);    // ... the foot at end A
    add(0.0f, 0.0f, 0.0f, 3.0e38f, 1.0f, 0.0f, 0.0f);  // radius * radius overflows to +inf: every finite distance is in range
    add(3.0e38f, 0.0f, 0.0f, 1.0f, 3.0e38f, 0.0f, 0.0f); // end B overflows to +inf: followed, nothing in range
    add(nan, 0.0f, 0.0f, inf, 0.0f, 1.0f, 0.0f);       // degenerate: misses and a count of 0 without a walk
    add(0.0f, inf, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f);
    add(0.0f, 0.0f, 0.0f, 1.0f, 0.0f, nan, 0.0f);
    add(0.0f, 0.0f, 0.0f, 1.0f, -inf, 0.0f, 0.0f);
    add(0.0f, 0.0f, 0.0f, nan, 0.0f, 1.0f, 0.0f);
    add(0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f);
    add(0.0f, 0.0f, 0.0f, -1.0f, 0.0f, 1.0f, 0.0f);

    const uint32_t Ks[3] = {1u, 4u, 16u};
    HostListAccess acc[3][2], any_acc, point_acc, small_acc;
    for (auto& row : acc)
        for (HostListAccess& a : row) a.init(b);
    any_acc.init(b), point_acc.init(b), small_acc.init(b);
    size_t listed[3] = {0, 0, 0}, overfull[3] = {0, 0, 0}, n_small = 0, n_zero = 0, n_walked = 0, n_pierced = 0;
    int fails[3][2] = {{0, 0}, {0, 0}, {0, 0}}, any_fails = 0, zero_fails = 0;
    std::vector<std::pair<uint64_t, uint32_t>> cand; // (order, slot): every record and sphere in range of the finite radius
    for (size_t k = 0; k < qs.size(); k++) {
        for (int fin = 0; fin < 2; fin++) { // fin: the radius COUNT_ALL and ANY run with
            const float radius = fin && std::isinf(qs[k].r) ? COUNT_ALL_RADIUS : qs[k].r;
            if (fin && radius == qs[k].r && k % 2 && !qs[k].small) continue; // the finite radii once more under COUNT_ALL: every second query is enough
            const CcQuery q = cc_query(qs[k].A, radius, qs[k].ax);
            const bool valid = cc_query_valid(q);
            cand.clear();
            if (valid) {
                const uint64_t start = cp_start(radius);
                for (uint32_t s = 0; s < spheres.size(); s++) {
                    float place;
                    const uint64_t c = cp_order(cc_sphere(spheres[s].centre, spheres[s].radius, q, place), s);
                    if (c < start) cand.push_back({c, s});
                }
                for (uint32_t r : recs) {
                    const DevTri& t = b.tris[r];
                    float s, v, w;
                    const uint64_t c = cp_order(cc_triangle(t.v0, t.e1, t.e2, q, s, v, w), t.prim_id ^ RT_PRIM_SPHERE_FLAG);
                    if (c < start) cand.push_back({c, r});
                }
                std::sort(cand.begin(), cand.end());
                n_walked += !fin;
                n_pierced += !fin && !cand.empty() && (cand[0].first >> 32) == 0u;
            }
            const uint32_t total = (uint32_t)cand.size();
            for (int ki = 0; ki < 3; ki++) {
                const int all = fin;
                const uint32_t K = Ks[ki];
                HostListAccess& a = acc[ki][all];
                uint32_t got[16 * 8], want[16 * 8];
                const unsigned long long n1 = a.nodes, t1 = a.tris;
                const uint32_t got_count = all ? kernel_lane<CC_COUNT_ALL>(a, spheres, q, K, got) : kernel_lane<CC_LIST>(a, spheres, q, K, got);
                const uint32_t written = total < K ? total : K;
                for (uint32_t j = 0; j < K; j++) {
                    cp_answer_miss(radius, want + 8 * j);
                    if (j < written) answer(b, spheres, cand[j].first, cand[j].second, q, want + 8 * j);
                }
                const uint32_t want_count = all ? total : written;
                if (!all) listed[ki] += written, overfull[ki] += total > K;
                bool bad = std::memcmp(got, want, (size_t)K * 32) != 0 || got_count != want_count;
                if (!valid) bad = bad || a.nodes != n1 || a.tris != t1; // degenerate: no walk
                if (bad) {
                    if (g_fail < 20) {
                        uint32_t j = 0;
                        while (j + 1 < K && std::memcmp(got + 8 * j, want + 8 * j, 32) == 0) j++;
                        std::printf("FAIL: capsule %zu (%.9g %.9g %.9g r %.9g axis %.9g %.9g %.9g) K %u all %d: count %u, brute force %u; first difference at "
                                    "record %u: prim %08x dist %.9g s %.9g, brute force prim %08x dist %.9g s %.9g\n",
                                    k, q.A[0], q.A[1], q.A[2], q.r, q.ax[0], q.ax[1], q.ax[2], K, all, got_count, want_count, j, got[8 * j + 6],
                                    cp_float(got[8 * j + 3]), cp_float(got[8 * j + 4]), want[8 * j + 6], cp_float(want[8 * j + 3]), cp_float(want[8 * j + 4]));
                    }
                    g_fail++, fails[ki][all]++;
                }
                // a zero axis: rt_closest_point_all's records (s and the reserved word 0 where u and v are), count and work
                if (!all && q.ax[0] == 0.0f && q.ax[1] == 0.0f && q.ax[2] == 0.0f) {
                    uint32_t pt[16 * 8];
                    const unsigned long long n0 = point_acc.nodes, t0 = point_acc.tris;
                    const uint32_t pt_count = point_lane(point_acc, spheres, q.A, radius, K, pt);
                    bool differs = pt_count != got_count || a.nodes - n1 != point_acc.nodes - n0 || a.tris - t1 != point_acc.tris - t0;
                    for (uint32_t j = 0; j < K; j++)
                        differs = differs || std::memcmp(got + 8 * j, pt + 8 * j, 16) != 0 || std::memcmp(got + 8 * j + 6, pt + 8 * j + 6, 8) != 0 ||
                                  got[8 * j + 4] != 0u || got[8 * j + 5] != 0u;
                    n_zero += ki == 0;
                    if (differs) {
                        if (g_fail < 20) std::printf("FAIL: capsule %zu K %u: a zero axis differs from cp_walk_all (counts %u %u)\n", k, K, got_count, pt_count);
                        g_fail++, zero_fails++;
                    }
                }
            }
            if (fin) { // ANY: 1 iff anything is in range, with no more tests than COUNT_ALL's
                uint32_t none[8];
                const unsigned long long t1 = any_acc.tris;
                const uint32_t got_any = kernel_lane<CC_ANY>(any_acc, spheres, q, 0u, none);
                const unsigned long long t2 = small_acc.tris, n2 = small_acc.nodes;
                const uint32_t got_all = kernel_lane<CC_COUNT_ALL>(small_acc, spheres, q, 0u, none);
                if (got_any != (total ? 1u : 0u) || got_all != total || any_acc.tris - t1 > small_acc.tris - t2) {
                    if (g_fail < 20) std::printf("FAIL: capsule %zu ANY %u with %u in range; %llu tests, COUNT_ALL %llu\n", k, got_any, total, any_acc.tris - t1, small_acc.tris - t2);
                    g_fail++, any_fails++;
                }
                if (!qs[k].small) small_acc.tris = t2, small_acc.nodes = n2; // keeps the small capsules' work alone
                else n_small++;
            }
        }
    }
    const double nq = (double)qs.size();
    for (int ki = 0; ki < 3; ki++)
        for (int all = 0; all < 2; all++)
            std::printf("K %2u%s: %d failed, %.1f node visits and %.1f triangle tests per query, stack %d of %zu%s\n", Ks[ki], all ? " COUNT_ALL" : "          ",
                        fails[ki][all], (double)acc[ki][all].nodes / nq, (double)acc[ki][all].tris / nq, acc[ki][all].max_sp, acc[ki][all].stack.size(),
                        all ? "" : (", " + std::to_string(listed[ki]) + " records listed, " + std::to_string(overfull[ki]) + " queries with more in range").c_str());
    std::printf("ANY           : %d failed, %.1f node visits and %.1f triangle tests per query\n", any_fails, (double)any_acc.nodes / nq, (double)any_acc.tris / nq);
    std::printf("zero axis     : %d failed over %zu capsules against cp_walk_all\n", zero_fails, n_zero);
    std::printf("small capsules: %.1f node visits and %.1f triangle tests per capsule over %zu capsules (COUNT_ALL; brute force %zu)\n",
                n_small ? (double)small_acc.nodes / (double)n_small : 0.0, n_small ? (double)small_acc.tris / (double)n_small : 0.0, n_small, recs.size());
    std::printf("kind %d n %zu method %d: %zu nodes depth %u, %zu capsules (%zu walked, %zu at distance 0) x K {1, 4, 16} x {listed, COUNT_ALL} + ANY, %d failures\n",
                kind, n, opt.method, b.nodes.size(), b.depth, qs.size(), n_walked, n_pierced, g_fail);
    return g_fail ? 1 : 0;
}
