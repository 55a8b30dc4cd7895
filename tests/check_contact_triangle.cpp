// Host check of the triangle contact query (gpu_raytracer_amd/csrc/contact_triangle_rules.h), built by
// tests/test_contact_triangle_abi.py with AddressSanitizer + UBSan.  It builds trees with bvh_builder.cpp on check_bvh's inputs and
// asks about resting triangles - small ones near surfaces, wide ones, in a scene triangle's plane, through a scene triangle, with
// an infinite margin, points and segments, corner queries (a vertex bit-equal to a record's vertex, the rest pointing away, at a
// margin just above 0), scattered, far outside, with coordinates around 1e4, around, across and inside the spheres, degenerate -
// the way the kernel does: cc_offer_sphere for the spheres, ct_walk for the tree, the listed primitives' records once more for the
// answers, with a host-side stack and list whose every index is checked against what the kernel's launch provides, for K in {1, 4,
// 16} with and without COUNT_ALL and in ANY mode, and compares every record's and count's bytes with a brute-force sort over all
// records and spheres by the same rules.  COUNT_ALL and ANY run with finite margins only: a query whose margin is infinite gets
// COUNT_ALL_MARGIN there.  A point query must also give cp_walk_all's records, count, node visits and triangle tests.  A bound that
// culls a box holding one of the K, a tie across the K-th place that is lost, a candidate counted twice, or a list or stack that
// outgrows its words shows here, before any kernel runs.
// usage: check_contact_triangle <n_triangles> <seed> <kind> [method]   as check_closest_point_all
//        check_contact_triangle eval <in> <out>   the statement alone: <in> holds records of 18 floats (v0 e1 e2 q0 q1 q2) or, where
//            e1 is (R, nan, nan), a sphere of centre v0 and radius R; <out> gets 5 floats each: dist2 qu qv v w (v = w = 0 for a sphere)
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
#include "contact_triangle_rules.h"
#include "host_access.h"

using namespace rt;

namespace {

int g_fail = 0;
const float COUNT_ALL_MARGIN = 2.0f;

struct Sphere {
    float centre[3], radius;
    uint32_t material;
};

struct Query {
    float v[3][3], margin;
    bool small; // a small triangle near a surface: what the culling figure is taken over
    uint32_t corner = 0xFFFFFFFFu; // a corner query: the record it was built on, which it must list at distance 0
};

void answer(const BvhBuild& b, const std::vector<Sphere>& spheres, uint64_t order, uint32_t slot, const CtQuery& q, uint32_t out[8]) {
    if ((uint32_t)order & RT_PRIM_SPHERE_FLAG) {
        const DevTri& t = b.tris[slot];
        float rec[9];
        for (int a = 0; a < 3; a++) rec[a] = t.v0[a], rec[3 + a] = t.e1[a], rec[6 + a] = t.e2[a];
        ct_answer_triangle(rec, t.material_id, order, q, out);
    } else {
        const Sphere& s = spheres[slot];
        ct_answer_sphere(s.centre, s.radius, s.material, order, q, out);
    }
}

// what k_contact_triangle does for one lane: K records and the count
template <int MODE>
uint32_t kernel_lane(HostListAccess& acc, const std::vector<Sphere>& spheres, const CtQuery& q, uint32_t K, uint32_t* out) {
    acc.list.assign((size_t)3 * K, 0xDEADBEEFu);
    CpList list;
    cp_list_init(list, MODE == CC_ANY ? 0u : K, q.box.r);
    if (ct_query_valid(q)) {
        bool done = false;
        for (uint32_t s = 0; s < spheres.size() && !done; s++) {
            float qu, qv;
            done = cc_offer_sphere<MODE>(acc, list, cp_order(ct_sphere(spheres[s].centre, spheres[s].radius, q, qu, qv), s), s);
        }
        if (!done) ct_walk<MODE>(acc, (uint32_t)acc.b->nodes.size(), q, list);
    }
    for (uint32_t k = 0; k < list.cap; k++) {
        cp_answer_miss(q.box.r, out + 8 * k);
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

int eval_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    std::FILE* g = std::fopen(out, "wb");
    if (!f || !g) return 2;
    float r[18];
    while (std::fread(r, sizeof(float), 18, f) == 18) {
        const CtQuery q = ct_query(r + 9, r + 12, r + 15, 1.0f);
        float o[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (std::isnan(r[4]) && std::isnan(r[5])) o[0] = ct_sphere(r, r[3], q, o[1], o[2]);
        else o[0] = ct_triangle(r, r + 3, r + 6, q, o[1], o[2], o[3], o[4]);
        std::fwrite(o, sizeof(float), 5, g);
    }
    std::fclose(f);
    return std::fclose(g) ? 2 : 0;
}

} // namespace

int main(int argc, char** argv) {
    if (argc > 3 && std::strcmp(argv[1], "eval") == 0) return eval_file(argv[2], argv[3]);
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

    std::vector<Query> qs;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const size_t n_each = n >= 10000 ? 24 : 64; // the brute force is n tests per query
    // a triangle of size `size` around `at`; by k mod 4: general, a segment (v2 == v1), a point, general
    auto around = [&](Query& q, const float at[3], float size, size_t k) {
        for (int j = 0; j < 3; j++)
            for (int a = 0; a < 3; a++) q.v[j][a] = at[a] + u(rng) * size;
        if (k % 4 == 1)
            for (int a = 0; a < 3; a++) q.v[2][a] = q.v[1][a];
        if (k % 4 == 2)
            for (int a = 0; a < 3; a++) q.v[1][a] = q.v[2][a] = q.v[0][a];
    };
    for (size_t k = 0; k < n_each && !recs.empty(); k++) {
        const uint32_t slot = recs[rng() % recs.size()];
        const DevTri& t = b.tris[slot];
        const float bu = 0.5f * (u(rng) + 1.0f) * 0.5f, bv = 0.5f * (u(rng) + 1.0f) * 0.5f;
        float surf[3], at[3];
        for (int a = 0; a < 3; a++)
            surf[a] = k % 4 == 0 ? t.v0[a] : k % 4 == 1 ? t.v0[a] + t.e1[a] * bu : t.v0[a] + (t.e1[a] * bu + t.e2[a] * bv); // vertex, edge, face
        Query small, wide, lying, pierce, open, corner;
        small.small = true, wide.small = lying.small = pierce.small = open.small = corner.small = false;
        // a small triangle near the surface: short lists
        small.margin = 0.05f;
        for (int a = 0; a < 3; a++) at[a] = surf[a] + u(rng) * 0.04f;
        around(small, at, 0.1f, 0);
        // a margin that holds a handful: lists that overflow K = 1 and 4
        wide.margin = 1.5f;
        for (int a = 0; a < 3; a++) at[a] = surf[a] + u(rng) * 0.3f;
        around(wide, at, 0.5f, k);
        // in the scene triangle's plane: distance 0 without piercing
        lying.margin = 0.1f;
        for (int j = 0; j < 3; j++) {
            const float p = u(rng), q2 = u(rng);
            for (int a = 0; a < 3; a++) lying.v[j][a] = t.v0[a] + (t.e1[a] * p + t.e2[a] * q2);
        }
        if (k % 3 == 0)
            for (int a = 0; a < 3; a++) lying.v[0][a] = surf[a];
        // through the scene triangle's interior, or pierced by one of its edges
        float nrm[3];
        sw_cross(t.e1, t.e2, nrm);
        const float nl = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
        pierce.margin = 0.02f;
        for (int a = 0; a < 3; a++) {
            const float nu = nl > 0.0f && std::isfinite(nl) ? nrm[a] / nl * 0.3f : 0.0f;
            const float mid = t.v0[a] + (t.e1[a] * 0.3f + t.e2[a] * 0.3f);
            pierce.v[0][a] = mid + nu + u(rng) * 0.03f;
            pierce.v[1][a] = mid - nu + u(rng) * 0.03f;
            pierce.v[2][a] = (k % 2 ? t.v0[a] + t.e1[a] * 2.0f : mid + nu) + u(rng) * 0.03f;
        }
        // an infinite margin: the K nearest of the whole scene
        open.margin = inf;
        for (int a = 0; a < 3; a++) at[a] = surf[a] + u(rng) * 0.5f;
        around(open, at, 0.4f, k + 3);
        // a corner query: a vertex bit-equal to the record's v0, the rest pointing away from the triangle, a margin just above 0 whose
        // square is still a normal f32 (a smaller one's square is 0, and nothing is below cp_start(0)): it must list the record it was
        // built on at distance 0, which a bound that culls the box touching only at that corner would lose
        corner.margin = 1e-18f;
        corner.corner = slot;
        for (int a = 0; a < 3; a++) {
            corner.v[0][a] = t.v0[a];
            corner.v[1][a] = t.v0[a] - (t.e1[a] + t.e2[a]) * 0.5f;
            corner.v[2][a] = t.v0[a] - (t.e1[a] * 0.25f + t.e2[a]);
        }
        if (k % 3 == 1) std::swap(corner.v[0], corner.v[2]);
        qs.push_back(small), qs.push_back(wide), qs.push_back(lying), qs.push_back(pierce), qs.push_back(open), qs.push_back(corner);
    }
    for (size_t k = 0; k < n_each; k++) {
        Query scat, far, big;
        scat.small = far.small = big.small = false;
        float at[3];
        for (int a = 0; a < 3; a++) at[a] = u(rng) * 12.0f;
        scat.margin = k % 2 ? 6.0f : 0.5f;
        around(scat, at, k % 3 ? 0.6f : 8.0f, k); // some large ones: the loose bound of a triangle askew to the axes
        for (int a = 0; a < 3; a++) at[a] = u(rng) * 3000.0f;
        far.margin = k % 2 ? inf : 100.0f;
        around(far, at, 1.0f, k + 1);
        for (int a = 0; a < 3; a++) at[a] = 1e4f + u(rng) * 50.0f;
        big.margin = k % 2 ? inf : 2.0e4f;
        around(big, at, k % 2 ? 3.0f : 0.1f, k + 2);
        qs.push_back(scat), qs.push_back(far), qs.push_back(big);
    }
    auto add = [&](float margin, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
        qs.push_back({{{ax, ay, az}, {bx, by, bz}, {cx, cy, cz}}, margin, false});
    };
    add(inf, 2.0f, 1.0f, -1.0f, 2.0f, 1.0f, -1.0f, 2.0f, 1.0f, -1.0f);     // a sphere's centre, a point (two coincident spheres: both listed, the lower index first)
    add(inf, 2.0f, 1.0f, -1.0f, 2.0f, 1.2f, -1.0f, 2.1f, 1.0f, -1.0f);     // from the centre, wholly inside
    add(inf, 2.1f, 1.2f, -0.9f, 2.2f, 1.2f, -0.9f, 2.1f, 1.3f, -0.9f);     // inside it
    add(1e-3f, 2.1f, 1.2f, -0.9f, 2.2f, 1.2f, -0.9f, 2.1f, 1.3f, -0.9f);   // ... and too far for this margin
    add(1.0f, 2.0f, 1.0f, -1.0f, 2.0f, 3.0f, -1.0f, 2.5f, 1.0f, -1.0f);    // from the centre through the surface
    add(0.5f, 1.0f, 1.0f, -1.0f, 3.0f, 1.0f, -1.0f, 1.0f, 3.0f, -1.0f);    // through it, all vertices outside, the nearest point inside
    add(0.5f, 2.0f, 1.75f, -1.0f, 2.0f, 1.75f, -1.0f, 2.0f, 1.75f, -1.0f); // on the surface, a point
    add(0.5f, 2.0f, 1.75f, -1.0f, 2.0f, 2.75f, -1.0f, 3.0f, 2.75f, -1.0f); // a vertex on the surface, outward
    add(20.0f, 9.0f, 0.0f, 3.0f, 9.0f, 1.0f, 3.0f, 9.0f, 0.0f, 4.0f);      // outside the other
    add(2.0f, -4.0f, 3.0f, 3.0f, -4.0f, 4.0f, 3.0f, -4.0f, 4.0f, 3.0f);    // ... a segment given as v2 == v1
    add(3.0e38f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f);    // margin * margin overflows to +inf: every finite distance is in range
    add(1.0f, 3.0e38f, 0.0f, 0.0f, -3.0e38f, 0.0f, 0.0f, 0.0f, 3.0e38f, 0.0f); // edges overflow to +inf: followed, nothing in range
    add(inf, nan, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f);         // degenerate: misses and a count of 0 without a walk
    add(1.0f, 0.0f, inf, 0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f);
    add(1.0f, 0.0f, 0.0f, 0.0f, 0.0f, nan, 0.0f, 1.0f, 0.0f, 0.0f);
    add(1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, -inf, 0.0f, 0.0f);
    add(nan, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f);
    add(0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f);
    add(-1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f);
    add(-inf, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f);

    const uint32_t Ks[3] = {1u, 4u, 16u};
    HostListAccess acc[3][2], any_acc, point_acc, small_acc;
    for (auto& row : acc)
        for (HostListAccess& a : row) a.init(b);
    any_acc.init(b), point_acc.init(b), small_acc.init(b);
    size_t listed[3] = {0, 0, 0}, overfull[3] = {0, 0, 0}, n_small = 0, n_point = 0, n_walked = 0, n_touching = 0, n_corner = 0, n_corner_found = 0;
    int fails[3][2] = {{0, 0}, {0, 0}, {0, 0}}, any_fails = 0, point_fails = 0;
    std::vector<std::pair<uint64_t, uint32_t>> cand; // (order, slot): every record and sphere in range of the finite margin
    for (size_t k = 0; k < qs.size(); k++) {
        for (int fin = 0; fin < 2; fin++) { // fin: the margin COUNT_ALL and ANY run with
            const float margin = fin && std::isinf(qs[k].margin) ? COUNT_ALL_MARGIN : qs[k].margin;
            if (fin && margin == qs[k].margin && k % 2 && !qs[k].small && qs[k].corner == 0xFFFFFFFFu) continue; // the finite margins once more under COUNT_ALL: every second query is enough (check_contact_capsule's rule); the small and the corner queries all run
            const CtQuery q = ct_query(qs[k].v[0], qs[k].v[1], qs[k].v[2], margin);
            const bool valid = ct_query_valid(q);
            cand.clear();
            if (valid) {
                const uint64_t start = cp_start(margin);
                for (uint32_t s = 0; s < spheres.size(); s++) {
                    float qu, qv;
                    const uint64_t c = cp_order(ct_sphere(spheres[s].centre, spheres[s].radius, q, qu, qv), s);
                    if (c < start) cand.push_back({c, s});
                }
                for (uint32_t r : recs) {
                    const DevTri& t = b.tris[r];
                    float qu, qv, v, w;
                    const uint64_t c = cp_order(ct_triangle(t.v0, t.e1, t.e2, q, qu, qv, v, w), t.prim_id ^ RT_PRIM_SPHERE_FLAG);
                    if (c < start) cand.push_back({c, r});
                }
                std::sort(cand.begin(), cand.end());
                n_walked += !fin;
                n_touching += !fin && !cand.empty() && (cand[0].first >> 32) == 0u;
                if (!fin && qs[k].corner != 0xFFFFFFFFu) { // the brute force itself must hold the corner's record at dist2 == 0; the walk is held to it below
                    const std::pair<uint64_t, uint32_t> own{cp_order(0.0f, b.tris[qs[k].corner].prim_id ^ RT_PRIM_SPHERE_FLAG), qs[k].corner};
                    n_corner++;
                    if (std::find(cand.begin(), cand.end(), own) != cand.end()) n_corner_found++;
                    else {
                        if (g_fail < 20) std::printf("FAIL: corner query %zu does not list record %u at distance 0 (%u in range)\n", k, qs[k].corner, (unsigned)cand.size());
                        g_fail++;
                    }
                }
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
                    cp_answer_miss(margin, want + 8 * j);
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
                        std::printf("FAIL: query %zu (%.9g %.9g %.9g | %.9g %.9g %.9g | %.9g %.9g %.9g margin %.9g) K %u all %d: count %u, brute force %u; first "
                                    "difference at record %u: prim %08x dist %.9g, brute force prim %08x dist %.9g\n",
                                    k, q.q[0][0], q.q[0][1], q.q[0][2], q.q[1][0], q.q[1][1], q.q[1][2], q.q[2][0], q.q[2][1], q.q[2][2], margin, K, all, got_count,
                                    want_count, j, got[8 * j + 6], cp_float(got[8 * j + 3]), want[8 * j + 6], cp_float(want[8 * j + 3]));
                    }
                    g_fail++, fails[ki][all]++;
                }
                // a point: rt_closest_point_all's records (qu = qv = 0 where u and v are), count and work
                if (!all && std::memcmp(q.q[0], q.q[1], 12) == 0 && std::memcmp(q.q[0], q.q[2], 12) == 0) {
                    uint32_t pt[16 * 8];
                    const unsigned long long n0 = point_acc.nodes, t0 = point_acc.tris;
                    const uint32_t pt_count = point_lane(point_acc, spheres, q.q[0], margin, K, pt);
                    bool differs = pt_count != got_count || a.nodes - n1 != point_acc.nodes - n0 || a.tris - t1 != point_acc.tris - t0;
                    for (uint32_t j = 0; j < K; j++)
                        differs = differs || std::memcmp(got + 8 * j, pt + 8 * j, 16) != 0 || std::memcmp(got + 8 * j + 6, pt + 8 * j + 6, 8) != 0 ||
                                  got[8 * j + 4] != 0u || got[8 * j + 5] != 0u;
                    n_point += ki == 0;
                    if (differs) {
                        if (g_fail < 20) std::printf("FAIL: query %zu K %u: a point differs from cp_walk_all (counts %u %u)\n", k, K, got_count, pt_count);
                        g_fail++, point_fails++;
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
                    if (g_fail < 20) std::printf("FAIL: query %zu ANY %u with %u in range; %llu tests, COUNT_ALL %llu\n", k, got_any, total, any_acc.tris - t1, small_acc.tris - t2);
                    g_fail++, any_fails++;
                }
                if (!qs[k].small) small_acc.tris = t2, small_acc.nodes = n2; // keeps the small triangles' work alone
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
    std::printf("points        : %d failed over %zu queries against cp_walk_all\n", point_fails, n_point);
    std::printf("corner queries: %zu of %zu list their record at distance 0\n", n_corner_found, n_corner);
    std::printf("small triangles: %.1f node visits and %.1f triangle tests per query over %zu queries (COUNT_ALL; brute force %zu)\n",
                n_small ? (double)small_acc.nodes / (double)n_small : 0.0, n_small ? (double)small_acc.tris / (double)n_small : 0.0, n_small, recs.size());
    std::printf("kind %d n %zu method %d: %zu nodes depth %u, %zu queries (%zu walked, %zu at distance 0) x K {1, 4, 16} x {listed, COUNT_ALL} + ANY, %d failures\n",
                kind, n, opt.method, b.nodes.size(), b.depth, qs.size(), n_walked, n_touching, g_fail);
    return g_fail ? 1 : 0;
}
