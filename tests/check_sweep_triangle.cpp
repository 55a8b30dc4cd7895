// Host check of the triangle sweep (gpu_raytracer_amd/csrc/sweep_triangle_rules.h), built by tests/test_sweep_triangle_abi.py with
// AddressSanitizer + UBSan.  It builds trees with bvh_builder.cpp on check_bvh's inputs, runs the walk the kernel runs - st_walk with
// the same per-node bound, order, stack discipline and leaf test (early returns included) - with a host-side stack whose index is
// checked against what the kernel's launch provides, and compares every answer's bytes with a brute force over all records and
// spheres by the same rules, without a limit on the time.  A bound that culls a box holding the winner, an early return that changes
// an answer, a visiting order that loses a tie, or a stack that outgrows its entries shows here, before any kernel runs.
// usage: check_sweep_triangle <n_triangles> <seed> <kind> [method]   as check_bvh: method 0 binned SAH (default), 1 PLOC; kind 0 soup,
//                    1 coplanar grid, 2 coincident points, 3 collinear chain, 4 huge + tiny mixed, 5 with NaN / inf vertices
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "bvh_builder.h"
#include "host_access.h"
#include "sweep_triangle_rules.h"

using namespace rt;

namespace {

int g_fail = 0;

struct Sphere {
    float centre[3], radius;
    uint32_t material;
};
struct Sweep {
    float v[3][3], d[3], tmax;
    bool small; // counted for the cull's figures
};

void answer(const BvhBuild& b, const std::vector<Sphere>& spheres, const CpBest& best, const StQuery& q, const Sweep& s, uint32_t out[8]) {
    sb_answer_miss(q.b.tmax, out);
    if (best.slot == 0xFFFFFFFFu) return;
    if ((uint32_t)best.order & RT_PRIM_SPHERE_FLAG) {
        const DevTri& t = b.tris[best.slot];
        float rec[9];
        for (int a = 0; a < 3; a++) rec[a] = t.v0[a], rec[3 + a] = t.e1[a], rec[6 + a] = t.e2[a];
        st_answer_triangle(rec, t.material_id, best.order, q, out);
    } else {
        const Sphere& sp = spheres[best.slot];
        st_answer_sphere(sp.centre, sp.radius, sp.material, best.order, q, s.v[1], s.v[2], out);
    }
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

    std::vector<Sweep> qs;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const size_t n_each = 96;
    // a triangle of size `size` around `at`, or the sliver (lo, lo, lo), (hi, hi, lo), (lo, hi, hi) of the box at -+ size / 2
    auto shape = [&](Sweep& s, const float at[3], float size, int form) {
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++) {
                if (form == 0) s.v[k][a] = at[a] + u(rng) * 0.5f * size;
                else if (form == 1) s.v[k][a] = at[a] + (((k == 1 && a < 2) || (k == 2 && a > 0)) ? 0.5f : -0.5f) * size;
                else if (form == 2) s.v[k][a] = k == 1 ? s.v[0][a] : at[a] + u(rng) * 0.5f * size; // a segment: q1 == q0
                else s.v[k][a] = at[a];                                                              // a point
            }
        if (form == 2 && (rng() & 1u))
            for (int a = 0; a < 3; a++) s.v[1][a] = s.v[0][a] + 2.0f * (s.v[2][a] - s.v[0][a]); // q2 on q0 q1
        s.small = size <= 0.3f;
    };
    auto aim = [&](Sweep& s, const float from[3], const float to[3], float speed) {
        for (int a = 0; a < 3; a++) s.d[a] = (to[a] - from[a]) * speed;
    };
    const float sizes[4] = {0.05f, 0.3f, 1.2f, 3.0f};
    for (size_t k = 0; k < n_each && !recs.empty(); k++) {
        const DevTri& t = b.tris[recs[rng() % recs.size()]];
        const float bu = 0.5f * (u(rng) + 1.0f) * 0.5f, bv = 0.5f * (u(rng) + 1.0f) * 0.5f;
        float surf[3], from[3], off[3];
        for (int a = 0; a < 3; a++) {
            surf[a] = k % 4 == 0 ? t.v0[a] : k % 4 == 1 ? t.v0[a] + t.e1[a] * bu : t.v0[a] + (t.e1[a] * bu + t.e2[a] * bv); // vertex, edge, face
            off[a] = u(rng);
            from[a] = surf[a] + off[a] * (k % 2 ? 1.5f : 8.0f);
        }
        Sweep toward, graze, touch, flat, corner;
        shape(toward, from, sizes[k % 4], (int)(k % 8 < 4 ? 0 : k % 4));
        toward.tmax = k % 5 == 4 ? 0.5f : inf; // some end before the contact
        aim(toward, from, surf, 0.2f + 2.4f * (u(rng) + 1.0f));
        // past the point along an axis, the sliver's bounds on another axis at the point's coordinate -+ 0.1 %
        const float gs = 0.1f + 0.2f * (u(rng) + 1.0f);
        const int along = (int)(k % 3), across = (int)((k + 1) % 3);
        float pass[3];
        for (int a = 0; a < 3; a++) pass[a] = surf[a], from[a] = surf[a];
        pass[across] = from[across] = surf[across] + (0.5f * gs + 1e-6f) * (k % 2 ? 1.001f : 0.999f);
        from[along] -= 3.0f;
        shape(graze, from, gs, 1);
        graze.tmax = inf;
        aim(graze, from, pass, 0.7f);
        // in contact at the start, or nearly: the point inside the sliver's bounds
        for (int a = 0; a < 3; a++) from[a] = surf[a] + off[a] * 0.05f;
        shape(touch, from, 0.4f, (int)(k % 2));
        touch.tmax = k % 3 == 0 ? 1e-30f : inf;
        aim(touch, from, surf, 1.0f);
        touch.d[k % 3] = 0.0f; // and a zero direction component
        // flat on flat: a triangle in a coordinate plane through the point, offset along that plane's axis and moving along it, with
        // exact coordinates on that axis; in the record's own plane where the scene is the coplanar grid (kind 1, z = -3)
        const int ax = kind == 1 ? 2 : (int)(k % 3);
        const bool sliding = kind == 1 && k % 2; // inside z = -3, toward the point from 1.5 steps away
        flat.d[0] = flat.d[1] = flat.d[2] = 0.0f;
        if (sliding) flat.d[(k / 2) % 2] = k % 4 == 1 ? 1.5f : -0.75f, flat.d[1 - (k / 2) % 2] = 0.25f * u(rng);
        else flat.d[ax] = -0.5f;
        for (int a = 0; a < 3; a++) from[a] = sliding ? surf[a] - 1.5f * flat.d[a] : surf[a];
        shape(flat, from, sizes[k % 3], (int)(k % 4 == 3 ? 2 : 0));
        const float level = sliding ? -3.0f : std::floor(surf[ax]) + 2.0f;
        for (int v = 0; v < 3; v++) flat.v[v][ax] = level;
        flat.tmax = inf;
        // a corner sweep: a point that moves along one axis through the record's vertex that is extreme on another axis, so that the
        // swept bounds - a segment - meet the record's bounds in a face's edge only
        const int run = (int)(k % 3), top = (int)((k + 1) % 3);
        const float* vs[3] = {t.v0, nullptr, nullptr};
        float s1[3], s2[3];
        for (int a = 0; a < 3; a++) s1[a] = t.v0[a] + t.e1[a], s2[a] = t.v0[a] + t.e2[a];
        vs[1] = s1, vs[2] = s2;
        const float* peak = vs[0];
        for (int v = 1; v < 3; v++)
            if (vs[v][top] > peak[top]) peak = vs[v];
        for (int a = 0; a < 3; a++) from[a] = peak[a];
        from[run] = peak[run] - 2.0f;
        shape(corner, from, 0.0f, 3);
        corner.d[0] = corner.d[1] = corner.d[2] = 0.0f;
        corner.d[run] = 1.0f;
        corner.tmax = inf;
        qs.push_back(toward), qs.push_back(graze), qs.push_back(touch), qs.push_back(flat), qs.push_back(corner);
    }
    for (size_t k = 0; k < n_each; k++) {
        Sweep scat, far, big;
        float to[3], from[3];
        for (int a = 0; a < 3; a++) to[a] = u(rng) * 10.0f, from[a] = u(rng) * 30.0f;
        shape(scat, from, k % 2 ? 0.3f : 2e-3f, (int)(k % 16 == 1 ? 3 : k % 16 == 2 ? 2 : 0));
        scat.tmax = k % 4 == 3 ? 0.9f : inf;
        aim(scat, from, to, 1.0f);
        if (k % 8 == 0) scat.d[0] = 0.0f, scat.d[1] = -0.0f; // along z
        for (int a = 0; a < 3; a++) from[a] = u(rng) * 3000.0f;
        shape(far, from, 0.25f, 0);
        far.tmax = inf;
        aim(far, from, to, 1e-3f);
        for (int a = 0; a < 3; a++) from[a] = 1e4f + u(rng) * 50.0f;
        shape(big, from, k % 2 ? 3.0f : 0.05f, 0);
        big.tmax = k % 2 ? inf : 2.0f;
        aim(big, from, to, 1.0f);
        qs.push_back(scat), qs.push_back(far), qs.push_back(big);
    }
    auto add = [&](float x0, float y0, float z0, float x1, float y1, float z1, float x2, float y2, float z2, float dx, float dy, float dz, float tmax) {
        qs.push_back({{{x0, y0, z0}, {x1, y1, z1}, {x2, y2, z2}}, {dx, dy, dz}, tmax, false});
    };
    add(2.0f, 1.0f, -1.0f, 2.1f, 1.0f, -1.0f, 2.0f, 1.1f, -1.0f, 0.3f, 0.2f, -0.1f, inf);   // from inside a sphere outward (two coincident: the lower index)
    add(2.0f, 1.0f, -1.0f, 2.1f, 1.0f, -1.0f, 2.0f, 1.1f, -1.0f, 0.3f, 0.2f, -0.1f, 1e-3f); // ... and too far for this tmax
    add(2.0f, 1.0f, -1.0f, 2.9f, 1.0f, -1.0f, 2.0f, 1.1f, -1.0f, 1.0f, 0.0f, 0.0f, inf);    // across its surface at the start
    add(9.0f, 0.5f, 3.0f, 9.0f, 0.7f, 3.1f, 9.0f, 0.4f, 3.3f, -2.0f, 0.0f, 0.0f, inf);     // toward the other from outside: face on
    add(9.0f, 0.5f, 3.0f, 9.5f, 0.5f, 3.0f, 9.5f, 0.6f, 3.2f, -2.0f, 0.0f, 0.0f, inf);     // ... a vertex first
    add(9.0f, 2.0f, 3.0f, 9.0f, 2.0f, 3.0f, 9.0f, -1.0f, 4.0f, -2.0f, -0.3f, 0.1f, inf);   // ... a segment
    add(-4.0f, 0.5f, 3.0f, -4.0f, 0.5f, 3.0f, -4.0f, 0.5f, 3.0f, 0.0f, 1.0f, 0.0f, inf);   // a point from its centre
    add(-1e6f, -1e6f, -50.0f, 1e6f, -1e6f, -50.0f, 0.0f, 1e6f, -50.0f, 0.0f, 0.0f, 1.0f, inf); // one triangle around everything, rising
    add(-1e6f, -1e6f, -1e6f, 1e6f, -1e6f, 1e6f, 0.0f, 1e6f, 0.0f, 0.1f, 0.2f, 0.3f, inf);       // ... and one that cuts everything
    add(-3e38f, -3e38f, 0.0f, 3e38f, -3e38f, 0.0f, 0.0f, 3e38f, 0.0f, 0.0f, 0.0f, 1.0f, inf);   // products that overflow
    add(-1e30f, -1e30f, -20.0f, 1e30f, -1e30f, -20.0f, 0.0f, 1e30f, -20.0f, 0.0f, 1e30f, 1.0f, inf);
    add(1e20f, 0.0f, 0.0f, 1e20f, 1.0f, 0.0f, 1e20f, 0.0f, 1.0f, -1e19f, 0.0f, 0.0f, inf);
    add(nan, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, -1.0f, inf); // not walked
    add(0.0f, 0.0f, 0.0f, 1.0f, inf, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, -1.0f, inf);
    add(0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, -inf, 0.0f, 0.0f, -1.0f, inf);
    add(0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, nan, -1.0f, inf);
    add(0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, inf, 0.0f, -1.0f, inf);
    add(0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, -0.0f, 0.0f, inf);
    add(0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, -1.0f, nan);
    add(0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, -1.0f, 0.0f);
    add(0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, -1.0f, -1.0f);

    HostAccess acc;
    acc.init(b);
    size_t found = 0, at_start = 0, by_axis[28] = {0}, n_small = 0;
    unsigned long long small_nodes = 0, small_tris = 0;
    for (size_t k = 0; k < qs.size(); k++) {
        const Sweep& s = qs[k];
        const StQuery q = st_query(s.v[0], s.v[1], s.v[2], s.d, s.tmax);
        uint32_t got[8], want[8];
        CpBest walk{sw_start(q.b.tmax), 0xFFFFFFFFu}, brute = walk;
        const unsigned long long nodes0 = acc.nodes, tris0 = acc.tris;
        if (st_query_valid(s.v[0], s.v[1], s.v[2], s.d, s.tmax)) {
            for (uint32_t i = 0; i < spheres.size(); i++) {
                const uint64_t c = cp_order(st_sphere(spheres[i].centre, spheres[i].radius, q, s.v[1], s.v[2]), i);
                if (c < walk.order) walk.order = c, walk.slot = i;
            }
            brute = walk;
            st_walk(acc, (uint32_t)b.nodes.size(), q, walk);
            for (uint32_t r : recs) {
                const DevTri& t = b.tris[r];
                uint32_t axis;
                float w_in;
                const uint64_t c = cp_order(st_triangle(t.v0, t.e1, t.e2, q, INFINITY, axis, w_in), t.prim_id ^ RT_PRIM_SPHERE_FLAG);
                if (c < brute.order) brute.order = c, brute.slot = r;
            }
        }
        if (s.small) n_small++, small_nodes += acc.nodes - nodes0, small_tris += acc.tris - tris0;
        answer(b, spheres, walk, q, s, got);
        answer(b, spheres, brute, q, s, want);
        found += want[6] != RT_PRIM_MISS;
        at_start += want[6] != RT_PRIM_MISS && want[3] == 0u;
        if (want[6] != RT_PRIM_MISS) by_axis[want[4] < 27u ? want[4] : 27u]++;
        if (std::memcmp(got, want, sizeof got) != 0) {
            if (g_fail < 20)
                std::printf("FAIL: sweep %zu (%.9g %.9g %.9g | %.9g %.9g %.9g | %.9g %.9g %.9g, d %.9g %.9g %.9g, tmax %.9g): walk prim %08x t %.9g axis %u, brute "
                            "force prim %08x t %.9g axis %u\n",
                            k, s.v[0][0], s.v[0][1], s.v[0][2], s.v[1][0], s.v[1][1], s.v[1][2], s.v[2][0], s.v[2][1], s.v[2][2], s.d[0], s.d[1], s.d[2], s.tmax,
                            got[6], cp_float(got[3]), got[4], want[6], cp_float(want[3]), want[4]);
            g_fail++;
        }
    }
    std::printf("axes 0..25, sphere, none:");
    for (size_t a = 0; a < 28; a++) std::printf(" %zu", by_axis[a]);
    std::printf("\nsmall sweeps: %.1f node visits and %.1f triangle tests per sweep over %zu sweeps\n", n_small ? (double)small_nodes / (double)n_small : 0.0,
                n_small ? (double)small_tris / (double)n_small : 0.0, n_small);
    std::printf("kind %d n %zu method %d: %zu nodes depth %u, %zu sweeps (%zu hit, %zu of them at the start), %.1f node visits and %.1f triangle tests per "
                "sweep (brute force %zu), stack %d of %zu, %d failures\n",
                kind, n, opt.method, b.nodes.size(), b.depth, qs.size(), found, at_start, (double)acc.nodes / (double)qs.size(),
                (double)acc.tris / (double)qs.size(), recs.size(), acc.max_sp, acc.stack.size(), g_fail);
    return g_fail ? 1 : 0;
}
