// Host check of the box sweep (gpu_raytracer_amd/csrc/sweep_box_rules.h), built by tests/test_sweep_box_abi.py with AddressSanitizer +
// UBSan.  It builds trees with bvh_builder.cpp on check_bvh's inputs, runs the walk the kernel runs - sb_walk with the same per-node
// bound, order, stack discipline and leaf test (early returns included) - with a host-side stack whose index is checked against what
// the kernel's launch provides, and compares every answer's bytes with a brute force over all records and spheres by the same rules,
// without a limit on the time.  A bound that culls a box holding the winner, an early return that changes an answer, a visiting order
// that loses a tie, or a stack that outgrows its entries shows here, before any kernel runs.
// usage: check_sweep_box <n_triangles> <seed> <kind> [method]   as check_bvh: method 0 binned SAH (default), 1 PLOC; kind 0 soup,
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
#include "sweep_box_rules.h"

using namespace rt;

namespace {

int g_fail = 0;

struct Sphere {
    float centre[3], radius;
    uint32_t material;
};

void answer(const BvhBuild& b, const std::vector<Sphere>& spheres, const CpBest& best, const SbQuery& q, uint32_t out[8]) {
    sb_answer_miss(q.tmax, out);
    if (best.slot == 0xFFFFFFFFu) return;
    if ((uint32_t)best.order & RT_PRIM_SPHERE_FLAG) {
        const DevTri& t = b.tris[best.slot];
        float rec[9];
        for (int a = 0; a < 3; a++) rec[a] = t.v0[a], rec[3 + a] = t.e1[a], rec[6 + a] = t.e2[a];
        sb_answer_triangle(rec, t.material_id, best.order, q, out);
    } else {
        const Sphere& s = spheres[best.slot];
        sb_answer_sphere(s.centre, s.radius, s.material, best.order, q, out);
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

    // sweeps: toward a point of a surface, grazing past a surface with a face at a distance of -+ a little, starting in contact, from
    // far outside, with coordinates around 1e4, along an axis (zero direction components), zero half extents, inside and toward the
    // spheres
    struct Sweep {
        float c[3], h[3], d[3], tmax;
    };
    std::vector<Sweep> qs;
    const float inf = std::numeric_limits<float>::infinity();
    const size_t n_each = 96;
    auto aim = [&](Sweep& s, const float from[3], const float to[3], float speed) {
        for (int a = 0; a < 3; a++) s.c[a] = from[a], s.d[a] = (to[a] - from[a]) * speed;
    };
    auto extents = [&](Sweep& s, float lo, float hi, size_t k) {
        for (int a = 0; a < 3; a++) s.h[a] = lo + (hi - lo) * 0.5f * (u(rng) + 1.0f);
        if (k % 8 == 7) s.h[k % 3] = 0.0f; // a moving slab
    };
    for (size_t k = 0; k < n_each && !recs.empty(); k++) {
        const DevTri& t = b.tris[recs[rng() % recs.size()]];
        const float bu = 0.5f * (u(rng) + 1.0f) * 0.5f, bv = 0.5f * (u(rng) + 1.0f) * 0.5f;
        float surf[3], from[3], off[3];
        for (int a = 0; a < 3; a++) {
            surf[a] = k % 4 == 0 ? t.v0[a] : k % 4 == 1 ? t.v0[a] + t.e1[a] * bu : t.v0[a] + (t.e1[a] * bu + t.e2[a] * bv); // vertex, edge, face
            off[a] = u(rng);
            from[a] = surf[a] + off[a] * (k % 2 ? 1.5f : 8.0f);
        }
        Sweep toward, graze, touch;
        extents(toward, 0.01f, 0.3f, k);
        toward.tmax = k % 5 == 4 ? 0.5f : inf; // some end before the contact
        aim(toward, from, surf, 0.2f + 2.4f * (u(rng) + 1.0f));
        // past the point along an axis, with the box's face on another axis at the point's coordinate -+ 0.1 %
        extents(graze, 0.05f, 0.25f, k + 1);
        const int along = (int)(k % 3), across = (int)((k + 1) % 3);
        float pass[3];
        for (int a = 0; a < 3; a++) pass[a] = surf[a], from[a] = surf[a];
        pass[across] = from[across] = surf[across] + (graze.h[across] + 1e-6f) * (k % 2 ? 1.001f : 0.999f);
        from[along] -= 3.0f;
        graze.tmax = inf;
        aim(graze, from, pass, 0.7f);
        // in contact at the start: the point inside the box
        extents(touch, 0.15f, 0.25f, k + 2);
        for (int a = 0; a < 3; a++) from[a] = surf[a] + off[a] * 0.1f;
        touch.tmax = k % 3 == 0 ? 1e-30f : inf;
        aim(touch, from, surf, 1.0f);
        touch.d[k % 3] = 0.0f; // and a zero direction component
        qs.push_back(toward), qs.push_back(graze), qs.push_back(touch);
    }
    for (size_t k = 0; k < n_each; k++) {
        Sweep scat, far, big;
        float to[3], from[3];
        for (int a = 0; a < 3; a++) to[a] = u(rng) * 10.0f, from[a] = u(rng) * 30.0f;
        extents(scat, k % 2 ? 0.1f : 1e-3f, k % 2 ? 0.3f : 2e-3f, k);
        scat.tmax = k % 4 == 3 ? 0.9f : inf;
        aim(scat, from, to, 1.0f);
        if (k % 8 == 0) scat.d[0] = 0.0f, scat.d[1] = -0.0f; // along z
        if (k % 16 == 1) scat.h[0] = scat.h[1] = scat.h[2] = 0.0f; // a moving point: a ray
        for (int a = 0; a < 3; a++) from[a] = u(rng) * 3000.0f;
        extents(far, 0.2f, 0.5f, k + 3);
        far.tmax = inf;
        aim(far, from, to, 1e-3f);
        for (int a = 0; a < 3; a++) from[a] = 1e4f + u(rng) * 50.0f;
        extents(big, k % 2 ? 1.0f : 0.02f, k % 2 ? 2.0f : 0.05f, k + 5);
        big.tmax = k % 2 ? inf : 2.0f;
        aim(big, from, to, 1.0f);
        qs.push_back(scat), qs.push_back(far), qs.push_back(big);
    }
    const float hb[3] = {0.1f, 0.05f, 0.2f};
    auto add = [&](float cx, float cy, float cz, float dx, float dy, float dz, float tmax) { qs.push_back({{cx, cy, cz}, {hb[0], hb[1], hb[2]}, {dx, dy, dz}, tmax}); };
    add(2.0f, 1.0f, -1.0f, 0.3f, 0.2f, -0.1f, inf);  // from a sphere's centre outward (two coincident spheres: the lower index)
    add(2.1f, 1.2f, -0.9f, 0.0f, 1.0f, 0.0f, inf);   // inside it
    add(2.1f, 1.2f, -0.9f, 0.0f, 1.0f, 0.0f, 1e-3f); // ... and too far for this tmax
    add(2.0f, 1.7f, -1.0f, 1.0f, 0.0f, 0.0f, inf);   // in contact with it from inside
    add(9.0f, 0.5f, 3.0f, -2.0f, 0.0f, 0.0f, inf);   // toward the other from outside: a face piece
    add(9.0f, 2.1f, 3.0f, -2.0f, 0.0f, 0.0f, inf);   // ... an edge piece
    add(9.0f, 2.0f, 4.6f, -2.0f, 0.0f, 0.0f, inf);   // ... a corner piece
    add(9.0f, 2.0f, 4.6f, -2.0f, -0.3f, 0.1f, inf);

    HostAccess acc;
    acc.init(b);
    size_t found = 0, at_start = 0, by_axis[15] = {0};
    for (size_t k = 0; k < qs.size(); k++) {
        const SbQuery q = sb_query(qs[k].c, qs[k].h, qs[k].d, qs[k].tmax);
        uint32_t got[8], want[8];
        CpBest walk{sw_start(q.tmax), 0xFFFFFFFFu}, brute = walk;
        if (sb_query_valid(q)) {
            for (uint32_t s = 0; s < spheres.size(); s++) {
                const uint64_t c = cp_order(sb_sphere(spheres[s].centre, spheres[s].radius, q), s);
                if (c < walk.order) walk.order = c, walk.slot = s;
            }
            brute = walk;
            sb_walk(acc, (uint32_t)b.nodes.size(), q, walk);
            for (uint32_t r : recs) {
                const DevTri& t = b.tris[r];
                uint32_t axis;
                float w_in;
                const uint64_t c = cp_order(sb_triangle(t.v0, t.e1, t.e2, q, INFINITY, axis, w_in), t.prim_id ^ RT_PRIM_SPHERE_FLAG);
                if (c < brute.order) brute.order = c, brute.slot = r;
            }
        }
        answer(b, spheres, walk, q, got);
        answer(b, spheres, brute, q, want);
        found += want[6] != RT_PRIM_MISS;
        at_start += want[6] != RT_PRIM_MISS && want[3] == 0u;
        if (want[6] != RT_PRIM_MISS) by_axis[want[4] < 14u ? want[4] : 14u]++;
        if (std::memcmp(got, want, sizeof got) != 0) {
            if (g_fail < 20)
                std::printf("FAIL: sweep %zu (%.9g %.9g %.9g h %.9g %.9g %.9g, d %.9g %.9g %.9g, tmax %.9g): walk prim %08x t %.9g axis %u, brute force prim %08x t %.9g axis %u\n",
                            k, q.c[0], q.c[1], q.c[2], q.h[0], q.h[1], q.h[2], q.d[0], q.d[1], q.d[2], q.tmax, got[6], cp_float(got[3]), got[4], want[6],
                            cp_float(want[3]), want[4]);
            g_fail++;
        }
    }
    std::printf("axes 0..12, sphere, none:");
    for (size_t a = 0; a < 15; a++) std::printf(" %zu", by_axis[a]);
    std::printf("\nkind %d n %zu method %d: %zu nodes depth %u, %zu sweeps (%zu hit, %zu of them at the start), %.1f node visits and %.1f triangle tests per "
                "sweep (brute force %zu), stack %d of %zu, %d failures\n",
                kind, n, opt.method, b.nodes.size(), b.depth, qs.size(), found, at_start, (double)acc.nodes / (double)qs.size(),
                (double)acc.tris / (double)qs.size(), recs.size(), acc.max_sp, acc.stack.size(), g_fail);
    return g_fail ? 1 : 0;
}
