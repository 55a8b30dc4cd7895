// Host check of the capsule sweep (gpu_raytracer_amd/csrc/sweep_capsule_rules.h), built by tests/test_sweep_capsule_abi.py with
// AddressSanitizer + UBSan.  It builds trees with bvh_builder.cpp on check_bvh's inputs, runs the walk the kernel runs - sc_walk with
// the same per-node bound, order, stack discipline and leaf test - with a host-side stack whose index is checked against what the
// kernel's launch provides, and compares every answer's bytes with a brute force over all records and spheres by the same rules.  A
// bound that culls a box holding the winner, a visiting order that loses a tie, or a stack that outgrows its entries shows here,
// before any kernel runs.  It also says which of the four piece groups, or the start rule, decided each triangle contact.
// usage: check_sweep_capsule <n_triangles> <seed> <kind> [method]   as check_bvh: method 0 binned SAH (default), 1 PLOC; kind 0 soup,
//                    1 coplanar grid, 2 coincident points, 3 collinear chain, 4 huge + tiny mixed, 5 with NaN / inf vertices
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <limits>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "bvh_builder.h"
#include "host_access.h"
#include "sweep_capsule_rules.h"

using namespace rt;

namespace {

int g_fail = 0;

struct Sphere {
    float centre[3], radius;
    uint32_t material;
};

void answer(const BvhBuild& b, const std::vector<Sphere>& spheres, const CpBest& best, const ScQuery& q, uint32_t out[8]) {
    sc_answer_miss(q.s.tmax, out);
    if (best.slot == 0xFFFFFFFFu) return;
    if ((uint32_t)best.order & RT_PRIM_SPHERE_FLAG) {
        const DevTri& t = b.tris[best.slot];
        float rec[9];
        for (int a = 0; a < 3; a++) rec[a] = t.v0[a], rec[3 + a] = t.e1[a], rec[6 + a] = t.e2[a];
        sc_answer_triangle(rec, t.material_id, best.order, q, out);
    } else {
        const Sphere& s = spheres[best.slot];
        sc_answer_sphere(s.centre, s.radius, s.material, best.order, q, out);
    }
}

// which rule decided the winner's time: 0..3 the first piece group that gives it, 4 the start rule
int decided_by(const DevTri& t, const ScQuery& q) {
    float s, v, w, g[4];
    if (cap_triangle(t.v0, t.e1, t.e2, q.s.c, q.ax, q.aa, s, v, w) <= q.s.rr) return 4;
    sc_pieces(t.v0, t.e1, t.e2, q, g);
    int k = 0;
    for (int i = 1; i < 4; i++)
        if (g[i] < g[k]) k = i;
    return k;
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

    // sweeps: the body toward a point of a surface (vertex, edge, face) with an axis that is zero, parallel to an edge of that
    // triangle, in its plane, upright or diagonal; grazing past the point at r (1 -+ 1e-3) from the axis; starting in contact, some of
    // them with the axis through the triangle; scattered; from far outside; with coordinates around 1e4; along a coordinate axis;
    // inside and toward the spheres
    struct Sweep {
        float A[3], r, ax[3], d[3], tmax;
    };
    std::vector<Sweep> qs;
    const float inf = std::numeric_limits<float>::infinity();
    const size_t n_each = 96;
    auto place = [&](Sweep& s, const float mid[3], const float to[3], float speed, float where) { // the axis point at `where` starts at mid
        for (int a = 0; a < 3; a++) s.A[a] = mid[a] - s.ax[a] * where, s.d[a] = (to[a] - mid[a]) * speed;
    };
    auto axis_of = [&](Sweep& s, const DevTri* t, size_t k, float len) {
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
        for (int a = 0; a < 3; a++) s.ax[a] = kind5 == 0 || !(l > 0.0f) || !std::isfinite(l) ? 0.0f : x[a] / l * len;
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
        toward.r = 0.01f + 0.15f * (u(rng) + 1.0f);
        axis_of(toward, &t, k, 0.05f + 0.4f * (u(rng) + 1.0f));
        toward.tmax = k % 5 == 4 ? 0.5f : inf; // some end before the contact
        place(toward, from, surf, 0.2f + 2.4f * (u(rng) + 1.0f), 0.5f * (u(rng) + 1.0f));
        // past the point, a point of the axis at r (1 -+ 1e-3) from it, moving across the offset
        graze.r = 0.05f + 0.1f * (u(rng) + 1.0f);
        axis_of(graze, &t, k + 1, 0.3f);
        const bool has_axis = graze.ax[0] != 0.0f || graze.ax[1] != 0.0f || graze.ax[2] != 0.0f;
        const float other[3] = {has_axis ? graze.ax[0] : off[1], has_axis ? graze.ax[1] : off[2] + 2.0f, has_axis ? graze.ax[2] : off[0]};
        float side[3], pass[3];
        sw_cross(off, other, side); // across the offset and the axis
        const float sl = std::sqrt(side[0] * side[0] + side[1] * side[1] + side[2] * side[2]) + 1e-20f;
        for (int a = 0; a < 3; a++) side[a] /= sl;
        float ol = std::sqrt(off[0] * off[0] + off[1] * off[1] + off[2] * off[2]) + 1e-20f;
        for (int a = 0; a < 3; a++) pass[a] = surf[a] + off[a] / ol * graze.r * (k % 2 ? 1.001f : 0.999f), from[a] = pass[a] - side[a] * 3.0f;
        graze.tmax = inf;
        place(graze, from, pass, 0.7f, 0.5f * (u(rng) + 1.0f));
        // in contact at the start; every third with the axis through the triangle's interior and both ends farther than r
        touch.r = k % 3 == 2 ? 0.02f : 0.15f + 0.05f * (u(rng) + 1.0f);
        axis_of(touch, &t, k + 2, 0.4f);
        for (int a = 0; a < 3; a++) from[a] = surf[a] + off[a] * 0.1f;
        if (k % 3 == 2) {
            float nrm[3];
            sw_cross(t.e1, t.e2, nrm);
            const float nl = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
            for (int a = 0; a < 3; a++) {
                touch.ax[a] = nl > 0.0f && std::isfinite(nl) ? nrm[a] / nl * 0.3f + off[a] * 0.03f : 0.0f;
                from[a] = t.v0[a] + (t.e1[a] * 0.3f + t.e2[a] * 0.3f);
            }
        }
        touch.tmax = k % 3 == 0 ? 1e-30f : inf;
        place(touch, from, surf, 1.0f, k % 3 == 2 ? 0.5f : 0.5f * (u(rng) + 1.0f));
        touch.d[k % 3] = k % 3 == 2 ? 0.7f : 0.0f; // a zero direction component, but never a zero direction
        qs.push_back(toward), qs.push_back(graze), qs.push_back(touch);
    }
    for (size_t k = 0; k < n_each; k++) {
        Sweep scat, far, big;
        float to[3], from[3];
        for (int a = 0; a < 3; a++) to[a] = u(rng) * 10.0f, from[a] = u(rng) * 30.0f;
        scat.r = k % 2 ? 0.1f + 0.1f * (u(rng) + 1.0f) : 1e-3f;
        axis_of(scat, nullptr, k, k % 2 ? 0.6f : 2.0f);
        scat.tmax = k % 4 == 3 ? 0.9f : inf;
        place(scat, from, to, 1.0f, 0.0f);
        if (k % 8 == 0) scat.d[0] = 0.0f, scat.d[1] = -0.0f; // along z
        for (int a = 0; a < 3; a++) from[a] = u(rng) * 3000.0f;
        far.r = 0.2f + 0.15f * (u(rng) + 1.0f);
        axis_of(far, nullptr, k + 1, 1.0f);
        far.tmax = inf;
        place(far, from, to, 1e-3f, 0.5f);
        for (int a = 0; a < 3; a++) from[a] = 1e4f + u(rng) * 50.0f;
        big.r = k % 2 ? 1.0f : 0.02f;
        axis_of(big, nullptr, k + 2, k % 2 ? 3.0f : 0.1f);
        big.tmax = k % 2 ? inf : 2.0f;
        place(big, from, to, 1.0f, 0.5f);
        qs.push_back(scat), qs.push_back(far), qs.push_back(big);
    }
    auto add = [&](float x, float y, float z, float ax, float ay, float az, float dx, float dy, float dz, float tmax) {
        qs.push_back({{x, y, z}, 0.1f, {ax, ay, az}, {dx, dy, dz}, tmax});
    };
    add(2.0f, 1.0f, -1.0f, 0.0f, 0.2f, 0.0f, 0.3f, 0.2f, -0.1f, inf);  // from a sphere's centre outward (two coincident spheres: the lower index)
    add(2.1f, 1.2f, -0.9f, 0.1f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, inf);   // inside it
    add(2.1f, 1.2f, -0.9f, 0.1f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 1e-3f); // ... and too far for this tmax
    add(2.0f, 1.7f, -1.0f, 0.0f, -0.3f, 0.0f, 1.0f, 0.0f, 0.0f, inf);  // in contact with it from inside
    add(1.0f, 1.0f, -1.0f, 2.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, inf);   // the axis through it, both ends outside: in contact
    add(9.0f, 0.5f, 3.0f, 0.0f, 0.0f, 0.0f, -2.0f, 0.0f, 0.0f, inf);   // toward the other from outside: a zero axis
    add(9.0f, 0.0f, 3.0f, 0.0f, 1.0f, 0.0f, -2.0f, 0.0f, 0.0f, inf);   // ... the cylinder wall
    add(9.0f, 2.2f, 3.0f, 0.0f, 1.0f, 0.0f, -2.0f, 0.0f, 0.0f, inf);   // ... end A
    add(9.0f, -2.2f, 3.0f, 0.3f, 1.0f, 0.2f, -2.0f, 0.0f, 0.0f, inf);  // ... end B
    add(9.0f, 2.0f, 4.6f, 0.5f, 0.5f, 0.5f, -2.0f, -0.3f, 0.1f, inf);

    // the sweeps are independent: a few threads take every T-th one, each with a stack and counters of its own
    struct Tally {
        HostAccess acc;
        size_t found = 0, at_start = 0, decided[5] = {0, 0, 0, 0, 0}, by_sphere = 0;
    };
    const unsigned n_threads = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<Tally> tally(n_threads);
    std::mutex print_lock;
    auto work = [&](unsigned me) {
        Tally& y = tally[me];
        y.acc.init(b);
        for (size_t k = me; k < qs.size(); k += n_threads) {
            const ScQuery q = sc_query(qs[k].A, qs[k].r, qs[k].ax, qs[k].d, qs[k].tmax);
            uint32_t got[8], want[8];
            CpBest walk{sw_start(q.s.tmax), 0xFFFFFFFFu}, brute = walk;
            if (sc_query_valid(q)) {
                for (uint32_t s = 0; s < spheres.size(); s++) {
                    const uint64_t c = cp_order(sc_sphere(spheres[s].centre, spheres[s].radius, q), s);
                    if (c < walk.order) walk.order = c, walk.slot = s;
                }
                brute = walk;
                sc_walk(y.acc, (uint32_t)b.nodes.size(), q, walk);
                for (uint32_t r : recs) {
                    const DevTri& t = b.tris[r];
                    const uint64_t c = cp_order(sc_triangle(t.v0, t.e1, t.e2, q), t.prim_id ^ RT_PRIM_SPHERE_FLAG);
                    if (c < brute.order) brute.order = c, brute.slot = r;
                }
            }
            answer(b, spheres, walk, q, got);
            answer(b, spheres, brute, q, want);
            y.found += want[6] != RT_PRIM_MISS;
            y.at_start += want[6] != RT_PRIM_MISS && want[3] == 0u;
            if (want[6] != RT_PRIM_MISS) {
                if (want[6] & RT_PRIM_SPHERE_FLAG) y.by_sphere++;
                else y.decided[decided_by(b.tris[brute.slot], q)]++;
            }
            if (std::memcmp(got, want, sizeof got) != 0) {
                std::lock_guard<std::mutex> hold(print_lock);
                if (g_fail < 20)
                    std::printf("FAIL: sweep %zu (%.9g %.9g %.9g r %.9g axis %.9g %.9g %.9g, d %.9g %.9g %.9g, tmax %.9g): walk prim %08x t %.9g s %.9g, brute force prim %08x t %.9g s %.9g\n",
                                k, q.s.c[0], q.s.c[1], q.s.c[2], q.s.r, q.ax[0], q.ax[1], q.ax[2], q.s.d[0], q.s.d[1], q.s.d[2], q.s.tmax, got[6], cp_float(got[3]),
                                cp_float(got[4]), want[6], cp_float(want[3]), cp_float(want[4]));
                g_fail++;
            }
        }
    };
    std::vector<std::thread> threads;
    for (unsigned me = 1; me < n_threads; me++) threads.emplace_back(work, me);
    work(0);
    for (std::thread& t : threads) t.join();
    HostAccess acc;
    acc.init(b);
    size_t found = 0, at_start = 0, decided[5] = {0}, by_sphere = 0;
    for (const Tally& y : tally) {
        acc.nodes += y.acc.nodes, acc.tris += y.acc.tris, acc.max_sp = std::max(acc.max_sp, y.acc.max_sp);
        found += y.found, at_start += y.at_start, by_sphere += y.by_sphere;
        for (int g = 0; g < 5; g++) decided[g] += y.decided[g];
    }
    std::printf("decided by end A, end B, wall x vertex, wall x edge, start, sphere: %zu %zu %zu %zu %zu %zu\n", decided[0], decided[1], decided[2], decided[3],
                decided[4], by_sphere);
    std::printf("kind %d n %zu method %d: %zu nodes depth %u, %zu sweeps (%zu hit, %zu of them at the start), %.1f node visits and %.1f triangle tests per "
                "sweep (brute force %zu), stack %d of %zu, %d failures\n",
                kind, n, opt.method, b.nodes.size(), b.depth, qs.size(), found, at_start, (double)acc.nodes / (double)qs.size(),
                (double)acc.tris / (double)qs.size(), recs.size(), acc.max_sp, acc.stack.size(), g_fail);
    return g_fail ? 1 : 0;
}
