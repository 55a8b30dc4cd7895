// Host check of the oriented-box queries (gpu_raytracer_amd/csrc/obb_rules.h), built by tests/test_obb_abi.py with AddressSanitizer +
// UBSan.  It builds trees with bvh_builder.cpp on check_bvh's inputs and runs the two walks the kernels run - ob_sweep_walk and
// ob_walk, with the world bounding box's node tests, the frame's leaf tests and their early returns - with a host-side stack whose
// index is checked against what the kernels' launches provide, and compares every answer's bytes, and every list and count, with a
// brute force over all records and spheres by the same rules.  A world bound that culls a node holding a primitive the turned box
// touches shows here, before any kernel runs.  It also holds, pair by pair, the sweep's (t = 0, NONE) to the overlap's statement for
// the start pose, and the answers at the exact identity to sweep_box_rules.h's and overlap_rules.h's.
// usage: check_obb <n_triangles> <seed> <kind> [method]   as check_bvh: method 0 binned SAH (default), 1 PLOC; kind 0 soup,
//                    1 coplanar grid, 2 coincident points, 3 collinear chain, 4 huge + tiny mixed, 5 with NaN / inf vertices
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
#include "obb_rules.h"

using namespace rt;

namespace {

int g_fail = 0;
const uint32_t K_MAX = 32u; // RT_OVERLAP_MAX

struct Sphere {
    float centre[3], radius;
    uint32_t material;
};

struct Sweep {
    float c[3], h[3], q[4], d[3], tmax;
};

void record(const DevTri& t, float rec[9]) {
    for (int a = 0; a < 3; a++) rec[a] = t.v0[a], rec[3 + a] = t.e1[a], rec[6 + a] = t.e2[a];
}

void answer(const BvhBuild& b, const std::vector<Sphere>& spheres, const CpBest& best, const ObSweep& s, float tmax, uint32_t out[8]) {
    sb_answer_miss(tmax, out);
    if (best.slot == 0xFFFFFFFFu) return;
    if ((uint32_t)best.order & RT_PRIM_SPHERE_FLAG) {
        float rec[9];
        record(b.tris[best.slot], rec);
        ob_answer_triangle(rec, b.tris[best.slot].material_id, best.order, s, out);
    } else {
        const Sphere& sp = spheres[best.slot];
        ob_answer_sphere(sp.centre, sp.radius, sp.material, best.order, s, out);
    }
}

// what k_sweep_box answers: the identity's yardstick
void aligned_answer(const BvhBuild& b, const std::vector<Sphere>& spheres, const std::vector<uint32_t>& recs, const Sweep& w, uint32_t out[8]) {
    const SbQuery q = sb_query(w.c, w.h, w.d, w.tmax);
    sb_answer_miss(q.tmax, out);
    if (!sb_query_valid(q)) return;
    CpBest best{sw_start(q.tmax), 0xFFFFFFFFu};
    for (uint32_t s = 0; s < spheres.size(); s++) {
        const uint64_t c = cp_order(sb_sphere(spheres[s].centre, spheres[s].radius, q), s);
        if (c < best.order) best.order = c, best.slot = s;
    }
    for (uint32_t r : recs) {
        const DevTri& t = b.tris[r];
        uint32_t axis;
        float w_in;
        const uint64_t c = cp_order(sb_triangle(t.v0, t.e1, t.e2, q, INFINITY, axis, w_in), t.prim_id ^ RT_PRIM_SPHERE_FLAG);
        if (c < best.order) best.order = c, best.slot = r;
    }
    if (best.slot == 0xFFFFFFFFu) return;
    if ((uint32_t)best.order & RT_PRIM_SPHERE_FLAG) {
        float rec[9];
        record(b.tris[best.slot], rec);
        sb_answer_triangle(rec, b.tris[best.slot].material_id, best.order, q, out);
    } else {
        const Sphere& sp = spheres[best.slot];
        sb_answer_sphere(sp.centre, sp.radius, sp.material, best.order, q, out);
    }
}

// what k_overlap_obb does for one lane: K ids and the count
template <int MODE>
uint32_t overlap_lane(HostKeyAccess& acc, const std::vector<Sphere>& spheres, const Sweep& q, uint32_t K, uint32_t* out) {
    acc.list.assign((size_t)K, 0xDEADBEEFu);
    OvList list;
    ov_list_init(list, MODE == OV_ANY ? 0u : K);
    ObBox box;
    if (ob_query_valid(q.c, q.h, q.q, box.R)) {
        ob_box_init(box, q.c, q.h);
        for (uint32_t s = 0; s < spheres.size(); s++) {
            if (MODE == OV_ANY && list.total) break;
            if (ov_list_wants<MODE>(list, s) && ob_sphere(spheres[s].centre, spheres[s].radius, box)) ov_list_offer(acc, list, s);
        }
        if (MODE != OV_ANY || list.total == 0u) ob_walk<MODE>(acc, (uint32_t)acc.b->nodes.size(), box, list);
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
    std::normal_distribution<float> gauss(0.0f, 1.0f);
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

    // check_sweep_box's sweeps - toward a point of a surface, grazing, starting in contact, scattered, from far outside, around 1e4,
    // along an axis, zero half extents, at the spheres - each with a rotation by index: uniform, of any length; the exact identity,
    // also as (0, 0, 0, -3) and (-0, 0, -0, -3); within 1e-3 rad of it; a quarter turn; a long thin box turned 45 degrees about an axis
    std::vector<Sweep> qs;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const size_t n_each = 96;
    size_t n_rot = 0;
    auto turn = [&](Sweep& s) {
        const size_t k = n_rot++;
        float q[4] = {gauss(rng), gauss(rng), gauss(rng), gauss(rng)};
        const float len = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), scale = (0.5f + 0.75f * (u(rng) + 1.0f)) / (len > 0.0f ? len : 1.0f);
        for (float& x : q) x *= scale;
        if (k % 8 == 1) q[0] = q[1] = q[2] = 0.0f, q[3] = k % 16 == 1 ? 1.0f : -3.0f;
        if (k % 32 == 9) q[0] = q[2] = -0.0f; // R's off-diagonal zeros are then not all +0
        if (k % 8 == 2) q[0] = u(rng) * 4e-4f, q[1] = u(rng) * 4e-4f, q[2] = u(rng) * 4e-4f, q[3] = 1.0f;
        if (k % 8 == 3) q[0] = q[1] = 0.0f, q[2] = q[3] = std::sqrt(0.5f);
        if (k % 8 == 4) { // long and thin, turned 45 degrees: the world bound is at its loosest
            const int along = (int)(k % 3), about = (int)((k + 1) % 3);
            s.h[along] *= 8.0f;
            q[0] = q[1] = q[2] = 0.0f, q[about] = std::sin(0.39269908f), q[3] = std::cos(0.39269908f);
        }
        for (int a = 0; a < 4; a++) s.q[a] = q[a];
    };
    auto aim = [&](Sweep& s, const float from[3], const float to[3], float speed) {
        for (int a = 0; a < 3; a++) s.c[a] = from[a], s.d[a] = (to[a] - from[a]) * speed;
    };
    auto extents = [&](Sweep& s, float lo, float hi, size_t k) {
        for (int a = 0; a < 3; a++) s.h[a] = lo + (hi - lo) * 0.5f * (u(rng) + 1.0f);
        if (k % 8 == 7) s.h[k % 3] = 0.0f; // a moving slab
        turn(s);
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
        // past the point along an axis, a little more or less than the box's reach on another axis away from it
        extents(graze, 0.05f, 0.25f, k + 1);
        const int along = (int)(k % 3), across = (int)((k + 1) % 3);
        float pass[3];
        for (int a = 0; a < 3; a++) pass[a] = surf[a], from[a] = surf[a];
        pass[across] = from[across] = surf[across] + (graze.h[across] + 1e-6f) * (k % 2 ? 1.001f : 0.999f);
        from[along] -= 3.0f;
        graze.tmax = inf;
        aim(graze, from, pass, 0.7f);
        // in contact at the start: the point inside the box, or near it
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
    auto add = [&](float cx, float cy, float cz, float dx, float dy, float dz, float tmax) {
        Sweep s{{cx, cy, cz}, {hb[0], hb[1], hb[2]}, {0.0f, 0.0f, 0.0f, 1.0f}, {dx, dy, dz}, tmax};
        turn(s);
        qs.push_back(s);
    };
    for (int rep = 0; rep < 4; rep++) {
        add(2.0f, 1.0f, -1.0f, 0.3f, 0.2f, -0.1f, inf);  // from a sphere's centre outward (two coincident spheres: the lower index)
        add(2.1f, 1.2f, -0.9f, 0.0f, 1.0f, 0.0f, inf);   // inside it
        add(2.1f, 1.2f, -0.9f, 0.0f, 1.0f, 0.0f, 1e-3f); // ... and too far for this tmax
        add(2.0f, 1.7f, -1.0f, 1.0f, 0.0f, 0.0f, inf);   // in contact with it from inside
        add(9.0f, 0.5f, 3.0f, -2.0f, 0.0f, 0.0f, inf);   // toward the other from outside
        add(9.0f, 2.1f, 3.0f, -2.0f, 0.0f, 0.0f, inf);
        add(9.0f, 2.0f, 4.6f, -2.0f, 0.0f, 0.0f, inf);
        add(9.0f, 2.0f, 4.6f, -2.0f, -0.3f, 0.1f, inf);
    }
    const size_t n_ordinary = qs.size();
    // degenerate rotations: no walk
    const float bad[6][4] = {{nan, 0.0f, 0.0f, 1.0f}, {0.0f, inf, 0.0f, 1.0f}, {0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 2e19f, 2e19f}, {0.0f, 1e-30f, 0.0f, 1e-30f},
                             {0.0f, 0.0f, 0.0f, -inf}};
    for (const float* q : bad) qs.push_back({{0.5f, 0.5f, 0.5f}, {0.3f, 0.3f, 0.3f}, {q[0], q[1], q[2], q[3]}, {1.0f, 0.5f, 0.25f}, inf});
    qs.push_back({{0.5f, 0.5f, 0.5f}, {0.3f, 0.3f, 0.3f}, {0.0f, 0.0f, 1e-10f, 1e-10f}, {1.0f, 0.5f, 0.25f}, inf}); // tiny but valid: it walks

    HostAccess acc;
    HostKeyAccess list_acc, any_acc;
    acc.init(b), list_acc.init(b), any_acc.init(b);
    size_t found = 0, at_start = 0, by_axis[15] = {0}, identities = 0, touched = 0, listed = 0;
    int sweep_fails = 0, overlap_fails = 0, start_fails = 0, identity_fails = 0;
    std::vector<uint32_t> keys;
    for (size_t k = 0; k < qs.size(); k++) {
        const Sweep& w = qs[k];
        ObSweep s;
        const bool ok = ob_sweep_init(s, w.c, w.h, w.q, w.d, w.tmax);
        float R[9];
        const bool box_ok = ob_query_valid(w.c, w.h, w.q, R);
        if (k < n_ordinary ? !box_ok : (box_ok != (k + 1 == qs.size()))) {
            std::printf("FAIL: query %zu: validity %d\n", k, (int)box_ok);
            g_fail++;
        }
        // ---- the sweep
        uint32_t got[8], want[8];
        CpBest walk{sw_start(w.tmax), 0xFFFFFFFFu}, brute = walk;
        const unsigned long long n0 = acc.nodes;
        keys.clear();
        if (ok) {
            for (uint32_t i = 0; i < spheres.size(); i++) {
                const uint64_t c = cp_order(ob_sweep_sphere(spheres[i].centre, spheres[i].radius, s), i);
                if (c < walk.order) walk.order = c, walk.slot = i;
            }
            brute = walk;
            ob_sweep_walk(acc, (uint32_t)b.nodes.size(), s, walk);
        }
        ObBox box;
        if (box_ok) {
            (void)ob_query_valid(w.c, w.h, w.q, box.R);
            ob_box_init(box, w.c, w.h);
            for (uint32_t i = 0; i < spheres.size(); i++)
                if (ob_sphere(spheres[i].centre, spheres[i].radius, box)) keys.push_back(i);
        }
        for (uint32_t r : recs) {
            float rec[9];
            record(b.tris[r], rec);
            const bool touches = box_ok && ob_triangle(rec, box);
            if (touches) keys.push_back(b.tris[r].prim_id ^ RT_PRIM_SPHERE_FLAG);
            if (!ok) continue;
            uint32_t axis;
            float w_in;
            ObTriangle t;
            const float time = ob_sweep_triangle(rec, s, INFINITY, axis, w_in, t);
            if ((time == 0.0f && axis == SB_AXIS_NONE) != touches) { // consequence (b), pair by pair
                if (start_fails < 5) std::printf("FAIL: query %zu record %u: sweep t %.9g axis %u, overlap %d\n", k, r, time, axis, (int)touches);
                start_fails++, g_fail++;
            }
            const uint64_t c = cp_order(time, b.tris[r].prim_id ^ RT_PRIM_SPHERE_FLAG);
            if (c < brute.order) brute.order = c, brute.slot = r;
        }
        if (!ok && acc.nodes != n0) std::printf("FAIL: query %zu is degenerate and walked\n", k), g_fail++;
        answer(b, spheres, walk, s, w.tmax, got);
        answer(b, spheres, brute, s, w.tmax, want);
        found += want[6] != RT_PRIM_MISS;
        at_start += want[6] != RT_PRIM_MISS && want[3] == 0u;
        if (want[6] != RT_PRIM_MISS) by_axis[want[4] < 14u ? want[4] : 14u]++;
        if (std::memcmp(got, want, sizeof got) != 0) {
            if (sweep_fails < 20)
                std::printf("FAIL: sweep %zu (%.9g %.9g %.9g h %.9g %.9g %.9g q %.9g %.9g %.9g %.9g d %.9g %.9g %.9g tmax %.9g): walk prim %08x t %.9g axis %u, brute "
                            "force prim %08x t %.9g axis %u\n",
                            k, w.c[0], w.c[1], w.c[2], w.h[0], w.h[1], w.h[2], w.q[0], w.q[1], w.q[2], w.q[3], w.d[0], w.d[1], w.d[2], w.tmax, got[6],
                            cp_float(got[3]), got[4], want[6], cp_float(want[3]), want[4]);
            sweep_fails++, g_fail++;
        }
        // ---- the exact identity: the axis-aligned statements' bytes (consequence (a); a sphere normal's -0 would show here)
        if (ok && w.q[0] == 0.0f && w.q[1] == 0.0f && w.q[2] == 0.0f) {
            uint32_t aligned[8];
            aligned_answer(b, spheres, recs, w, aligned);
            identities++;
            bool same = std::memcmp(aligned, want, sizeof want) == 0;
            for (uint32_t r : recs) {
                float rec[9];
                record(b.tris[r], rec);
                same = same && ov_triangle(b.tris[r].v0, b.tris[r].e1, b.tris[r].e2, w.c, w.h) == ob_triangle(rec, box);
            }
            if (!same) {
                if (identity_fails < 5) std::printf("FAIL: query %zu at the identity differs from the axis-aligned statement (t %.9g against %.9g)\n", k, cp_float(want[3]), cp_float(aligned[3]));
                identity_fails++, g_fail++;
            }
        }
        // ---- the overlap of the start pose: the list at K = 32 with COUNT_ALL, and ANY
        std::sort(keys.begin(), keys.end());
        const uint32_t total = (uint32_t)keys.size(), written = total < K_MAX ? total : K_MAX;
        uint32_t ids[K_MAX], want_ids[K_MAX], none[1];
        const unsigned long long l0 = list_acc.nodes, a0 = any_acc.nodes;
        const uint32_t count = overlap_lane<OV_COUNT_ALL>(list_acc, spheres, w, K_MAX, ids);
        const uint32_t any = overlap_lane<OV_ANY>(any_acc, spheres, w, 0u, none);
        for (uint32_t j = 0; j < K_MAX; j++) want_ids[j] = j < written ? (keys[j] ^ RT_PRIM_SPHERE_FLAG) : RT_PRIM_MISS;
        touched += total > 0, listed += written;
        if (std::memcmp(ids, want_ids, sizeof ids) != 0 || count != total || any != (total ? 1u : 0u) ||
            (!box_ok && (list_acc.nodes != l0 || any_acc.nodes != a0))) {
            if (overlap_fails < 20) std::printf("FAIL: box %zu: count %u any %u, brute force %u; first id %08x against %08x\n", k, count, any, total, ids[0], want_ids[0]);
            overlap_fails++, g_fail++;
        }
    }
    std::printf("axes 0..12, sphere, none:");
    for (size_t a = 0; a < 15; a++) std::printf(" %zu", by_axis[a]);
    const double nq = (double)qs.size();
    std::printf("\noverlap: %d failed, %.1f node visits and %.1f triangle tests per box (COUNT_ALL), stack %d of %zu, %zu boxes touched, %zu ids listed\n",
                overlap_fails, (double)list_acc.nodes / nq, (double)list_acc.tris / nq, list_acc.max_sp, list_acc.stack.size(), touched, listed);
    std::printf("start in contact: %d pairs differ; identity: %d of %zu differ\n", start_fails, identity_fails, identities);
    std::printf("kind %d n %zu method %d: %zu nodes depth %u, %zu sweeps (%zu hit, %zu of them at the start), %.1f node visits and %.1f triangle tests per "
                "sweep (brute force %zu), stack %d of %zu, %d failures\n",
                kind, n, opt.method, b.nodes.size(), b.depth, qs.size(), found, at_start, (double)acc.nodes / nq, (double)acc.tris / nq, recs.size(),
                acc.max_sp, acc.stack.size(), g_fail);
    return g_fail ? 1 : 0;
}
