// Host check of the posed-mesh queries (gpu_raytracer_amd/csrc/mesh_pose_rules.h), built by tests/test_posed_mesh_abi.py with
// AddressSanitizer + UBSan.  It builds trees with bvh_builder.cpp on check_bvh's inputs and answers poses of a small mesh the way a
// group of lanes of k_sweep_mesh does: lane g walks the posed triangles g, g + G, ... with its running order, every lane of a pose
// sharing one word.  The lanes of a pose run in a given order - forward, reverse, a seeded shuffle - two at a time, the two walks
// interleaved at node granularity (two threads that hand a baton over at every node visit), and the word is carried from pair to
// pair.  Every order, and the run without the word, must give the bytes of a brute force over all (mesh triangle, primitive) pairs;
// the node visits with the word must not exceed those without; and every stack index is checked against what the kernel's launch
// provides (tests/host_access.h).  The overlap answer (pairs, first) is held to its brute force the same way.
// usage: check_posed_mesh <n_triangles> <seed> <kind> [method]   as check_bvh: method 0 binned SAH (default), 1 PLOC; kind 0 soup,
//                    1 coplanar grid, 2 coincident points, 3 collinear chain, 4 huge + tiny mixed, 5 with NaN / inf vertices
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include "bvh_builder.h"
#include "host_access.h"
#include "mesh_pose_rules.h"

using namespace rt;

namespace {

int g_fail = 0;

struct Sphere {
    float centre[3], radius;
    uint32_t material;
};
struct MeshTri {
    float v[3][3];
};
struct PoseSweep {
    float position[3], rotation[4], d[3], tmax;
};

// two walks that take turns: yield() hands the baton to the other walk unless that one has finished
struct Baton {
    std::mutex mu;
    std::condition_variable cv;
    int turn = 0;
    bool done[2] = {false, false};
    void yield(int me) {
        std::unique_lock<std::mutex> lk(mu);
        if (done[1 - me]) return;
        turn = 1 - me;
        cv.notify_all();
        cv.wait(lk, [&] { return turn == me || done[1 - me]; });
    }
    void start(int me) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return turn == me || done[1 - me]; });
    }
    void finish(int me) {
        std::unique_lock<std::mutex> lk(mu);
        done[me] = true, turn = 1 - me;
        cv.notify_all();
    }
};
struct TurnAccess : HostAccess { // a node visit is where the neighbour's walk continues
    Baton* baton = nullptr;
    int me = 0;
    void node(uint32_t idx, uint32_t w[20]) {
        if (baton) baton->yield(me);
        HostAccess::node(idx, w);
    }
};
struct HostWord { // the pose's word; the baton's mutex orders the two walks' accesses
    uint32_t* p;
    uint32_t read() const { return *p; }
    void lower(uint32_t bits) {
        if (bits < *p) *p = bits;
    }
};

uint32_t group_of(uint32_t m) { // posed_mesh_group of posed_mesh.h
    uint32_t g = 1u;
    while (g < m && g < 64u) g <<= 1;
    return g;
}

void posed(const MeshTri& t, const MpPose& P, float q[3][3]) {
    for (int k = 0; k < 3; k++) mp_vertex(P, t.v[k], q[k]);
}

// what lane g of G runs for a pose: k_sweep_mesh's loop over its triangles
template <class Access, class Shared>
void lane_sweep(Access& acc, const BvhBuild& b, const std::vector<Sphere>& spheres, const std::vector<MeshTri>& mesh, const PoseSweep& s, const MpPose& P,
                uint32_t g, uint32_t G, Shared sh, MpBest& own) {
    mp_best_init(own, s.tmax);
    CpBest best{own.order, MP_NONE};
    for (uint32_t j = g; j < mesh.size(); j += G) {
        float q[3][3];
        posed(mesh[j], P, q);
        if (!st_query_valid(q[0], q[1], q[2], s.d, s.tmax)) continue;
        const StQuery sq = st_query(q[0], q[1], q[2], s.d, s.tmax);
        best.order = mp_tighten(best.order, sh.read());
        for (uint32_t i = 0; i < spheres.size(); i++)
            mp_sweep_sphere(cp_order(st_sphere(spheres[i].centre, spheres[i].radius, sq, q[1], q[2]), i), i, j, best, own, sh);
        mp_sweep_walk(acc, (uint32_t)b.nodes.size(), sq, j, best, own, sh);
    }
}

// rule 6 and the winner's record
void reduce(const BvhBuild& b, const std::vector<Sphere>& spheres, const std::vector<MeshTri>& mesh, const PoseSweep& s, const MpPose& P, bool valid,
            const std::vector<MpBest>& lanes, uint32_t out[8]) {
    mp_answer_miss(s.tmax, out);
    if (!valid) return;
    uint64_t least = ~0ull;
    for (const MpBest& o : lanes) least = std::min(least, mp_reduce_order(o));
    const MpBest* win = nullptr;
    for (const MpBest& o : lanes)
        if (o.j != MP_NONE && o.order == least && (!win || o.j < win->j)) win = &o;
    if (!win) return;
    float q[3][3];
    posed(mesh[win->j], P, q);
    const StQuery sq = st_query(q[0], q[1], q[2], s.d, s.tmax);
    if ((uint32_t)win->order & RT_PRIM_SPHERE_FLAG) {
        const DevTri& t = b.tris[win->slot];
        float rec[9];
        for (int a = 0; a < 3; a++) rec[a] = t.v0[a], rec[3 + a] = t.e1[a], rec[6 + a] = t.e2[a];
        st_answer_triangle(rec, t.material_id, win->order, sq, out);
    } else {
        const Sphere& sp = spheres[win->slot];
        st_answer_sphere(sp.centre, sp.radius, sp.material, win->order, sq, q[1], q[2], out);
    }
    out[5] = win->j;
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
    std::vector<uint32_t> recs; // the leaves' records: padding records are not triangles
    for (size_t first = 0; first + RT_DEV_LEAF_STRIDE <= b.tris.size(); first += RT_DEV_LEAF_STRIDE)
        for (uint32_t x = 0; x < b.tris[first].leaf_count && x < RT_DEV_LEAF_STRIDE; x++) recs.push_back((uint32_t)(first + x));

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    unsigned long long shared_nodes = 0, plain_nodes = 0;
    size_t n_poses = 0, found = 0, at_start = 0, tied = 0;
    int max_sp = 0;
    size_t stack_size = 0;
    for (const uint32_t m : {1u, 2u, 12u, 65u}) {
        // the mesh: triangles of edge ~0.3 around the origin; triangle 1 repeats triangle 0 (the lower index must win), and from 12
        // triangles on one has a NaN vertex (it meets nothing, the others still answer)
        std::vector<MeshTri> mesh(m);
        for (uint32_t j = 0; j < m; j++) {
            const float c[3] = {u(rng) * 0.3f, u(rng) * 0.3f, u(rng) * 0.3f};
            for (int k = 0; k < 3; k++)
                for (int a = 0; a < 3; a++) mesh[j].v[k][a] = c[a] + u(rng) * 0.15f;
        }
        if (m >= 2) mesh[1] = mesh[0];
        if (m >= 12) mesh[5].v[1][2] = nan, mesh[7] = mesh[3];
        const uint32_t G = group_of(m);
        std::vector<PoseSweep> poses;
        for (size_t k = 0; k < 24 && !recs.empty(); k++) {
            const DevTri& t = b.tris[recs[rng() % recs.size()]];
            PoseSweep s;
            float off[3];
            for (int a = 0; a < 3; a++) off[a] = u(rng), s.position[a] = t.v0[a] + off[a] * (k % 3 == 0 ? 0.2f : k % 3 == 1 ? 1.5f : 6.0f);
            for (int a = 0; a < 4; a++) s.rotation[a] = u(rng) * (k % 4 == 0 ? 3.0f : 1.0f);
            if (k % 8 == 1) s.rotation[0] = s.rotation[1] = s.rotation[2] = 0.0f, s.rotation[3] = -3.0f;
            for (int a = 0; a < 3; a++) s.d[a] = -off[a] * (0.5f + u(rng) * 0.25f);
            if (k % 6 == 5) s.d[k % 3] = 0.0f;
            s.tmax = k % 5 == 4 ? 0.75f : inf;
            poses.push_back(s);
        }
        for (size_t k = 0; k < 6; k++) { // scattered, and toward the spheres
            PoseSweep s;
            const Sphere& sp = spheres[k % 3];
            for (int a = 0; a < 3; a++) s.position[a] = k % 2 ? sp.centre[a] + u(rng) * 4.0f : u(rng) * 12.0f;
            for (int a = 0; a < 4; a++) s.rotation[a] = u(rng);
            for (int a = 0; a < 3; a++) s.d[a] = k % 2 ? sp.centre[a] - s.position[a] : u(rng);
            s.tmax = inf;
            poses.push_back(s);
        }
        poses.push_back({{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, -1.0f}, inf});      // invalid poses: not walked
        poses.push_back({{0.0f, 0.0f, 0.0f}, {3e19f, 3e19f, 0.0f, 1.0f}, {0.0f, 0.0f, -1.0f}, inf});    // the norm overflows
        poses.push_back({{nan, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 1.0f}, {0.0f, 0.0f, -1.0f}, inf});
        poses.push_back({{0.0f, inf, 0.0f}, {0.0f, 0.0f, 0.0f, 1.0f}, {0.0f, 0.0f, -1.0f}, inf});
        poses.push_back({{0.0f, 0.0f, 0.0f}, {0.0f, nan, 0.0f, 1.0f}, {0.0f, 0.0f, -1.0f}, inf});
        poses.push_back({{1.0f, 2.0f, 3.0f}, {0.1f, 0.2f, 0.3f, 1.0f}, {0.0f, 0.0f, 0.0f}, inf});       // valid pose, every triangle a miss
        poses.push_back({{1.0f, 2.0f, 3.0f}, {0.1f, 0.2f, 0.3f, 1.0f}, {0.0f, 0.0f, -1.0f}, 0.0f});
        poses.push_back({{1.0f, 2.0f, 3.0f}, {0.1f, 0.2f, 0.3f, 1.0f}, {0.0f, 0.0f, -1.0f}, nan});

        for (const PoseSweep& s : poses) {
            n_poses++;
            MpPose P;
            const bool valid = mp_pose(s.position, s.rotation, P);
            // the brute force: every (j, primitive) pair, no limit on the time
            uint32_t want[8];
            {
                MpBest bb;
                mp_best_init(bb, s.tmax);
                size_t at_least = 0;
                for (uint32_t j = 0; valid && j < m; j++) {
                    float q[3][3];
                    posed(mesh[j], P, q);
                    if (!st_query_valid(q[0], q[1], q[2], s.d, s.tmax)) continue;
                    const StQuery sq = st_query(q[0], q[1], q[2], s.d, s.tmax);
                    auto offer = [&](uint64_t c, uint32_t slot) {
                        if (c < sw_start(s.tmax) && c == bb.order && bb.j != MP_NONE) at_least++;
                        if (c < bb.order) bb.order = c, bb.j = j, bb.slot = slot, at_least = 1; // strict: at equal (t, key) the lower j stays
                    };
                    for (uint32_t i = 0; i < spheres.size(); i++) offer(cp_order(st_sphere(spheres[i].centre, spheres[i].radius, sq, q[1], q[2]), i), i);
                    for (uint32_t r : recs) {
                        const DevTri& t = b.tris[r];
                        uint32_t axis;
                        float w_in;
                        offer(cp_order(st_triangle(t.v0, t.e1, t.e2, sq, INFINITY, axis, w_in), t.prim_id ^ RT_PRIM_SPHERE_FLAG), r);
                    }
                }
                reduce(b, spheres, mesh, s, P, valid, {bb}, want);
                found += want[6] != RT_PRIM_MISS;
                at_start += want[6] != RT_PRIM_MISS && want[3] == 0u;
                tied += at_least > 1;
            }
            auto compare = [&](const char* what, const uint32_t got[8]) {
                if (std::memcmp(got, want, sizeof want) == 0) return;
                if (g_fail < 20)
                    std::printf("FAIL: m %u pose (%.9g %.9g %.9g | %.9g %.9g %.9g %.9g | d %.9g %.9g %.9g, tmax %.9g) %s: triangle %u prim %08x t %.9g axis %u, "
                                "brute force triangle %u prim %08x t %.9g axis %u\n",
                                m, s.position[0], s.position[1], s.position[2], s.rotation[0], s.rotation[1], s.rotation[2], s.rotation[3], s.d[0], s.d[1], s.d[2],
                                s.tmax, what, got[5], got[6], cp_float(got[3]), got[4], want[5], want[6], cp_float(want[3]), want[4]);
                g_fail++;
            };
            std::vector<TurnAccess> acc(G);
            for (TurnAccess& a : acc) a.init(b);
            stack_size = acc[0].stack.size();
            std::vector<MpBest> lanes(G);
            uint32_t got[8];
            // without the word, lane after lane
            for (uint32_t g = 0; g < G; g++) {
                mp_best_init(lanes[g], s.tmax);
                if (valid) lane_sweep(acc[g], b, spheres, mesh, s, P, g, G, MpNoShare{}, lanes[g]);
            }
            reduce(b, spheres, mesh, s, P, valid, lanes, got);
            compare("without the word", got);
            for (TurnAccess& a : acc) plain_nodes += a.nodes, a.nodes = 0;
            // with the word, in three orders, two lanes at a time
            std::vector<uint32_t> order(G);
            for (int pass = 0; pass < 3; pass++) {
                std::iota(order.begin(), order.end(), 0u);
                if (pass == 1) std::reverse(order.begin(), order.end());
                if (pass == 2) std::shuffle(order.begin(), order.end(), rng);
                uint32_t word = cp_bits(s.tmax);
                for (uint32_t g = 0; g < G; g++) mp_best_init(lanes[g], s.tmax);
                for (uint32_t k = 0; valid && k < G; k += 2) {
                    Baton baton;
                    const bool pair = k + 1 < G;
                    if (!pair) baton.done[1] = true;
                    auto run = [&](int me) {
                        const uint32_t g = order[k + (uint32_t)me];
                        acc[g].baton = &baton, acc[g].me = me;
                        baton.start(me);
                        lane_sweep(acc[g], b, spheres, mesh, s, P, g, G, HostWord{&word}, lanes[g]);
                        baton.finish(me);
                        acc[g].baton = nullptr;
                    };
                    if (pair) {
                        std::thread other(run, 1);
                        run(0);
                        other.join();
                    } else {
                        run(0);
                    }
                }
                reduce(b, spheres, mesh, s, P, valid, lanes, got);
                compare(pass == 0 ? "forward" : pass == 1 ? "reverse" : "shuffled", got);
                if (pass == 0)
                    for (TurnAccess& a : acc) shared_nodes += a.nodes;
                for (TurnAccess& a : acc) a.nodes = 0;
            }
            for (const TurnAccess& a : acc) max_sp = std::max(max_sp, a.max_sp);

            // the overlap answer: lanes as k_overlap_mesh runs them against every (j, primitive) pair
            {
                HostKeyAccess oa;
                oa.init(b);
                uint64_t pairs_walk = 0, pairs_brute = 0;
                uint32_t first_walk = MP_NONE, first_brute = MP_NONE;
                for (uint32_t j = 0; valid && j < m; j++) {
                    float q[3][3];
                    posed(mesh[j], P, q);
                    if (!ot_query_valid(q[0], q[1], q[2])) continue;
                    OtQuery oq;
                    ot_query_init(oq, q[0], q[1], q[2]);
                    OvList list;
                    ov_list_init(list, 0u);
                    uint32_t c = 0;
                    for (uint32_t i = 0; i < spheres.size(); i++)
                        if (ot_sphere(spheres[i].centre, spheres[i].radius, oq)) ov_list_offer(oa, list, i), c++;
                    ot_walk<OV_COUNT_ALL>(oa, (uint32_t)b.nodes.size(), oq, list);
                    for (uint32_t r : recs) c += ot_triangle(b.tris[r].v0, b.tris[r].e1, b.tris[r].e2, oq) ? 1u : 0u;
                    pairs_walk += list.total, pairs_brute += c;
                    if (list.total && first_walk == MP_NONE) first_walk = j;
                    if (c && first_brute == MP_NONE) first_brute = j;
                }
                max_sp = std::max(max_sp, oa.max_sp);
                if (pairs_walk != pairs_brute || first_walk != first_brute) {
                    if (g_fail < 20)
                        std::printf("FAIL: m %u overlap: walk %llu pairs first %u, brute force %llu pairs first %u\n", m, (unsigned long long)pairs_walk, first_walk,
                                    (unsigned long long)pairs_brute, first_brute);
                    g_fail++;
                }
            }
        }
    }
    if (shared_nodes > plain_nodes) {
        std::printf("FAIL: %llu node visits with the word, %llu without\n", shared_nodes, plain_nodes);
        g_fail++;
    }
    std::printf("node visits: %llu with the shared word, %llu without (%.3f)\n", shared_nodes, plain_nodes,
                plain_nodes ? (double)shared_nodes / (double)plain_nodes : 1.0);
    std::printf("kind %d n %zu method %d: %zu nodes depth %u, %zu poses (%zu hit, %zu of them at the start, %zu with a tie for the first contact), stack %d of %zu, "
                "%d failures\n",
                kind, n, opt.method, b.nodes.size(), b.depth, n_poses, found, at_start, tied, max_sp, stack_size, g_fail);
    return g_fail ? 1 : 0;
}
