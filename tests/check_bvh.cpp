// Structural validator for the 8-wide quantised tree of gpu_raytracer_amd/csrc/bvh_builder.cpp (host code; built by
// tests/test_device_bvh.py with AddressSanitizer + UBSan).  It decodes nodes exactly as visit_node8 and the group walk do
// and checks what the kernels rely on:
//   * node 0 is the root of every non-empty build; inner children are consecutive nodes in slot order
//     (child_base + number of inner slots below), every leaf owns RT_DEV_LEAF_STRIDE records in slot order
//     (tri_base + stride * number of leaf slots below); imask and lmask are disjoint; a slot that is in neither is
//     EMPTY and its box inverted (the walk masks hits with imask | lmask, so a degenerate evaluation cannot follow it);
//   * every input triangle with finite coordinates appears in exactly one leaf, leaves hold 1..4 triangles, the run
//     length sits in the first record of the leaf and only there (padding records carry none);
//   * every triangle lies inside the dequantised box of every ancestor's child slot (the boxes are conservative);
//   * the reported depth bounds the real one and stays within the stack the kernels provide.
// usage: check_bvh <n_triangles> <seed> <kind> [method]   method: 0 binned SAH (default), 1 PLOC;   kind: 0 soup, 1 coplanar grid, 2 coincident points, 3 collinear chain,
//                                                      4 huge + tiny mixed, 5 with NaN / inf vertices
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "bvh_builder.h"
#include "bvh_check.h"

using namespace rt;
using namespace rtcheck;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atoll(argv[1]) : 1000;
    const uint32_t seed = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 1;
    const int kind = argc > 3 ? std::atoi(argv[3]) : 0;
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<BuildTri> tris(n);
    size_t n_finite = 0;
    for (size_t i = 0; i < n; i++) {
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
        bool finite = true;
        for (int a = 0; a < 3; a++) finite = finite && std::isfinite(t.v0[a]) && std::isfinite(t.v1[a]) && std::isfinite(t.v2[a]);
        n_finite += finite ? 1 : 0;
    }
    BvhBuild b;
    BvhBuildOptions opt;
    opt.method = argc > 4 ? std::atoi(argv[4]) : 0; // 0: binned SAH + insertion-based optimisation, 1: PLOC (the tree the device build makes)
    build_bvh(tris.data(), tris.size(), opt, b);
    std::vector<uint32_t> seen(n, 0);
    uint32_t real_depth = 0;
    size_t leaves = 0;
    check_tree(b, seen, &real_depth, &leaves);
    if (n_finite == 0) CHECK(b.nodes.empty() && b.tris.empty(), "empty build has nodes");
    size_t once = 0;
    for (size_t i = 0; i < n; i++) {
        bool finite = true;
        for (int a = 0; a < 3; a++) finite = finite && std::isfinite(tris[i].v0[a]) && std::isfinite(tris[i].v1[a]) && std::isfinite(tris[i].v2[a]);
        CHECK(seen[i] == (finite ? 1u : 0u), "triangle %zu appears %u times", i, seen[i]);
        once += seen[i] == 1;
    }
    std::printf("kind %d n %zu: %zu nodes, %zu leaves, depth %u (reported %u), %zu triangles placed, %d failures, nodes_hash %08x tris_hash %08x\n", kind, n, b.nodes.size(),
                leaves, real_depth, b.depth, once, g_fail, hash_nodes(b), hash_tris(b));
    return g_fail ? 1 : 0;
}
