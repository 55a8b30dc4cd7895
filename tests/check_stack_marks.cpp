// A MODEL of the traversal stacks' step rules, not the kernels: it replays, on the host builders' trees (gpu_raytracer_amd/csrc/
// bvh_builder.cpp, methods 0 and 1), the two stack disciplines of the device walks and prints how many entries a lane ever holds.
// Host code; built by tests/test_stack_cases.py with AddressSanitizer + UBSan, as tests/test_device_bvh.py builds check_bvh.cpp.
//   (a) one entry per visit: `traverse` of device_common.h (and traverse_all, the parity walks, and group_walk under the closest-point,
//       nearest-K, sweep and overlap queries): a visit takes a slot off the current group, parks the rest if any is left, tests the
//       node's leaves at once.  Bound: depth - 1 (group_walk.h).
//   (b) k_wf_trace of wavefront.hip: 64 lanes in lock step; what is left of a node is a group G of inner children and a group T of
//       leaves; a visit parks the siblings still to visit and, when the lane already holds a postponed T, the new T; the wave takes
//       node steps while fewer than RT_WF8_LEAF_THRESHOLD (24) lanes hold a T, else one leaf slot per lane per leaf step.  Bound:
//       2 * depth + 2, of which RT_WF8_LDS_STACK (8) live in LDS and the rest in the HBM overflow area.  The replay has no refill:
//       a wave is 64 consecutive rays of the file, and its lanes idle once their ray is finished.
// Nodes are decoded as bvh_check.h decodes them (float64 planes); the box filter is the kernels' formula (visit_node8: slack and
// limit included) evaluated in float64, the triangle test Moeller-Trumbore in float64 on the DevTri records.  The marks therefore
// need not be the device's to the entry; tests/test_gpu_stack_marks.py reads those from the counting kernel.
//
// Triangles and rays REACH this program through small binary files the test writes (tests/stack_cases.py is the one statement of the
// deck): <tris.bin> float32 [n][3][3] corners, each <rays.bin> float32 [N][8] = ox oy oz tmin dx dy dz tmax.
// Besides the marks it counts, per ray set, the rays whose closest hit was found THROUGH THE OVERFLOW: accepted in a leaf group that was
// popped from an entry beyond the LDS part, or that came from a node reached through such an entry.  Those are the rays for which a lost
// or misaddressed overflow entry changes the answer.
// usage: check_stack_marks <tris.bin> <method> <lds entries: RT_WF8_LDS_STACK> <rays.bin> [<rays.bin> ...]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "bvh_builder.h"
#include "bvh_check.h"

using namespace rt;
using namespace rtcheck;

static const uint32_t NONE = 0xFFFFFFFFu, MISS = 0xFFFFFFFFu;
static const int WAVE = 64, LEAF_THRESHOLD = 24;
static const double SLACK = 1.0e-5, LIMIT = 1.0000153;

static std::vector<float> read_floats(const char* path, size_t per_record) {
    std::vector<float> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::printf("FAIL: cannot open %s\n", path);
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes < 0 || (size_t)bytes % (per_record * sizeof(float)) != 0) {
        std::printf("FAIL: %s holds %ld bytes, not records of %zu floats\n", path, bytes, per_record);
        std::exit(2);
    }
    v.resize((size_t)bytes / sizeof(float));
    if (!v.empty() && std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) {
        std::printf("FAIL: short read of %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

struct Ray {
    double o[3], d[3], inv[3], tmin, t;
    uint32_t prim, oct;
};

static Ray make_ray(const float* r) {
    Ray y;
    for (int a = 0; a < 3; a++) {
        y.o[a] = r[a];
        y.d[a] = r[4 + a];
        const double c = std::fabs(y.d[a]) < 1e-30 ? std::copysign(1e-30, y.d[a]) : y.d[a]; // make_filter_ray
        y.inv[a] = 1.0 / c;
    }
    y.tmin = r[3];
    y.t = r[7];
    y.prim = MISS;
    y.oct = (y.inv[0] < 0.0 ? 1u : 0u) | (y.inv[1] < 0.0 ? 2u : 0u) | (y.inv[2] < 0.0 ? 4u : 0u);
    return y;
}

// the set slot of m with the smallest (slot XOR oct): first_slot of device_common.h, the table of k_wf_trace
static uint32_t first_slot(uint32_t m, uint32_t oct) {
    uint32_t best = 0, key = 99;
    for (uint32_t i = 0; i < 8; i++)
        if (((m >> i) & 1u) && (i ^ oct) < key) key = i ^ oct, best = i;
    return best;
}

// visit_node8: the mask of occupied slots the ray enters within [0, closest]
static uint32_t visit(const BvhBuild& b, uint32_t idx, const Ray& y, uint32_t& cb, uint32_t& tb, uint32_t& im, uint32_t& lm) {
    const DevNode8& n = b.nodes[idx];
    im = n.ex_imask >> 24;
    lm = n.lmask & 0xFFu;
    cb = n.child_base;
    tb = n.tri_base;
    double A[3], B[3], E[3];
    for (int a = 0; a < 3; a++) {
        const double scale = std::ldexp(1.0, (int)(int8_t)((n.ex_imask >> (8 * a)) & 0xFFu));
        A[a] = scale * y.inv[a];
        B[a] = ((double)n.org[a] - y.o[a]) * y.inv[a];
        E[a] = (255.0 * std::fabs(A[a]) + std::fabs(B[a])) * SLACK;
    }
    const double limit = y.t * LIMIT;
    uint32_t hm = 0;
    for (int s = 0; s < 8; s++) {
        if (!(((im | lm) >> s) & 1u)) continue;
        double tmin = 0.0, tmax = limit;
        for (int a = 0; a < 3; a++) {
            const double qlo = (n.qlo[a][s >> 2] >> (8 * (s & 3))) & 0xFFu, qhi = (n.qhi[a][s >> 2] >> (8 * (s & 3))) & 0xFFu;
            const bool pos = y.inv[a] >= 0.0;
            const double tn = (pos ? qlo : qhi) * A[a] + B[a] - E[a], tf = (pos ? qhi : qlo) * A[a] + B[a] + E[a];
            tmin = std::max(tmin, tn);
            tmax = std::min(tmax, tf);
        }
        if (tmin <= tmax) hm |= 1u << s;
    }
    return hm;
}

// test_leaf: all triangles of the leaf whose first record is `first`; ANY: true at the first accepted one
static bool test_leaf(const BvhBuild& b, uint32_t first, Ray& y, bool any) {
    const uint32_t count = b.tris[first].leaf_count;
    for (uint32_t i = 0; i < count; i++) {
        const DevTri& t = b.tris[first + i];
        double e1[3], e2[3], s[3], h[3], q[3];
        for (int a = 0; a < 3; a++) e1[a] = t.e1[a], e2[a] = t.e2[a], s[a] = y.o[a] - (double)t.v0[a];
        h[0] = y.d[1] * e2[2] - y.d[2] * e2[1], h[1] = y.d[2] * e2[0] - y.d[0] * e2[2], h[2] = y.d[0] * e2[1] - y.d[1] * e2[0];
        const double det = e1[0] * h[0] + e1[1] * h[1] + e1[2] * h[2];
        if (std::fabs(det) < 1e-5) continue;
        const double f = 1.0 / det, u = f * (s[0] * h[0] + s[1] * h[1] + s[2] * h[2]);
        if (u < 0.0 || u > 1.0) continue;
        q[0] = s[1] * e1[2] - s[2] * e1[1], q[1] = s[2] * e1[0] - s[0] * e1[2], q[2] = s[0] * e1[1] - s[1] * e1[0];
        const double v = f * (y.d[0] * q[0] + y.d[1] * q[1] + y.d[2] * q[2]);
        if (v < 0.0 || u + v > 1.0) continue;
        const double tt = f * (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]);
        if (tt > y.tmin && (tt < y.t || (tt == y.t && t.prim_id < y.prim))) {
            y.t = tt;
            y.prim = t.prim_id;
            if (any) return true;
        }
    }
    return false;
}

static uint32_t popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// (a) `traverse`: -> the most entries the lane's stack ever held
static int walk_a(const BvhBuild& b, Ray y) {
    if (b.nodes.empty()) return 0;
    std::vector<std::pair<uint32_t, uint32_t>> stack;
    uint32_t g_base = 0, g_bits = 1u | (1u << 8);
    int mark = 0;
    for (;;) {
        if ((g_bits & 0xFFu) == 0u) {
            if (stack.empty()) break;
            g_base = stack.back().first, g_bits = stack.back().second;
            stack.pop_back();
        }
        const uint32_t i = first_slot(g_bits & 0xFFu, y.oct);
        g_bits ^= 1u << i;
        const uint32_t node = g_base + popc((g_bits >> 8) & ((1u << i) - 1u));
        if (g_bits & 0xFFu) {
            stack.emplace_back(g_base, g_bits);
            mark = std::max(mark, (int)stack.size());
        }
        uint32_t cb, tb, im, lm;
        const uint32_t hm = visit(b, node, y, cb, tb, im, lm);
        uint32_t t = hm & lm;
        while (t) {
            const uint32_t sl = first_slot(t, y.oct);
            t ^= 1u << sl;
            test_leaf(b, tb + RT_DEV_LEAF_STRIDE * popc(lm & ((1u << sl) - 1u)), y, false);
        }
        g_base = cb;
        g_bits = (hm & im) | (im << 8);
    }
    return mark;
}

// (b) k_wf_trace: one wave of up to 64 rays -> the most entries any lane ever held
struct Lane {
    Ray y;
    bool active = false;
    uint32_t cur = NONE, g_base = 0, g_bits = 0, t_base = 0, t_bits = 0, oct = 0;
    bool g_ovf = false, t_ovf = false, cur_ovf = false, hit_ovf = false; // the group / node / hit descends from an entry popped beyond the LDS part
    std::vector<std::pair<uint32_t, uint32_t>> stack; // (base | kind, bits)
};
static const uint32_t KIND_T = 0x80000000u;

static int walk_b(const BvhBuild& b, const Ray* rays, int n, bool any, int lds, size_t* hits, size_t* via_overflow) {
    Lane L[WAVE];
    for (int l = 0; l < n; l++) {
        L[l].y = rays[l];
        L[l].oct = any ? rays[l].oct ^ 7u : rays[l].oct; // shadow segments walk far to near
        L[l].g_bits = b.nodes.empty() ? 0u : (1u | (1u << 8));
        L[l].active = true;
    }
    int mark = 0;
    for (;;) {
        int m_node = 0, m_leaf = 0, still = 0;
        for (int l = 0; l < n; l++) { // fetch
            Lane& z = L[l];
            if (z.cur != NONE) {
                m_node++;
                m_leaf += (z.t_bits & 0xFFu) != 0u;
                continue;
            }
            if ((z.g_bits & 0xFFu) == 0u && !z.stack.empty()) {
                const std::pair<uint32_t, uint32_t> e = z.stack.back();
                const bool beyond = (int)z.stack.size() - 1 >= lds; // the entry's index: in the overflow area
                if (!(e.first & KIND_T)) {
                    z.stack.pop_back();
                    z.g_base = e.first, z.g_bits = e.second, z.g_ovf = beyond;
                } else if ((z.t_bits & 0xFFu) == 0u) {
                    z.stack.pop_back();
                    z.t_base = e.first & ~KIND_T, z.t_bits = e.second, z.t_ovf = beyond;
                }
            }
            if (z.g_bits & 0xFFu) {
                const uint32_t i = first_slot(z.g_bits & 0xFFu, z.oct);
                z.g_bits ^= 1u << i;
                z.cur = z.g_base + popc((z.g_bits >> 8) & ((1u << i) - 1u));
                z.cur_ovf = z.g_ovf;
            }
            m_node += z.cur != NONE;
            m_leaf += (z.t_bits & 0xFFu) != 0u;
        }
        if (m_node != 0 && m_leaf < LEAF_THRESHOLD) {
            for (int l = 0; l < n; l++) {
                Lane& z = L[l];
                if (z.cur == NONE) continue;
                uint32_t cb, tb, im, lm;
                const uint32_t hm = visit(b, z.cur, z.y, cb, tb, im, lm);
                z.cur = NONE;
                if (z.g_bits & 0xFFu) z.stack.emplace_back(z.g_base, z.g_bits);
                z.g_base = cb;
                z.g_bits = (hm & im) | (im << 8);
                z.g_ovf = z.cur_ovf;
                const uint32_t nt = hm & lm;
                if (nt) { // (a T parked under a node reached through the overflow lies beyond the LDS part itself: its index tells when it is popped)
                    if ((z.t_bits & 0xFFu) == 0u) z.t_base = tb, z.t_bits = nt | (lm << 8), z.t_ovf = z.cur_ovf;
                    else z.stack.emplace_back(tb | KIND_T, nt | (lm << 8));
                }
                mark = std::max(mark, (int)z.stack.size());
            }
        } else if (m_leaf != 0) {
            for (int l = 0; l < n; l++) {
                Lane& z = L[l];
                if ((z.t_bits & 0xFFu) == 0u) continue;
                const uint32_t i = first_slot(z.t_bits & 0xFFu, z.oct);
                z.t_bits ^= 1u << i;
                const uint32_t prim_before = z.y.prim;
                const double t_before = z.y.t;
                const bool stop = test_leaf(b, z.t_base + RT_DEV_LEAF_STRIDE * popc((z.t_bits >> 8) & ((1u << i) - 1u)), z.y, any);
                if (z.y.prim != prim_before || z.y.t != t_before) z.hit_ovf = z.t_ovf;
                if (stop) {
                    z.cur = NONE;
                    z.g_bits = z.t_bits = 0u;
                    z.stack.clear();
                }
            }
        }
        for (int l = 0; l < n; l++) {
            Lane& z = L[l];
            const bool busy = ((z.g_bits | z.t_bits) & 0xFFu) != 0u || !z.stack.empty() || z.cur != NONE;
            if (z.active && !busy) {
                z.active = false;
                if (hits && z.y.prim != MISS) (*hits)++;
                if (via_overflow && z.y.prim != MISS && z.hit_ovf) (*via_overflow)++;
            }
            still += busy;
        }
        if (!still) break;
    }
    return mark;
}

int main(int argc, char** argv) {
    if (argc < 5) {
        std::printf("usage: check_stack_marks <tris.bin> <method> <lds entries> <rays.bin> [<rays.bin> ...]\n");
        return 2;
    }
    const std::vector<float> corners = read_floats(argv[1], 9);
    const size_t n = corners.size() / 9;
    std::vector<BuildTri> tris(n);
    for (size_t i = 0; i < n; i++) {
        for (int a = 0; a < 3; a++) tris[i].v0[a] = corners[9 * i + a], tris[i].v1[a] = corners[9 * i + 3 + a], tris[i].v2[a] = corners[9 * i + 6 + a];
        tris[i].material_id = 0;
        tris[i].prim_id = (uint32_t)i;
    }
    BvhBuild b;
    BvhBuildOptions opt;
    opt.method = std::atoi(argv[2]);
    build_bvh(tris.data(), tris.size(), opt, b);
    std::vector<uint32_t> seen(n, 0);
    uint32_t real_depth = 0;
    size_t leaves = 0;
    check_tree(b, seen, &real_depth, &leaves);
    std::printf("tree method %d tris %zu nodes %zu leaves %zu depth %u real_depth %u failures %d\n", opt.method, n, b.nodes.size(), leaves, b.depth, real_depth, g_fail);
    const int tree_fail = g_fail;
    const int lds = std::atoi(argv[3]);
    for (int k = 4; k < argc; k++) {
        const std::vector<float> r = read_floats(argv[k], 8);
        const size_t nr = r.size() / 8;
        std::vector<Ray> rays(nr);
        for (size_t i = 0; i < nr; i++) rays[i] = make_ray(&r[8 * i]);
        int mark_a = 0, mark_b = 0, mark_b_any = 0;
        size_t hits = 0, waves = 0, via_overflow = 0;
        for (size_t i = 0; i < nr; i++) mark_a = std::max(mark_a, walk_a(b, rays[i]));
        for (size_t s = 0; s < nr; s += WAVE, waves++) {
            const int m = (int)std::min<size_t>(WAVE, nr - s);
            mark_b = std::max(mark_b, walk_b(b, &rays[s], m, false, lds, &hits, &via_overflow));
            mark_b_any = std::max(mark_b_any, walk_b(b, &rays[s], m, true, lds, nullptr, nullptr));
        }
        std::string name = argv[k];
        name = name.substr(name.find_last_of('/') + 1);
        std::printf("rays %s n %zu waves %zu mark_a %d mark_b %d mark_b_any %d hits %zu via_overflow %zu\n", name.c_str(), nr, waves, mark_a, mark_b, mark_b_any, hits, via_overflow);
    }
    return tree_fail ? 1 : 0;
}
