// host_access.h — the Access that group_walk (gpu_raytracer_amd/csrc/group_walk.h) asks of its caller, for the host checks
// (check_closest_point, check_closest_point_all, check_sweep, check_overlap): a built tree's nodes and records, a stack of the entries
// a lane of the kernel owns and, for the two listing queries, the list words the launch provides.  Every index is checked; a walk that
// leaves its tree, its stack or its list ends the program with a FAIL line.
#ifndef RT_TESTS_HOST_ACCESS_H
#define RT_TESTS_HOST_ACCESS_H

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh_builder.h"

struct HostAccess {
    const rt::BvhBuild* b;
    std::vector<uint64_t> stack; // the entries a lane of the kernel owns: DevScene::stack_entries / 2 + 1
    int max_sp = 0;
    unsigned long long nodes = 0, tris = 0;

    // the kernel's LDS per lane: DevScene::stack_entries / 2 + 1 with stack_entries = 2 * depth + 2
    void init(const rt::BvhBuild& build) { b = &build, stack.resize((2u * build.depth + 2u) / 2u + 1u); }
    void node(uint32_t idx, uint32_t w[20]) {
        if (idx >= b->nodes.size()) {
            std::printf("FAIL: node %u out of %zu\n", idx, b->nodes.size());
            std::exit(1);
        }
        static_assert(sizeof(DevNode8) == 80, "DevNode8 is 20 words");
        std::memcpy(w, &b->nodes[idx], sizeof(DevNode8));
        nodes++;
    }
    void record(uint32_t slot, float q[9], uint32_t ids[3]) {
        if (slot >= b->tris.size()) {
            std::printf("FAIL: record %u out of %zu\n", slot, b->tris.size());
            std::exit(1);
        }
        const DevTri& t = b->tris[slot];
        for (int a = 0; a < 3; a++) q[a] = t.v0[a], q[3 + a] = t.e1[a], q[6 + a] = t.e2[a];
        ids[0] = t.material_id, ids[1] = t.prim_id, ids[2] = t.leaf_count;
        tris++;
    }
    void check_sp(int sp) const {
        if (sp < 0 || (size_t)sp >= stack.size()) {
            std::printf("FAIL: stack entry %d of %zu\n", sp, stack.size());
            std::exit(1);
        }
    }
    void push(int sp, uint32_t base, uint32_t bits) {
        check_sp(sp);
        stack[(size_t)sp] = ((uint64_t)base << 32) | bits;
        if (sp + 1 > max_sp) max_sp = sp + 1;
    }
    void pop(int sp, uint32_t& base, uint32_t& bits) {
        check_sp(sp);
        base = (uint32_t)(stack[(size_t)sp] >> 32), bits = (uint32_t)stack[(size_t)sp];
    }
};

// with the words a lane of k_cp_nearest_all owns: 3 * max_nearest
struct HostListAccess : HostAccess {
    std::vector<uint32_t> list;

    void check_k(uint32_t k) const {
        if ((size_t)3 * k + 2 >= list.size()) {
            std::printf("FAIL: list entry %u of %zu\n", k, list.size() / 3);
            std::exit(1);
        }
    }
    void list_get(uint32_t k, uint32_t& d2, uint32_t& key, uint32_t& slot) const {
        check_k(k);
        d2 = list[3 * k], key = list[3 * k + 1], slot = list[3 * k + 2];
    }
    void list_set(uint32_t k, uint32_t d2, uint32_t key, uint32_t slot) {
        check_k(k);
        list[3 * k] = d2, list[3 * k + 1] = key, list[3 * k + 2] = slot;
    }
};

// with the words a lane of k_overlap_box owns: max_prims
struct HostKeyAccess : HostAccess {
    std::vector<uint32_t> list;

    void check_k(uint32_t k) const {
        if ((size_t)k >= list.size()) {
            std::printf("FAIL: list entry %u of %zu\n", k, list.size());
            std::exit(1);
        }
    }
    uint32_t list_get(uint32_t k) const {
        check_k(k);
        return list[k];
    }
    void list_set(uint32_t k, uint32_t key) {
        check_k(k);
        list[k] = key;
    }
};

#endif
