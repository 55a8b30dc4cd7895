// bvh_builder.cpp — binned-SAH binary build (host, multi-threaded) collapsed into the 8-wide quantised layout, see bvh_builder.h.
#include "bvh_builder.h"
#include "bvh_rules.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <future>
#include <limits>
#include <numeric>
#include <thread>
#include <utility>

namespace rt {
namespace {

struct TmpNode {
    Box box;
    uint32_t left, right; // inner: TmpNode indices; leaf: left = 0xFFFFFFFF
    uint32_t start, count;
};

#ifndef RT_BVH_REINSERT
#define RT_BVH_REINSERT 1
#endif
#ifndef RT_BVH_REINSERT_PASSES
#define RT_BVH_REINSERT_PASSES 2
#endif
#ifndef RT_BVH_REINSERT_MAX
#define RT_BVH_REINSERT_MAX 150000
#endif
#ifndef RT_BVH_REINSERT_FRACTION
#define RT_BVH_REINSERT_FRACTION 0.25
#endif
#ifndef RT_BVH_COLLAPSE_DP
#define RT_BVH_COLLAPSE_DP 1 /* measured: 0.8 % (sponza-like) to 1.5 % (bistro-like) over the greedy rule */
#endif
#ifndef RT_BVH_BINS
#define RT_BVH_BINS 32 /* SAH bins per axis: 32 instead of 16 gives 3 % fewer node visits on the sponza-like scene (+2 % throughput), 48 / 64 no more */
#endif
constexpr int kBins = RT_BVH_BINS;

struct Builder {
    const BuildTri* tris;
    std::vector<Box> boxes;
    std::vector<float> cent; // 3 per triangle
    std::vector<uint32_t> ids;
    std::vector<TmpNode> nodes;
    std::atomic<uint32_t> next_node{0};
    BvhBuildOptions opt;
    std::atomic<int> tasks_in_flight{0};
    int max_tasks = 1;

    uint32_t alloc() { return next_node.fetch_add(1); }

    static uint32_t ceil_log2(uint64_t v) {
        uint32_t r = 0;
        while ((1ull << r) < v) r++;
        return r;
    }

    void make_leaf(uint32_t me, uint32_t lo, uint32_t hi, const Box& box) {
        std::sort(ids.begin() + lo, ids.begin() + hi, [&](uint32_t a, uint32_t b) { return tris[a].prim_id < tris[b].prim_id; });
        nodes[me].box = box;
        nodes[me].left = nodes[me].right = 0xFFFFFFFFu;
        nodes[me].start = lo;
        nodes[me].count = hi - lo;
    }

    // depth = number of inner nodes above this node.  A subtree of n triangles split at the
    // object median needs ceil(log2(ceil(n / max_leaf))) more inner levels.
    void build(uint32_t me, uint32_t lo, uint32_t hi, uint32_t depth) {
        uint32_t n = hi - lo;
        Box box, cbox;
        box.reset();
        cbox.reset();
        for (uint32_t i = lo; i < hi; i++) {
            box.grow(boxes[ids[i]]);
            cbox.grow(&cent[3 * (size_t)ids[i]]);
        }
        if (n == 1) {
            make_leaf(me, lo, hi, box);
            return;
        }
        uint32_t levels_needed = ceil_log2((n + opt.max_leaf - 1) / opt.max_leaf);
        bool force_median = depth + levels_needed + 1 >= opt.max_depth;

        uint32_t mid = 0;
        bool have_split = false;
        if (!force_median) {
            float best_cost = std::numeric_limits<float>::infinity();
            int best_axis = -1, best_bin = -1;
            for (int axis = 0; axis < 3; axis++) {
                float cmin = cbox.mn[axis], cext = cbox.mx[axis] - cbox.mn[axis];
                if (!(cext > 0.0f)) continue;
                float scale = (float)kBins / cext;
                Box bin_box[kBins];
                uint32_t bin_cnt[kBins];
                for (int b = 0; b < kBins; b++) {
                    bin_box[b].reset();
                    bin_cnt[b] = 0;
                }
                for (uint32_t i = lo; i < hi; i++) {
                    int b = (int)((cent[3 * (size_t)ids[i] + axis] - cmin) * scale);
                    b = std::min(std::max(b, 0), kBins - 1);
                    bin_cnt[b]++;
                    bin_box[b].grow(boxes[ids[i]]);
                }
                float right_area[kBins];
                uint32_t right_cnt[kBins];
                Box acc;
                acc.reset();
                uint32_t cnt = 0;
                for (int b = kBins - 1; b > 0; b--) {
                    acc.grow(bin_box[b]);
                    cnt += bin_cnt[b];
                    right_area[b] = acc.half_area();
                    right_cnt[b] = cnt;
                }
                acc.reset();
                cnt = 0;
                for (int b = 0; b < kBins - 1; b++) {
                    acc.grow(bin_box[b]);
                    cnt += bin_cnt[b];
                    if (cnt == 0 || right_cnt[b + 1] == 0) continue;
                    float cost = acc.half_area() * (float)cnt + right_area[b + 1] * (float)right_cnt[b + 1];
                    if (cost < best_cost) {
                        best_cost = cost;
                        best_axis = axis;
                        best_bin = b;
                    }
                }
            }
            if (best_axis >= 0) {
                float parent_area = box.half_area();
                float split_cost = opt.cost_traverse + opt.cost_intersect * (parent_area > 0.0f ? best_cost / parent_area : (float)n);
                float leaf_cost = opt.cost_intersect * (float)n;
                if (n <= opt.max_leaf && leaf_cost <= split_cost) {
                    make_leaf(me, lo, hi, box);
                    return;
                }
                float cmin = cbox.mn[best_axis], cext = cbox.mx[best_axis] - cbox.mn[best_axis];
                float scale = (float)kBins / cext;
                auto it = std::partition(ids.begin() + lo, ids.begin() + hi, [&](uint32_t id) {
                    int b = (int)((cent[3 * (size_t)id + best_axis] - cmin) * scale);
                    b = std::min(std::max(b, 0), kBins - 1);
                    return b <= best_bin;
                });
                mid = (uint32_t)(it - ids.begin());
                have_split = mid > lo && mid < hi;
            } else if (n <= opt.max_leaf) { // all centroids coincide
                make_leaf(me, lo, hi, box);
                return;
            }
        } else if (n <= opt.max_leaf) {
            make_leaf(me, lo, hi, box);
            return;
        }
        if (!have_split) { // object median along the widest centroid axis (ties by id: deterministic)
            int axis = 0;
            float ext = cbox.mx[0] - cbox.mn[0];
            for (int a = 1; a < 3; a++)
                if (cbox.mx[a] - cbox.mn[a] > ext) {
                    ext = cbox.mx[a] - cbox.mn[a];
                    axis = a;
                }
            mid = lo + n / 2;
            std::nth_element(ids.begin() + lo, ids.begin() + mid, ids.begin() + hi, [&](uint32_t a, uint32_t b) {
                float ca = cent[3 * (size_t)a + axis], cb = cent[3 * (size_t)b + axis];
                return ca < cb || (ca == cb && a < b);
            });
        }
        uint32_t l = alloc(), r = alloc();
        nodes[me].box = box;
        nodes[me].left = l;
        nodes[me].right = r;
        nodes[me].start = nodes[me].count = 0;
        bool spawn = n > 32768 && tasks_in_flight.load(std::memory_order_relaxed) < max_tasks;
        if (spawn) {
            tasks_in_flight.fetch_add(1);
            auto fut = std::async(std::launch::async, [this, l, lo, mid, depth] { build(l, lo, mid, depth + 1); });
            build(r, mid, hi, depth + 1);
            fut.get();
            tasks_in_flight.fetch_sub(1);
        } else {
            build(l, lo, mid, depth + 1);
            build(r, mid, hi, depth + 1);
        }
    }
};

#if RT_BVH_REINSERT
// Insertion-based optimisation of the binary tree (after Bittner, Hapala, Havran, "Fast Insertion-Based Optimization of
// Bounding Volume Hierarchies", 2013, in its simplest form): take a subtree out (its parent goes with it, the sibling moves
// up), find by branch and bound the node next to which it enlarges the ancestors' boxes least, and put it back there.
// Candidates are the nodes with the largest area first.  The sum of the inner nodes' areas - what a top-down SAH build
// only approximates greedily - can only go down.  Returns the depth of the resulting tree.
static float union_area(const Box& a, const Box& b) {
    Box u = a;
    u.grow(b);
    return u.half_area();
}
static uint32_t reinsertion_optimize(std::vector<TmpNode>& nodes, uint32_t n_nodes, uint32_t& root, int passes, double fraction) {
    std::vector<uint32_t> parent(n_nodes, 0xFFFFFFFFu);
    auto is_leaf = [&](uint32_t x) { return nodes[x].left == 0xFFFFFFFFu; };
    {
        std::vector<uint32_t> st{root};
        while (!st.empty()) {
            const uint32_t x = st.back();
            st.pop_back();
            if (is_leaf(x)) continue;
            parent[nodes[x].left] = parent[nodes[x].right] = x;
            st.push_back(nodes[x].left);
            st.push_back(nodes[x].right);
        }
    }
    auto refit_up = [&](uint32_t x) { // recompute boxes from x to the root
        while (x != 0xFFFFFFFFu) {
            Box bx = nodes[nodes[x].left].box;
            bx.grow(nodes[nodes[x].right].box);
            nodes[x].box = bx;
            x = parent[x];
        }
    };
    struct Entry {
        float induced;
        uint32_t node;
        bool operator<(const Entry& o) const { return induced > o.induced; } // min-heap on the induced cost
    };
    for (int pass = 0; pass < passes; pass++) {
        std::vector<uint32_t> cand;
        for (uint32_t x = 0; x < n_nodes; x++)
            if (x != root && parent[x] != 0xFFFFFFFFu && parent[x] != root) cand.push_back(x);
        // a bounded number of candidates per pass (the step is serial: ~1.4 us per candidate): the largest nodes matter most
        const size_t take = std::min({cand.size(), (size_t)std::max(1.0, fraction * (double)cand.size()), (size_t)RT_BVH_REINSERT_MAX});
        std::partial_sort(cand.begin(), cand.begin() + (long)take, cand.end(), [&](uint32_t a, uint32_t b) {
            const float aa = nodes[a].box.half_area(), ab = nodes[b].box.half_area();
            return aa > ab || (aa == ab && a < b);
        });
        cand.resize(take);
        std::vector<Entry> heap;
        for (uint32_t nd : cand) {
            const uint32_t p = parent[nd];
            if (p == 0xFFFFFFFFu || p == root) continue; // moved under the root by an earlier step
            const uint32_t g = parent[p];
            const uint32_t sib = nodes[p].left == nd ? nodes[p].right : nodes[p].left;
            // take nd (and p) out: the sibling takes p's place
            if (nodes[g].left == p) nodes[g].left = sib;
            else nodes[g].right = sib;
            parent[sib] = g;
            refit_up(g);
            // branch and bound for the best neighbour
            const Box& nb = nodes[nd].box;
            const float na = nb.half_area();
            float best_cost = std::numeric_limits<float>::infinity();
            uint32_t best = sib;
            heap.clear();
            heap.push_back({0.0f, root});
            while (!heap.empty()) {
                std::pop_heap(heap.begin(), heap.end());
                const Entry e = heap.back();
                heap.pop_back();
                if (e.induced + na >= best_cost) break; // nothing cheaper can follow (heap order)
                const float direct = union_area(nodes[e.node].box, nb);
                const float total = e.induced + direct;
                if (total < best_cost) {
                    best_cost = total;
                    best = e.node;
                }
                if (!is_leaf(e.node)) {
                    const float child_induced = total - nodes[e.node].box.half_area();
                    if (child_induced + na < best_cost) {
                        heap.push_back({child_induced, nodes[e.node].left});
                        std::push_heap(heap.begin(), heap.end());
                        heap.push_back({child_induced, nodes[e.node].right});
                        std::push_heap(heap.begin(), heap.end());
                    }
                }
            }
            // put it back: p becomes the parent of (best, nd) where best was
            const uint32_t bp = parent[best];
            nodes[p].left = best;
            nodes[p].right = nd;
            parent[best] = p;
            parent[nd] = p;
            parent[p] = bp;
            if (bp == 0xFFFFFFFFu) root = p;
            else if (nodes[bp].left == best) nodes[bp].left = p;
            else nodes[bp].right = p;
            refit_up(p);
        }
    }
    uint32_t depth = 0; // inner levels on the longest path
    std::vector<std::pair<uint32_t, uint32_t>> st{{root, 1u}};
    while (!st.empty()) {
        auto [x, d] = st.back();
        st.pop_back();
        if (is_leaf(x)) continue;
        depth = std::max(depth, d);
        st.push_back({nodes[x].left, d + 1});
        st.push_back({nodes[x].right, d + 1});
    }
    return depth;
}
#endif

// ---- PLOC on the host (bvh_rules.h rules 2 and 4, the rounds in sequence): what the device build (csrc/device_build.hip) does in
// kernels.  It fills `nodes` (leaves first: node i = the i-th triangle in Morton order) and returns the root.
uint32_t build_ploc(const std::vector<Box>& boxes, const std::vector<float>& cent, std::vector<uint32_t>& ids, std::vector<TmpNode>& nodes, uint32_t radius) {
    const size_t n = ids.size();
    Box cb;
    cb.reset();
    for (size_t i = 0; i < n; i++) cb.grow(&cent[3 * (size_t)ids[i]]);
    std::vector<std::pair<uint64_t, uint32_t>> keyed(n);
    for (size_t i = 0; i < n; i++) keyed[i] = {morton63(&cent[3 * (size_t)ids[i]], cb.mn, cb.mx), ids[i]};
    std::sort(keyed.begin(), keyed.end());
    for (size_t i = 0; i < n; i++) ids[i] = keyed[i].second;
    nodes.resize(2 * n);
    std::vector<uint32_t> cl(n), nn(n), next;
    for (size_t i = 0; i < n; i++) {
        nodes[i].box = boxes[ids[i]];
        nodes[i].left = nodes[i].right = 0xFFFFFFFFu;
        nodes[i].start = (uint32_t)i;
        nodes[i].count = 1;
        cl[i] = (uint32_t)i;
    }
    uint32_t n_nodes = (uint32_t)n, m = (uint32_t)n, level = 0;
    next.reserve(n);
    while (m > 1) {
        for (uint32_t i = 0; i < m; i++)
            nn[i] = ploc_nearest(i, m, radius, level, [&](uint32_t j) {
                Box u = nodes[cl[i]].box;
                u.grow(nodes[cl[j]].box);
                return u.half_area();
            });
        next.clear();
        const uint32_t nodes_before = n_nodes;
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t role = ploc_role(nn.data(), i);
            if (role == 0u) next.push_back(cl[i]);
            if (role != 1u) continue;
            TmpNode& p = nodes[n_nodes];
            p.box = nodes[cl[i]].box;
            p.box.grow(nodes[cl[nn[i]]].box);
            p.left = cl[i];
            p.right = cl[nn[i]];
            p.start = p.count = 0;
            next.push_back(n_nodes++);
        }
        if (ploc_escalates(n_nodes - nodes_before, m, level)) level++;
        m = (uint32_t)next.size();
        std::copy(next.begin(), next.end(), cl.begin());
    }
    nodes.resize(n_nodes);
    return cl[0];
}

// ---- 8-wide collapse (DevNode8): the program of bvh_rules.h over the binary tree, then the emission, depth first, appending.
struct HostTree { // the binary tree as rules 6 and 9 read it
    const std::vector<TmpNode>& nodes;
    const std::vector<CollapseRec>& dp;
    const std::vector<uint32_t>& ids;
    bool inner(uint32_t n, uint32_t& l, uint32_t& r) const {
        l = nodes[n].left, r = nodes[n].right;
        return l != 0xFFFFFFFFu;
    }
    const CollapseRec& rec(uint32_t n) const { return dp[n]; }
    uint32_t leaf_tris(uint32_t n, uint32_t* out, uint32_t ng) const {
        for (uint32_t i = 0; i < nodes[n].count && ng < RT_DEV_LEAF_STRIDE; i++) out[ng++] = ids[nodes[n].start + i];
        return ng;
    }
};

void collapse8(const std::vector<TmpNode>& nodes, const std::vector<uint32_t>& ids, uint32_t n_nodes, uint32_t root, const BuildTri* tris_in, const BvhBuildOptions& opt,
               uint32_t max_leaf, BvhBuild& out) {
    std::vector<CollapseRec> dp(n_nodes);
    {
        struct Frame {
            uint32_t node;
            int phase;
        };
        std::vector<Frame> st;
        st.push_back({root, 0});
        while (!st.empty()) { // children before parents
            Frame f = st.back();
            st.pop_back();
            const TmpNode& t = nodes[f.node];
            if (t.left == 0xFFFFFFFFu) {
                collapse_leaf(dp[f.node], opt.cost_intersect, t.count, t.box.half_area());
            } else if (f.phase == 0) {
                st.push_back({f.node, 1});
                st.push_back({t.left, 0});
                st.push_back({t.right, 0});
            } else {
                collapse_inner(dp[f.node], dp[t.left], dp[t.right], t.box.half_area(), opt.cost_traverse8, opt.cost_intersect, max_leaf);
            }
        }
    }
    const HostTree tree{nodes, dp, ids};
    // A scene whose binary tree is one leaf gets a root node with that one child (slot 0 by rule 7), so that every walk starts at node 0.
    const bool one_leaf = nodes[root].left == 0xFFFFFFFFu;
    struct Item {
        uint32_t tmp, dev, depth;
    };
    std::vector<Item> stack;
    out.nodes.reserve(nodes.size() / 4 + 1);
    out.nodes.emplace_back();
    stack.push_back({root, 0, 1});
    const float root_area = nodes[root].box.half_area();
    double cost = 0.0;
    while (!stack.empty()) {
        Item it = stack.back();
        stack.pop_back();
        out.depth = std::max(out.depth, it.depth);
        const TmpNode& t = nodes[it.tmp];
        uint32_t ch[W8] = {root}, l, r;
        const int nch = one_leaf ? 1 : wide_children(tree, it.tmp, ch);
        Box cb[W8];
        for (int c = 0; c < nch; c++) cb[c] = nodes[ch[c]].box;
        int slot_child[W8];
        assign_slots(t.box, cb, nch, slot_child);
        uint32_t imask = 0, lmask = 0;
        for (int sl = 0; sl < W8; sl++) {
            if (slot_child[sl] < 0) continue;
            const uint32_t cn = ch[slot_child[sl]];
            if (!tree.inner(cn, l, r) || dp[cn].leaf) lmask |= 1u << sl;
            else imask |= 1u << sl;
        }
        const uint32_t child_base = (uint32_t)out.nodes.size();
        const int n_inner = __builtin_popcount(imask);
        for (int c = 0; c < n_inner; c++) out.nodes.emplace_back();
        const uint32_t tri_base = (uint32_t)out.tris.size();
        for (int sl = W8 - 1; sl >= 0; sl--) // inner children: visited in slot order
            if (imask & (1u << sl)) stack.push_back({ch[slot_child[sl]], child_base + (uint32_t)__builtin_popcount(imask & ((1u << sl) - 1u)), it.depth + 1});
        for (int sl = 0; sl < W8; sl++) {
            if (!(lmask & (1u << sl))) continue;
            const uint32_t cn = ch[slot_child[sl]];
            uint32_t gathered[RT_DEV_LEAF_STRIDE];
            const uint32_t ng = gather_leaf(tree, cn, tris_in, gathered);
            for (uint32_t x = 0; x < RT_DEV_LEAF_STRIDE; x++) out.tris.push_back(leaf_record(tris_in, gathered, ng, x));
            out.n_leaves++;
            if (root_area > 0) cost += opt.cost_intersect * ng * nodes[cn].box.half_area() / root_area;
        }
        if (root_area > 0) cost += opt.cost_traverse8 * t.box.half_area() / root_area;
        DevNode8& d = out.nodes[it.dev];
        quantise_node(d, imask, t.box, [&](int sl) { return slot_child[sl] < 0 ? (const Box*)nullptr : &cb[slot_child[sl]]; });
        d.child_base = one_leaf ? 0u : child_base;
        d.tri_base = tri_base;
        d.lmask = lmask;
        d._pad = 0;
    }
    out.sah_cost = cost;
}

} // namespace

void build_bvh(const BuildTri* tris_in, size_t n_in, const BvhBuildOptions& opt_in, BvhBuild& out) {
    out = BvhBuild();
    Builder b;
    b.opt = opt_in;
    if (b.opt.max_leaf < 1) b.opt.max_leaf = 1;
    if (b.opt.max_leaf > RT_DEV_LEAF_STRIDE) b.opt.max_leaf = RT_DEV_LEAF_STRIDE; // a leaf owns RT_DEV_LEAF_STRIDE triangle records
    if (b.opt.max_depth > RT_DEV_MAX_BVH_DEPTH) b.opt.max_depth = RT_DEV_MAX_BVH_DEPTH;
    int hw = (int)std::thread::hardware_concurrency();
    b.max_tasks = std::max(1, (b.opt.threads > 0 ? b.opt.threads : (hw > 0 ? hw : 1)) - 1);
    b.tris = tris_in;
    b.ids.reserve(n_in);
    b.boxes.resize(n_in);
    b.cent.resize(3 * n_in);
    for (size_t i = 0; i < n_in; i++) {
        const BuildTri& t = tris_in[i];
        if (!tri_finite(t.v0, t.v1, t.v2)) continue;
        b.boxes[i] = tri_box(t.v0, t.v1, t.v2);
        for (int a = 0; a < 3; a++) b.cent[3 * i + a] = b.boxes[i].centre(a);
        b.ids.push_back((uint32_t)i);
    }
    size_t n = b.ids.size();
    if (n == 0) return;
    if (opt_in.method == 1) { // PLOC on the host: the tree the device build makes (quality / structure reference)
        std::vector<TmpNode> pn;
        const uint32_t proot = build_ploc(b.boxes, b.cent, b.ids, pn, opt_in.ploc_radius);
        collapse8(pn, b.ids, (uint32_t)pn.size(), proot, tris_in, b.opt, b.opt.max_leaf, out);
        return;
    }
    b.nodes.resize(2 * n);
    uint32_t root = b.alloc();
    b.build(root, 0, (uint32_t)n, 0);
#if RT_BVH_REINSERT
    if (n > 8 && opt_in.reinsert) { // keep the top-down tree when the optimised one would exceed the depth the kernels' stacks are sized for
        std::vector<TmpNode> keep(b.nodes.begin(), b.nodes.begin() + b.next_node.load());
        const uint32_t keep_root = root;
        const uint32_t d = reinsertion_optimize(b.nodes, b.next_node.load(), root, RT_BVH_REINSERT_PASSES, RT_BVH_REINSERT_FRACTION);
        if (d > b.opt.max_depth) {
            std::copy(keep.begin(), keep.end(), b.nodes.begin());
            root = keep_root;
        }
    }
#endif

    collapse8(b.nodes, b.ids, b.next_node.load(), root, tris_in, b.opt, b.opt.max_leaf, out);
}

} // namespace rt
