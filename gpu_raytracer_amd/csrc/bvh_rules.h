// bvh_rules.h — the rules that turn triangles into the 8-wide quantised tree, stated once.
//
// Three pieces of code make or remake that tree: the host build (bvh_builder.cpp: binned SAH or PLOC, then the collapse), the device
// build (device_build.hip: PLOC and the collapse in kernels) and the refit (refit.hip).  The host's PLOC tree and the device's are
// byte-identical, and a refit with unchanged positions reproduces the nodes: every expression that decides a bit of the output is
// here, and the three callers differ only in how they store boxes and binary nodes and in what order they run.  Plain inline
// functions, host and device under hipcc, host only under any other compiler (tests build the host builder with g++).
// Operation order and precision are part of the rules: f32 where it says float, the quantisation in double.
#ifndef RT_BVH_RULES_H
#define RT_BVH_RULES_H

#include <cmath>
#include <cstdint>

#include "bvh_builder.h"

#ifdef __HIPCC__
#define RT_RULE __host__ __device__ inline
#else
#define RT_RULE inline
#endif

namespace rt {

// min / max.  Host code has always spelled them std::min / std::max (b < a ? b : a) and device code fminf / fmaxf; each side keeps
// its spelling here.  The two give the same bits whenever neither operand is NaN, and no NaN reaches a box: triangles with a
// non-finite coordinate are dropped (tri_finite) before any rule sees them.  Every min / max below goes through these four.
#ifdef __HIP_DEVICE_COMPILE__
RT_RULE float rule_min(float a, float b) { return fminf(a, b); }
RT_RULE float rule_max(float a, float b) { return fmaxf(a, b); }
RT_RULE double rule_min(double a, double b) { return fmin(a, b); }
RT_RULE double rule_max(double a, double b) { return fmax(a, b); }
#else
RT_RULE float rule_min(float a, float b) { return b < a ? b : a; }
RT_RULE float rule_max(float a, float b) { return a < b ? b : a; }
RT_RULE double rule_min(double a, double b) { return b < a ? b : a; }
RT_RULE double rule_max(double a, double b) { return a < b ? b : a; }
#endif

struct Box {
    float mn[3], mx[3];
    RT_RULE void reset() {
        for (int a = 0; a < 3; a++) mn[a] = INFINITY, mx[a] = -INFINITY;
    }
    RT_RULE void grow(const Box& b) {
        for (int a = 0; a < 3; a++) mn[a] = rule_min(mn[a], b.mn[a]), mx[a] = rule_max(mx[a], b.mx[a]);
    }
    RT_RULE void grow(const float p[3]) {
        for (int a = 0; a < 3; a++) mn[a] = rule_min(mn[a], p[a]), mx[a] = rule_max(mx[a], p[a]);
    }
    RT_RULE float centre(int a) const { return 0.5f * mn[a] + 0.5f * mx[a]; }
    RT_RULE float half_area() const { // ---- 3. half the surface area; 0 for an empty or NaN box
        const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
        if (!(dx >= 0.0f) || !(dy >= 0.0f) || !(dz >= 0.0f)) return 0.0f;
        return dx * dy + dy * dz + dz * dx;
    }
};

// ---- 1. a triangle: dropped unless all nine coordinates are finite (Möller–Trumbore can never accept it); its box; its centroid is
// the box's centre
RT_RULE bool tri_finite(const float v0[3], const float v1[3], const float v2[3]) {
    bool finite = true;
    for (int a = 0; a < 3; a++) finite = finite && std::isfinite(v0[a]) && std::isfinite(v1[a]) && std::isfinite(v2[a]);
    return finite;
}
RT_RULE Box tri_box(const float v0[3], const float v1[3], const float v2[3]) {
    Box b;
    for (int a = 0; a < 3; a++) {
        b.mn[a] = rule_min(rule_min(v0[a], v1[a]), v2[a]);
        b.mx[a] = rule_max(rule_max(v0[a], v1[a]), v2[a]);
    }
    return b;
}

// ---- 2. Morton code of a centroid within the bounds [lo, hi] of all centroids: 21 bits per axis spread to every third bit, x highest
RT_RULE uint64_t morton21(float x) { // x in [0, 1]
    uint64_t v = (uint64_t)(uint32_t)rule_min(rule_max(x * 2097152.0f, 0.0f), 2097151.0f);
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}
RT_RULE uint64_t morton63(const float c[3], const float lo[3], const float hi[3]) {
    uint64_t code = 0;
    for (int a = 0; a < 3; a++) {
        const float inv = hi[a] > lo[a] ? 1.0f / (hi[a] - lo[a]) : 0.0f;
        code |= morton21((c[a] - lo[a]) * inv) << (2 - a);
    }
    return code;
}

// ---- 4. PLOC (Meister, Bittner, "Parallel Locally-Ordered Clustering for Bounding Volume Hierarchy Construction", 2018): the clusters
// lie along the Morton curve; every round each finds its nearest neighbour (area of the union, rule 3: Box::half_area) within `radius`
// positions, and the pairs that chose each other merge.  Degenerate input stalls the pairing: with coincident triangles every
// cluster's nearest neighbour is the first of its window, in a chain of growing triangles it is the predecessor - one mutual pair per
// round, and a tree as deep as the input is long.  A round that merges less than a sixteenth of the clusters therefore escalates, for
// the rest of the build: level 1 prefers position i ^ 1 among EQUAL areas (coincident triangles then pair up perfectly), level 2
// pairs i and i ^ 1 outright.  Ordinary scenes never leave level 0.  (Level 1's rule at level 0 was measured: +5 % node visits on
// the sponza-like scene, whose tessellated walls are full of exact ties.)
template <class UnionArea> // union_area(j): half area of the union of cluster i's box and cluster j's
RT_RULE uint32_t ploc_nearest(uint32_t i, uint32_t m, uint32_t radius, uint32_t level, UnionArea union_area) {
    const uint32_t buddy = i ^ 1u;
    if (level == 2u) return buddy < m ? buddy : i;
    float best = INFINITY;
    uint32_t bj = i;
    if (level == 1u && buddy < m) best = union_area(buddy), bj = buddy;
    const uint32_t lo = i > radius ? i - radius : 0u, hi = m - 1u < i + radius ? m - 1u : i + radius;
    for (uint32_t j = lo; j <= hi; j++) { // first best: the lower position wins ties
        if (j == i) continue;
        const float a = union_area(j);
        if (a < best) best = a, bj = j;
    }
    return bj;
}
// role of cluster i this round: 0 stays, 1 merges with nn[i] (it is the lower of the pair and carries the new node), 2 disappears
RT_RULE uint32_t ploc_role(const uint32_t* nn, uint32_t i) {
    const uint32_t j = nn[i];
    if (j == i || nn[j] != i) return 0u;
    return i < j ? 1u : 2u;
}
RT_RULE bool ploc_escalates(uint32_t merged, uint32_t m, uint32_t level) { return merged < m / 16u && level < 2u; }

// ---- 5. The collapse program.  Which binary nodes become wide nodes, which are absorbed, which subtrees become one leaf is chosen by
// dynamic programming over the binary tree (minimum expected cost): c[k-1] = cheapest cost of a subtree when it may occupy at most k
// child slots of its wide parent: k = 1: either one leaf (<= max_leaf triangles, whatever their order: the leaf gathers them) or a
// wide node of its own, area * cost_traverse8 + the best split of 8 slots between its two children; k > 1: the best split of k slots
// between its children, or k - 1 slots.  (Round 1's 4-wide collapse used the same program with four slots; the greedy "open the child
// with the largest area" rule it replaced was 0.8-1.5 % worse.)  Next to the costs the record carries what the subtree will produce,
// so that a builder can know where everything goes before it writes anything.
constexpr int W8 = 8;
struct CollapseRec {
    float c[W8];
    uint8_t split[W8]; // [k-1]: slots for the left child when k are distributed (0: use k - 1); [0]: the split of 8 when the node is a wide node
    uint32_t count;    // triangles below (saturating well above max_leaf)
    uint32_t leaf;     // k = 1: the subtree is cheapest as a single leaf
    uint32_t wn[W8];   // [k-1]: wide nodes the subtree produces when it gets at most k child slots of its parent
    uint32_t ln[W8];   // [k-1]: leaves it produces
};
// effective number of slots the program uses when `k` are offered
RT_RULE int effective_slots(const CollapseRec& d, int k) {
    while (k > 1 && d.split[k - 1] == 0) k--;
    return k;
}
RT_RULE void collapse_leaf(CollapseRec& d, float cost_intersect, uint32_t count, float area) { // a leaf of the binary tree
    const float lc = cost_intersect * (float)count * area;
    for (int k = 0; k < W8; k++) d.c[k] = lc, d.split[k] = 0, d.wn[k] = 0u, d.ln[k] = 1u;
    d.count = count;
    d.leaf = 1;
}
RT_RULE void collapse_inner(CollapseRec& d, const CollapseRec& dl, const CollapseRec& dr, float area, float cost_traverse8, float cost_intersect, uint32_t max_leaf) {
    float dist[W8 + 1];
    uint8_t arg[W8 + 1];
    for (int k = 0; k <= W8; k++) dist[k] = INFINITY, arg[k] = 0;
    for (int k = 2; k <= W8; k++)
        for (int s = 1; s < k; s++) {
            const float v = dl.c[s - 1] + dr.c[k - s - 1];
            if (v < dist[k]) dist[k] = v, arg[k] = (uint8_t)s;
        }
    const float wide = cost_traverse8 * area + dist[W8];
    d.count = dl.count + dr.count < (1u << 20) ? dl.count + dr.count : 1u << 20;
    const float leafc = d.count <= max_leaf ? cost_intersect * (float)d.count * area : INFINITY;
    // Finite coordinates whose box area overflows f32 (~1e19 and beyond) make every cost inf or NaN: no `v < dist` above succeeds and
    // arg stays 0, which is not a split.  The rule then is explicit: a leaf only when the count allows it, else a wide
    // node split 1 : 7 - a poor tree, but a valid one.
    if (arg[W8] == 0) arg[W8] = 1;
    d.leaf = (d.count <= max_leaf && !(wide < leafc)) ? 1u : 0u;
    d.c[0] = rule_min(leafc, wide);
    d.split[0] = arg[W8];
    for (int k = 2; k <= W8; k++) {
        if (dist[k] < d.c[k - 2]) d.c[k - 1] = dist[k], d.split[k - 1] = arg[k];
        else d.c[k - 1] = d.c[k - 2], d.split[k - 1] = 0;
    }
    // what the subtree will produce: as one child (k = 1) a leaf, or a wide node whose 8 slots are split s0 : 8 - s0 ...
    {
        const int s0 = d.split[0];
        d.wn[0] = d.leaf ? 0u : 1u + dl.wn[s0 - 1] + dr.wn[W8 - s0 - 1];
        d.ln[0] = d.leaf ? 1u : dl.ln[s0 - 1] + dr.ln[W8 - s0 - 1];
    }
    for (int k = 2; k <= W8; k++) { // ... with k slots: through the split the program chose for the effective k
        const int kk = effective_slots(d, k);
        if (kk > 1) {
            const int sl = d.split[kk - 1];
            d.wn[k - 1] = dl.wn[sl - 1] + dr.wn[kk - sl - 1];
            d.ln[k - 1] = dl.ln[sl - 1] + dr.ln[kk - sl - 1];
        } else {
            d.wn[k - 1] = d.wn[0];
            d.ln[k - 1] = d.ln[0];
        }
    }
}

// A builder shows its binary tree to rules 6 and 9 through a `Tree`:
//   bool inner(node, l, r) const            the node's two children, false for a leaf of the binary tree
//   const CollapseRec& rec(node) const      its collapse record
//   uint32_t leaf_tris(node, out, n) const  appends a binary leaf's triangles (indices into the build's input) to out[n..], up to
//                                           RT_DEV_LEAF_STRIDE in all; returns the new n

// ---- 6. Children of the wide node made of binary node `bin` (an inner one): its subtree in at most 8 slots, through the program's
// splits, left before right.  A child is a leaf of the wide tree when it is a leaf of the binary tree or its record says `leaf`.
template <class Tree>
RT_RULE int wide_children(const Tree& t, uint32_t bin, uint32_t ch[W8]) {
    uint32_t st_node[2 * W8], l, r;
    int st_k[2 * W8], sp = 0, nch = 0;
    t.inner(bin, l, r);
    const int s0 = t.rec(bin).split[0];
    st_node[sp] = r, st_k[sp++] = W8 - s0;
    st_node[sp] = l, st_k[sp++] = s0;
    while (sp > 0) {
        const uint32_t node = st_node[--sp];
        bool is_child = true;
        if (t.inner(node, l, r)) {
            const int k = effective_slots(t.rec(node), st_k[sp]);
            if (k > 1 && sp + 2 <= 2 * W8) {
                const int s = t.rec(node).split[k - 1];
                st_node[sp] = r, st_k[sp++] = k - s;
                st_node[sp] = l, st_k[sp++] = s;
                is_child = false;
            }
        }
        if (is_child && nch < W8) ch[nch++] = node;
    }
    return nch;
}

// ---- 7. Slot assignment: slot s lies toward the corner (s & 1 ? +x : -x, s & 2 ? +y : -y, s & 4 ? +z : -z) of the node.  Greedy:
// repeatedly give the (child, slot) pair with the largest projection of the child's centre offset on the slot's diagonal.
// slot_child[s] = the child in slot s, -1 for an empty slot.
RT_RULE void assign_slots(const Box& parent, const Box* child, int nch, int slot_child[W8]) {
    float score[W8][W8];
    for (int c = 0; c < nch; c++) {
        float off[3];
        for (int a = 0; a < 3; a++) off[a] = child[c].centre(a) - parent.centre(a);
        for (int sl = 0; sl < W8; sl++) score[c][sl] = (sl & 1 ? off[0] : -off[0]) + (sl & 2 ? off[1] : -off[1]) + (sl & 4 ? off[2] : -off[2]);
    }
    bool done[W8];
    for (int sl = 0; sl < W8; sl++) slot_child[sl] = -1, done[sl] = false;
    for (int round = 0; round < nch; round++) {
        int bc = -1, bs = -1;
        float best = -INFINITY;
        for (int c = 0; c < nch; c++) {
            if (done[c]) continue;
            for (int sl = 0; sl < W8; sl++)
                if (slot_child[sl] < 0 && score[c][sl] > best) best = score[c][sl], bc = c, bs = sl;
        }
        if (bc < 0) { // only NaN scores are left (degenerate boxes): the first child and the first slot still free
            for (int c = 0; c < nch && bc < 0; c++)
                if (!done[c]) bc = c;
            for (int sl = 0; sl < W8 && bs < 0; sl++)
                if (slot_child[sl] < 0) bs = sl;
        }
        slot_child[bs] = bc;
        done[bc] = true;
    }
}

// ---- 8. Node quantisation: org, qlo, qhi and ex_imask of `d` from the node's box and its children's by slot: child_of_slot(s) is
// the box of the child in slot s (const Box*), null for an empty slot.
// Per axis a power-of-two grid of 255 steps over the box, its exponent clamped to [1, 254] before the bias (so [-126, 127] after);
// planes rounded outward and corrected until they contain the box as the kernels decode them; empty slots inverted (lo 255, hi 0): such
// a slot can only be entered when the float evaluation cannot tell 255 grid steps apart (degenerate node, ray origin ~1e8 grid steps
// away), and the traversal masks the hit bits with imask | lmask, so it is never followed.
template <class ChildOfSlot>
RT_RULE void quantise_node(DevNode8& d, uint32_t imask, const Box& parent, ChildOfSlot child_of_slot) {
    uint32_t ex[3];
    for (int a = 0; a < 3; a++) {
        d.org[a] = parent.mn[a];
        const double org = (double)d.org[a], extent = (double)parent.mx[a] - (double)parent.mn[a];
        int e = 1;
        if (extent > 0.0) {
            int fe;
            (void)std::frexp(extent / 255.0, &fe);
            e = fe + 127;
            if (e < 1) e = 1;
            if (e > 254) e = 254;
        }
        ex[a] = (uint32_t)(e - 127) & 0xFFu;
        const double scale = std::ldexp(1.0, e - 127);
        for (int h = 0; h < 2; h++) {
            uint32_t lo_word = 0, hi_word = 0;
            for (int i = 0; i < 4; i++) {
                const Box* child = child_of_slot(4 * h + i);
                uint32_t qlo = 255, qhi = 0;
                if (child) {
                    const double bmn = (double)child->mn[a], bmx = (double)child->mx[a];
                    double lo = std::floor((bmn - org) / scale);
                    double hi = std::ceil((bmx - org) / scale);
                    lo = rule_min(rule_max(lo, 0.0), 255.0);
                    hi = rule_min(rule_max(hi, 0.0), 255.0);
                    while (lo > 0.0 && org + lo * scale > bmn) lo -= 1.0;
                    while (hi < 255.0 && org + hi * scale < bmx) hi += 1.0;
                    qlo = (uint32_t)lo;
                    qhi = (uint32_t)hi;
                }
                lo_word |= qlo << (8 * i);
                hi_word |= qhi << (8 * i);
            }
            d.qlo[a][h] = lo_word;
            d.qhi[a][h] = hi_word;
        }
    }
    d.ex_imask = ex[0] | (ex[1] << 8) | (ex[2] << 16) | (imask << 24);
}

// ---- 9. Leaf records.  The position part of a record: e1 / e2 are the same f32 subtractions the reference does per test
// (shader/src/intersection.rs:104-105), done once; a refit redoes exactly these.
RT_RULE void put_positions(const float v0[3], const float v1[3], const float v2[3], DevTri* o) {
    for (int a = 0; a < 3; a++) {
        o->v0[a] = v0[a];
        o->e1[a] = v1[a] - v0[a];
        o->e2[a] = v2[a] - v0[a];
    }
}
RT_RULE void put_tri(const BuildTri& t, DevTri* o) {
    put_positions(t.v0, t.v1, t.v2, o);
    o->material_id = t.material_id;
    o->prim_id = t.prim_id;
    o->leaf_count = 0;
}
// The triangles of a leaf of the wide tree - all below `node` - ordered by the caller's triangle index (the tie rule of the closest
// hit does not need the order; it makes the arrays unique).  Returns their number.
template <class Tree>
RT_RULE uint32_t gather_leaf(const Tree& t, uint32_t node, const BuildTri* tris_in, uint32_t gathered[RT_DEV_LEAF_STRIDE]) {
    uint32_t ng = 0, todo[2 * RT_DEV_LEAF_STRIDE + 2], l, r;
    int nt = 0;
    todo[nt++] = node;
    while (nt > 0) {
        const uint32_t u = todo[--nt];
        if (!t.inner(u, l, r)) {
            ng = t.leaf_tris(u, gathered, ng);
        } else if (nt + 2 <= (int)(2 * RT_DEV_LEAF_STRIDE + 2)) {
            todo[nt++] = l;
            todo[nt++] = r;
        }
    }
    for (uint32_t x = 1; x < ng; x++) // insertion sort
        for (uint32_t y = x; y > 0 && tris_in[gathered[y]].prim_id < tris_in[gathered[y - 1]].prim_id; y--) {
            const uint32_t tmp = gathered[y];
            gathered[y] = gathered[y - 1];
            gathered[y - 1] = tmp;
        }
    return ng;
}
// Record x of the RT_DEV_LEAF_STRIDE a leaf owns: its x-th triangle or a blank, the leaf's length in the first.
RT_RULE DevTri leaf_record(const BuildTri* tris_in, const uint32_t* gathered, uint32_t ng, uint32_t x) {
    DevTri t;
    if (x < ng) put_tri(tris_in[gathered[x]], &t);
    else {
        for (int a = 0; a < 3; a++) t.v0[a] = t.e1[a] = t.e2[a] = 0.0f;
        t.material_id = t.prim_id = t.leaf_count = 0;
    }
    if (x == 0) t.leaf_count = ng;
    return t;
}

} // namespace rt
#endif
