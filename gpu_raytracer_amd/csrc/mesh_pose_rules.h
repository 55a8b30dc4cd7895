// mesh_pose_rules.h — the posed-mesh queries (rt_overlap_mesh, rt_sweep_mesh, include/rt_hip.h "Posed meshes"), stated once.
//
// Two pieces of code answer each: the kernels (posed_mesh.hip) and the host walk of tests/check_posed_mesh.cpp, which holds the walk
// of every posed triangle of a pose, with the shared word carried from lane to lane, to a brute force over all (mesh triangle,
// primitive) pairs before any kernel runs.  Both call what is here: the pose, the posed vertex, a lane's running best, the shared
// bound and the visitor that group_walk (group_walk.h) runs.  What is done WITH a posed triangle is not restated: it is
// overlap_triangle_rules.h (ot_query_valid, ot_sphere, ot_walk) and sweep_triangle_rules.h (st_query_valid, st_sphere, StVisit,
// st_answer_*), applied to the three posed vertices.  Every operation is one f32 rounding and nothing is fused (the build uses
// -ffp-contract=off), so numpy reproduces the bits (api.pose_triangles).
//
// ---- 1. The pose.  position p and rotation q = (x, y, z, w), which need not be of unit length.  R = ob_frame(q) of obb_rules.h,
// unchanged (its rule 1).  Vertex v of the mesh becomes
//   w_a = ((R_a0*v_0 + R_a1*v_1) + R_a2*v_2) + p_a
// that is ob_back followed by one addition: five roundings per component after R.  A pose is VALID iff p_0, p_1, p_2 are finite and
// ob_frame returns true (all four components of q finite, n finite and > 0).  An invalid pose is answered without a walk:
// rt_overlap_mesh gives pairs = 0 and first = 0xFFFFFFFF, rt_sweep_mesh the miss record - normal 0, tmax as given, axis NONE,
// triangle = prim_id = 0xFFFFFFFF, material 0.  A posed triangle of a valid pose is then judged by the triangle call's own rule
// (ot_query_valid, st_query_valid): a non-finite mesh vertex gives a non-finite posed vertex (a NaN or an infinity survives the
// products and sums, or 0 * inf makes a NaN) and that triangle touches nothing; a zero direction, a tmax that is NaN or <= 0 make
// every triangle of the pose a miss.
// Consequence, rotation = (0, 0, 0, w) with w finite and != 0, and p = 0: by obb_rules.h 6(a) R is the identity up to the signs
// of its zeros, ob_back gives (1*v_a + (+-0)*v_b) + (+-0)*v_c = v_a for finite v, and v_a + 0 = v_a: the posed vertices are the
// mesh's.  The one thing that can change is the sign of a zero (v_a = -0 may come out +0: -0 + +0 = +0), and as 6(a) argues no
// comparison of the two statements tells the zeros apart, t is t_in + 0.0f and a triangle's normal carries its own + 0.0f.  So
// with m = 1 rt_sweep_mesh returns rt_sweep_triangle's bytes (with triangle = 0 on a hit, 0xFFFFFFFF on a miss) and
// rt_overlap_mesh rt_overlap_triangle's count, for a mesh without a -0 component; with one, the only word that can differ is a
// zero component of a SPHERE's normal, whose sign st_sphere_normal takes from differences with the vertices (6(a)'s exception).
//
// ---- 2. The answers.  T_j = mesh triangle j posed; j < m.
//   overlap:  c_j = the number of primitives ot_sphere / ot_triangle hold for T_j (0 when ot_query_valid fails).
//             pairs = min(sum_j c_j, 0xFFFFFFFF), the sum in 64 bits;  first = the lowest j with c_j > 0, else 0xFFFFFFFF.
//             OV_ANY: pairs = 1 if some c_j > 0, else 0; triangles and primitives after the first touch need not be looked at.
//   sweep:    for T_j the candidates (bits of t, key) of sweep_triangle_rules.h rule 4, from (bits of tmax, 0), strict.  The pose's
//             answer is the least (bits of t, key, j) over the triangles that accepted a candidate: the record rt_sweep_triangle
//             gives T_j, with j in the word that is 0 there.  None: the miss record.
//
// ---- 3. One lane, several triangles.  A lane takes its triangles in increasing j and keeps ONE running order for all of them:
// a candidate of a later triangle is accepted only if it is strictly below the best of the earlier ones.  At equal (t, key) the
// earlier, lower j stays, which is the order of rule 2; a later triangle whose own first contact is later than the running best
// finds nothing, and would have lost anyway.  `own` is the lane's answer: (order, j, slot) of the last accepted candidate, j =
// 0xFFFFFFFF while there is none.  A lane HAS A HIT iff own.j was set by a candidate of its own.
//
// ---- 4. The shared bound (sweep).  The lanes that serve one pose share one 32-bit word, which starts at the bits of tmax.  A
// lane that accepts a candidate lowers the word to the bits of its t by an atomic minimum; these bits are those of t_in + 0.0f
// >= +0 or of a non-negative sphere time, so bit order is value order.  Before each of its triangles and at every node visit
// (MpSweepVisit::enter) a lane tightens its running order to
//   min(order, (word << 32) | 0xFFFFFFFF)                                                                       (mp_tighten)
// and StVisit::pass and the leaf limit read that order live.  Why the bytes do not depend on who wrote the word when:
//   - The word only ever holds tmax or the t of an accepted candidate of some triangle of the pose, so it is never below T, the
//     body's first contact time (the least t over all triangles); a stale read gives a larger word: a looser bound, nothing else.
//   - The tightened order is therefore >= (T, 0xFFFFFFFF) >= every candidate at time T, whatever its key.  sw_pass culls a slot only
//     if its entry time is STRICTLY later than the order's time and sb_over ends a test only if t_in is STRICTLY later, and
//     acceptance is c < order on the full 64 bits; a candidate at a time equal to the shared one is still reached, still
//     evaluated in full and still accepted unless the lane already holds a lower (t, key).
//   - So a lane whose true answer (rule 3, without any sharing) has t <= T - then t = T - reports exactly that answer: every
//     candidate at time T of each of its triangles is seen in the same order relation as without the word.
//   - Every other lane's true answer is later than T.  Whatever it reports - a candidate later than T that it met before the word
//     fell, or nothing - its order has a time > T or it has no hit, and it loses the reduction to a lane of the first kind, of
//     which there is at least one when anything is hit at all.  If nothing is hit the word stays tmax and nothing is culled by it.
// The bytes are deterministic; node visits and triangle tests are not (they depend on when the word fell).
// The tightened order is NOT the lane's answer: `own` keeps the order of the lane's own last accepted candidate apart from it.
//
// ---- 5. The shared stop (overlap, OV_ANY).  One flag per pose; a lane that finds a touch raises it, and a lane looks at it
// before each of its triangles.  pairs is 1 iff some lane found a touch, which the flag's timing cannot change.
//
// ---- 6. The reduction over the lanes of a pose: the minimum of own.order over the lanes with a hit (no hit: all ones), then the
// minimum j among the lanes that hold that order.  Each j belongs to one lane, so the winner is unique; it poses its triangle j
// again and writes st_answer_triangle / st_answer_sphere with j in word 5.  For the overlap: the sum of the lanes' 64-bit sums and
// the minimum of their lowest j.
#ifndef RT_MESH_POSE_RULES_H
#define RT_MESH_POSE_RULES_H

#include "obb_rules.h"
#include "sweep_triangle_rules.h"

namespace rt {

constexpr uint32_t MP_NONE = 0xFFFFFFFFu;

// rule 1
struct MpPose {
    float R[9], p[3];
};
RT_RULE bool mp_pose(const float position[3], const float rotation[4], MpPose& P) {
    P.p[0] = position[0], P.p[1] = position[1], P.p[2] = position[2];
    const bool turn = ob_frame(rotation, P.R);
    return turn && ov_finite(position[0]) && ov_finite(position[1]) && ov_finite(position[2]);
}
RT_RULE void mp_vertex(const MpPose& P, const float v[3], float w[3]) {
    float r[3];
    ob_back(P.R, v, r);
    RT_CP_UNROLL
    for (int a = 0; a < 3; a++) w[a] = r[a] + P.p[a];
}

// rule 3: a lane's answer
struct MpBest {
    uint64_t order; // of the lane's own last accepted candidate; sw_start(tmax) while there is none
    uint32_t j, slot; // its mesh triangle (MP_NONE: no hit) and its record in DevScene::tris or its sphere index
};
RT_RULE void mp_best_init(MpBest& own, float tmax) { own.order = sw_start(tmax), own.j = own.slot = MP_NONE; }

// rule 4.  A Shared supplies the pose's word: uint32_t read() and void lower(uint32_t bits), an atomic minimum.  MpNoShare is the
// variant without sharing: the word reads as all ones, which tightens nothing.
struct MpNoShare {
    RT_RULE uint32_t read() const { return 0xFFFFFFFFu; }
    RT_RULE void lower(uint32_t) {}
};
RT_RULE uint64_t mp_tighten(uint64_t order, uint32_t word) {
    const uint64_t bound = ((uint64_t)word << 32) | 0xFFFFFFFFull;
    return bound < order ? bound : order;
}
// an accepted candidate `c` (it is best.order already) of triangle j
template <class Shared>
RT_RULE void mp_accept(MpBest& own, Shared& sh, uint64_t c, uint32_t j, uint32_t slot) {
    own.order = c, own.j = j, own.slot = slot;
    sh.lower((uint32_t)(c >> 32));
}
// StVisit for triangle j of a lane: the bound tightened at every node, an accepted candidate recorded and published
template <class Shared>
struct MpSweepVisit {
    StVisit v;
    Shared& sh;
    MpBest& own;
    uint32_t j;

    RT_RULE uint32_t enter(const uint32_t w[20]) {
        v.best.order = mp_tighten(v.best.order, sh.read());
        return v.enter(w);
    }
    RT_RULE uint32_t pass(uint32_t occupied) const { return v.pass(occupied); }
    template <class Access>
    RT_RULE bool leaf(Access& acc, uint32_t slot, const float rec[9], const uint32_t ids[3]) {
        const uint64_t before = v.best.order;
        (void)v.leaf(acc, slot, rec, ids);
        if (v.best.order < before) mp_accept(own, sh, v.best.order, j, slot);
        return false;
    }
};
// The walk of posed triangle j (q, valid by st_query_valid) after its spheres: st_walk with the visitor above.  `best` is the lane's
// running order (rule 3), tightened; `own` its answer.
template <class Access, class Shared>
RT_RULE void mp_sweep_walk(Access& acc, uint32_t n_nodes, const StQuery& q, uint32_t j, CpBest& best, MpBest& own, Shared& sh) {
    MpSweepVisit<Shared> v{StVisit{q, cp_p_max(q.b.c), {1.0f / q.b.d[0], 1.0f / q.b.d[1], 1.0f / q.b.d[2]}, {}, sw_octant(q.b.d), 0u, best}, sh, own, j};
    group_walk(acc, n_nodes, v);
}
// a sphere's candidate c = cp_order(st_sphere(..), s) for triangle j, before the walk
template <class Shared>
RT_RULE void mp_sweep_sphere(uint64_t c, uint32_t s, uint32_t j, CpBest& best, MpBest& own, Shared& sh) {
    if (c < best.order) best.order = c, best.slot = s, mp_accept(own, sh, c, j, s);
}

// rule 6: the order a lane brings to the reduction
RT_RULE uint64_t mp_reduce_order(const MpBest& own) { return own.j != MP_NONE ? own.order : ~0ull; }
// the miss record of a pose, and the winner's record with its triangle
RT_RULE void mp_answer_miss(float tmax, uint32_t out[8]) {
    sb_answer_miss(tmax, out);
    out[5] = MP_NONE;
}

} // namespace rt
#endif
