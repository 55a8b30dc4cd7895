"""The triangle query's statement (include/rt_hip.h "Triangle queries", csrc/overlap_triangle_rules.h) in numpy, and the triangles the
tests ask about.

touching() evaluates the float32 statement for every query triangle against every triangle record and sphere of a scene - every numpy
operation is one f32 rounding, in the header's order - and overlap_all() turns it into the ids and counts rt_overlap_triangle must
return, byte for byte; first_k gives the statement at a smaller max_prims.  Test 1 (the bounds) is evaluated on all pairs and the 23
axes on the pairs that pass it only: the answer is a conjunction, and almost every pair ends at the bounds.  gaps() is the same
statement in float64 on the exact edges with a signed gap per pair, which the float32 statement is held to, and pierces() an
independent predicate the float64 statement is held to.  Helpers, no tests."""
import numpy as np

import closest_point_cases as cc
import overlap_cases as oc

F32 = np.float32
F64 = np.float64
OVERLAP_MAX = oc.OVERLAP_MAX
PRIM_MISS = cc.PRIM_MISS
SPHERE_FLAG = cc.SPHERE_FLAG

# The smallest k of the 1 / 1.5 / 2 / 3 / 5 / 7 x 10^e grid for which, on every pair of the batch, "touches in f32" implies gap64 <=
# k x diagonal and "does not" implies gap64 >= -k x diagonal (test_overlap_triangle_abi.py measures it again, prints it and asserts
# at 2 x K).  0: no pair of the batch disagrees in sign at all.
K_MEASURED = {"soup": 0.0, "cornell12": 0.0}


def make_triangles(v0, v1, v2):
    """(N, 12) float32 rt_query_triangle records: v0 0 v1 0 v2 0."""
    a = np.asarray(v0, F32).reshape(-1, 3)
    out = np.zeros((len(a), 12), F32)
    out[:, 0:3], out[:, 4:7], out[:, 8:11] = a, np.asarray(v1, F32).reshape(-1, 3), np.asarray(v2, F32).reshape(-1, 3)
    return out


def vertices(tris):
    return tris[:, 0:3], tris[:, 4:7], tris[:, 8:11]


def valid(tris):
    """Which queries are walked: all nine components finite."""
    with np.errstate(all="ignore"):
        return np.isfinite(tris[:, 0:3]).all(1) & np.isfinite(tris[:, 4:7]).all(1) & np.isfinite(tris[:, 8:11]).all(1)


def bounds(tris):
    q0, q1, q2 = vertices(tris)
    return np.fmin(np.fmin(q0, q1), q2), np.fmax(np.fmax(q0, q1), q2)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def axes(u1, u2, f1, f2):
    """The 23 axes of a pair, each (P, 3), in the dtype of the arrays: nS, nQ, the nine cross(u_i, f_j), cross(nQ, u_i), cross(nS, f_j),
    cross(nS, u_i), cross(nQ, f_j)."""
    u, f = (u1, u2, u2 - u1), (f1, f2, f2 - f1)
    ns, nq = _cross(f1, f2), _cross(u1, u2)
    out = [ns, nq] + [_cross(ui, fj) for ui in u for fj in f]
    out += [_cross(nq, ui) for ui in u] + [_cross(ns, fj) for fj in f] + [_cross(ns, ui) for ui in u] + [_cross(nq, fj) for fj in f]
    return out


def _project(L, a, u1, u2):
    """-> (min pS, max pS, min pQ, max pQ, the sum that must not be a NaN), each (P,)."""
    s0, s1, s2, t1, t2 = cc._dot(L, a[0]), cc._dot(L, a[1]), cc._dot(L, a[2]), cc._dot(L, u1), cc._dot(L, u2)
    zero = s0.dtype.type(0)
    return (np.fmin(np.fmin(s0, s1), s2), np.fmax(np.fmax(s0, s1), s2), np.fmin(np.fmin(zero, t1), t2), np.fmax(np.fmax(zero, t1), t2),
            ((s0 + s1) + s2) + (t1 + t2))


def _pairs(s, q0, q1, q2, rows, cols, with_gap):
    """Test 2 on the pairs (rows[i], cols[i]): s = (s0, s1, s2) per record.  -> touch (P,) bool and, with_gap, the largest scaled
    separation over the axes with |L| > 0 (-inf where there is none)."""
    with np.errstate(all="ignore"):
        p0 = q0[rows]
        u1, u2 = q1[rows] - p0, q2[rows] - p0
        a = [sk[cols] - p0 for sk in s]
        f1, f2 = s[1][cols] - s[0][cols], s[2][cols] - s[0][cols]
        touch = np.ones(len(rows), bool)
        gap = np.full(len(rows), -np.inf) if with_gap else None
        for L in axes(u1, u2, f1, f2):
            smin, smax, qmin, qmax, total = _project(L, a, u1, u2)
            touch &= (smin <= qmax) & (smax >= qmin) & (total == total)
            if with_gap:
                length = np.sqrt(cc._dot(L, L))
                sep = np.maximum(smin - qmax, qmin - smax) / np.where(length > 0, length, 1.0)
                gap = np.where(length > 0, np.maximum(gap, sep), gap)
        return touch, gap


def _records(scene, dtype):
    """s0, s1, s2 per record as the statement has them.  float32: v0, v0 + e1, v0 + e2 on the stored differences (so the edges f are
    s_k - s_0 only up to a rounding: the f32 pairs below take e1, e2 themselves); float64: the exact vertices."""
    with np.errstate(all="ignore"):
        v0, e1, e2, _ = cc.records(scene, dtype)
        return v0, e1, e2, (v0, v0 + e1, v0 + e2)


def _sphere_arrays(scene, dtype):
    sph = scene.spheres
    return np.ascontiguousarray(sph["center"], F32).reshape(-1, 3).astype(dtype), sph["radius"].astype(F32).astype(dtype)


def _sphere_terms(centre, radius, q0, q1, q2):
    """-> near2, far2, rr, each (N, s)."""
    with np.errstate(all="ignore"):
        near2 = cc.triangle_candidates(q0, q1 - q0, q2 - q0, centre)[0].T
        far2 = None
        for q in (q0, q1, q2):
            d = q[:, None, :] - centre[None]
            far2 = cc._dot(d, d) if far2 is None else np.fmax(far2, cc._dot(d, d))
        return near2, far2, np.broadcast_to((radius * radius)[None], near2.shape)


def touching(scene, tris):
    """(N, 12) float32 query triangles -> (N, n_spheres + n_triangles) bool in key order: the spheres' columns, then the triangles'."""
    tris = np.ascontiguousarray(tris, F32)
    q0, q1, q2 = vertices(tris)
    ok = valid(tris)
    centre, radius = _sphere_arrays(scene, F32)
    v0, e1, e2, s = _records(scene, F32)
    out = np.zeros((len(tris), len(centre) + len(v0)), bool)
    with np.errstate(all="ignore"):
        if len(centre) and len(tris):
            near2, far2, rr = _sphere_terms(centre, radius, q0, q1, q2)
            out[:, :len(centre)] = (near2 <= rr) & (far2 >= rr)
        if len(v0) and len(tris):
            qlo, qhi = bounds(tris)
            smin, smax = np.fmin(np.fmin(s[0], s[1]), s[2]), np.fmax(np.fmax(s[0], s[1]), s[2])
            finite = (np.abs(np.stack(s)) <= oc.FLT_MAX).all((0, 2))
            box = finite[None] & ok[:, None]
            for ax in range(3):
                box &= (smin[None, :, ax] <= qhi[:, None, ax]) & (smax[None, :, ax] >= qlo[:, None, ax])
            rows, cols = np.nonzero(box)
            p0 = q0[rows]
            u1, u2 = q1[rows] - p0, q2[rows] - p0
            a = [sk[cols] - p0 for sk in s]
            touch = np.ones(len(rows), bool)
            for L in axes(u1, u2, e1[cols], e2[cols]):
                lo_s, hi_s, lo_q, hi_q, total = _project(L, a, u1, u2)
                touch &= (lo_s <= hi_q) & (hi_s >= lo_q) & (total == total)
            out[rows[touch], len(centre) + cols[touch]] = True
    return out & ok[:, None]


def overlap_all(scene, tris, k=OVERLAP_MAX, touch=None):
    """-> ids (N, k) uint32 (ascending key, then PRIM_MISS), listed counts (N,) uint32 = min(total, k), total counts (N,) uint32."""
    return oc.overlap_all(scene, None, k, touching(scene, tris) if touch is None else touch)


first_k = oc.first_k


# -- the float64 statement with a gap ---------------------------------------------------------------------------------------------
def gaps(scene, tris, near=None):
    """The statement in float64 on the exact vertices -> (touch (N, cols) bool, gap (N, cols) float64, evaluated (N, cols) bool).
    A triangle's gap is the largest, over the three coordinate axes of test 1 and the 23 axes of test 2 with |L| > 0, of
    max(min pS - max pQ, min pQ - max pS) / |L|: the pair touches only if it is <= 0, and a positive gap is a distance by which one
    axis separates the two.  The 23 axes are evaluated where the coordinate axes' gap is <= near (default: a thousandth of the
    scene's diagonal) - `evaluated`; elsewhere the pair's bounds are clearly apart, it does not touch, and its gap is the
    coordinate axes' alone, a lower bound of the largest.  A sphere's gap is max(sqrt(near2) - R, R - sqrt(far2)).  Ordinary
    input: finite queries and records."""
    t = np.ascontiguousarray(tris, F32).astype(F64)
    q0, q1, q2 = vertices(t)
    centre, radius = _sphere_arrays(scene, F64)
    _, _, _, s = _records(scene, F64)
    near = 1e-3 * cc.diagonal(scene) if near is None else near
    cols = len(centre) + len(s[0])
    touch, gap, evaluated = np.zeros((len(t), cols), bool), np.zeros((len(t), cols), F64), np.zeros((len(t), cols), bool)
    if len(centre):
        near2, far2, rr = _sphere_terms(centre, radius, q0, q1, q2)
        touch[:, :len(centre)] = (near2 <= rr) & (far2 >= rr)
        gap[:, :len(centre)] = np.maximum(np.sqrt(near2) - radius[None], radius[None] - np.sqrt(far2))
        evaluated[:, :len(centre)] = True
    if len(s[0]):
        qlo, qhi = bounds(t)
        smin, smax = np.minimum(np.minimum(s[0], s[1]), s[2]), np.maximum(np.maximum(s[0], s[1]), s[2])
        cg = np.full((len(t), len(smin)), -np.inf)
        for ax in range(3):
            cg = np.maximum(cg, np.maximum(smin[None, :, ax] - qhi[:, None, ax], qlo[:, None, ax] - smax[None, :, ax]))
        rows, cl = np.nonzero(cg <= near)
        pair_touch, pair_gap = _pairs(s, q0, q1, q2, rows, cl, True)
        g = cg.copy()
        g[rows, cl] = np.maximum(cg[rows, cl], pair_gap)
        gap[:, len(centre):] = g
        touch[rows, len(centre) + cl] = pair_touch & (cg[rows, cl] <= 0)
        evaluated[rows, len(centre) + cl] = True
    return touch, gap, evaluated


def pierces(scene, tris, rows, cols):
    """The independent predicate, in float64, on the pairs (query rows[i], triangle cols[i]): some edge of one triangle pierces the
    other - the closed segment against the closed triangle, Moeller-Trumbore - both ways.  (A coplanar pair pierces nothing.)"""
    t = np.ascontiguousarray(tris, F32).astype(F64)
    q = [v[rows] for v in vertices(t)]
    _, _, _, s = _records(scene, F64)
    s = [v[cols] for v in s]

    def hit(p, d, a, e1, e2):
        with np.errstate(all="ignore"):
            h = np.cross(d, e2)
            det = (e1 * h).sum(-1)
            sv = p - a
            u = (sv * h).sum(-1) / det
            qv = np.cross(sv, e1)
            v, w = (d * qv).sum(-1) / det, (e2 * qv).sum(-1) / det
            return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (w >= 0) & (w <= 1)

    out = np.zeros(len(rows), bool)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        out |= hit(q[i], q[j] - q[i], s[0], s[1] - s[0], s[2] - s[0])
        out |= hit(s[i], s[j] - s[i], q[0], q[1] - q[0], q[2] - q[0])
    return out


# -- case makers ----------------------------------------------------------------------------------------------------------------------
SOUP_SIZES = np.array([0.05, 0.4, 1.2, 3.0])


def soup_triangles(scene, n, seed):
    """n triangles centred on closest_point_cases.four_kinds; vertex k = centre + (uniform[0, 1)^3 - 0.5) x size, size cycling through
    (0.05, 0.4, 1.2, 3.0) by index."""
    centre = cc.four_kinds(scene, n, seed).astype(F64)
    offset = (np.random.default_rng(seed).random((n, 3, 3)) - 0.5) * SOUP_SIZES[np.arange(n) % 4][:, None, None]
    v = (centre[:, None, :] + offset).astype(F32)
    return make_triangles(v[:, 0], v[:, 1], v[:, 2])


LATTICE = (np.arange(0.0, 2.51, 0.5), np.array([0.0, 0.5, 1.0]), np.array([-0.5, 0.0, 0.5, 1.0]))


def lattice_triangles(n=4096, seed=5):
    """Triangles on closest_point_all_cases.coplanar_walls() whose vertices are drawn from the lattice {0, 0.5 .. 2.5} x {0, 0.5, 1} x
    {-0.5, 0, 0.5, 1}: in the walls' planes, on their shared edges and corners, through them and beside them, segments and points
    among them (a repeated vertex).  Everything is exact in f32."""
    rng = np.random.default_rng(seed)
    v = np.stack([LATTICE[a][rng.integers(0, len(LATTICE[a]), (n, 3))] for a in range(3)], -1)  # (n, vertex, axis)
    return make_triangles(v[:, 0], v[:, 1], v[:, 2])


def lattice_points():
    """Every lattice point as a point query, and the zero-extent boxes overlap_cases answers at the same points."""
    p = np.stack(np.meshgrid(*LATTICE, indexing="ij"), -1).reshape(-1, 3)
    return make_triangles(p, p, p), oc.make_boxes(p, 0.0)


def deck_triangles(kind, n=64):
    """The sliver inscribed in each overlap_cases.deck_boxes(kind) box - (lo, lo, lo), (hi, hi, lo), (lo, hi, hi) - long and thin
    along z with the box's bounds: through the empty corner (touches nothing, enters every card's box), through the covered half
    (touches every card), or mixed per wave."""
    b = oc.deck_boxes(kind, n)
    lo, hi = b[:, 0:3] - b[:, 4:7], b[:, 0:3] + b[:, 4:7]
    return make_triangles(lo, np.stack([hi[:, 0], hi[:, 1], lo[:, 2]], 1), np.stack([lo[:, 0], hi[:, 1], hi[:, 2]], 1))
