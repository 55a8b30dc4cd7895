"""The triangle contact query's statement (include/rt_hip.h "Triangle contacts", csrc/contact_triangle_rules.h) in numpy, and the
triangles the tests ask about.

pair_dist2() evaluates the statement's squared distance of every query triangle from every sphere and triangle of a scene: in
float32 every numpy operation is one f32 rounding, in the header's order - cp_triangle and sc_pair_edge are sweep_capsule_cases',
the order and the range closest_point_cases' - so contacts_all(), which keeps the candidates below cp_start(margin), sorts them by
(dist2 bits, key) and writes the first K as rt_triangle_contact records with miss padding, gives the bytes rt_contact_triangle must
return; in float64 (the same statement on the exact edges) it gives the distances the float32 statement is held to.  The first
k < K records of a query are the statement's at max_contacts = k (first_k).  Helpers, no tests."""
import functools

import numpy as np

import closest_point_all_cases as ca
import closest_point_cases as cc
import contact_capsule_cases as ccc
import overlap_triangle_cases as otc
import sweep_capsule_cases as scs
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

F32 = np.float32
F64 = np.float64
CONTACT_MAX = 16
PRIM_MISS = cc.PRIM_MISS
SPHERE_FLAG = cc.SPHERE_FLAG
OUT_OF_RANGE = ca.OUT_OF_RANGE
PAIRS_PER_CHUNK = 1 << 15  # query x triangle pairs evaluated at a time (the statement holds some hundred arrays of that size)

# The smallest k of the grid 1, 1.5, 2, 3, 5, 7 x 10^n at which |distance32 - distance64| <= k x the scene's diagonal holds for every
# listed contact (K = CONTACT_MAX) of soup_triangles_with_margins(scene, 2048, 11), measured on the CPU against the float64
# statement (test_contact_triangle_abi.py asserts it, and that the next smaller grid value is violated; DESIGN.md section 4
# "Triangle contacts").  The largest differences measured: soup 2.17e-7 over 13364 listed contacts, of a diagonal of 7.90
# (2.74e-8); cornell12 2.17e-7 over 3358, of 3.46 (6.27e-8).
K_MEASURED = {"soup": 3e-8, "cornell12": 7e-8}
# The bound, in diagonals, on the f32 distance here of every pair the f32 overlap statement (overlap_triangle_cases.touching) lists,
# measured the same way on the soup batch: all 8187 touching pairs are at distance 0 exactly - an edge passes through the other
# triangle (rule d) or a sphere is crossed - so the smallest bound that holds is 0 itself, below every value of the grid.
K_TOUCH = {"soup": 0.0}

_dot = cc._dot
_cross = scs._cross
_order = cc._order
_cp_tri = scs._cp_tri
_pair_edge = scs._pair_edge
_clamp01 = scs._clamp01
records = cc.records
diagonal = cc.diagonal
keys = ccc.keys
columns = ccc.columns
_spheres = ccc._spheres


# -- the statement ------------------------------------------------------------------------------------------------------------------
def make_contact_triangles(v0, v1, v2, margin):
    """(N, 3) vertices and margins (a scalar or (N,)) -> (N, 12) float32 rt_triangle_contact_query records."""
    out = otc.make_triangles(v0, v1, v2)
    out[:, 3] = np.asarray(margin, F32)
    return out


def with_margin(tris, margin):
    """rt_query_triangle records with the margin written where _pad0 is."""
    out = np.array(tris, F32)
    out[:, 3] = np.asarray(margin, F32)
    return out


def valid(tris):
    """The queries that walk: finite vertices, margin > 0 (inf allowed)."""
    t = np.asarray(tris)
    with np.errstate(all="ignore"):
        return np.isfinite(t[:, 0:3]).all(1) & np.isfinite(t[:, 4:7]).all(1) & np.isfinite(t[:, 8:11]).all(1) & (t[:, 3] > 0)


def _edge_weights(edge, t):
    """ct_edge_weights: the weights of a triangle's second and third vertex at the place t of its edge 0, 1 or 2."""
    one = t.dtype.type(1)
    return (t, np.zeros_like(t)) if edge == 0 else (np.zeros_like(t), t) if edge == 1 else (one - t, t)


def _pierce(m, ax, a, b):
    """ct_pierce -> accepted, s, fv, fw."""
    n = _cross(a, b)
    nn, hA, hB = _dot(n, n), _dot(n, m), _dot(n, m + ax)
    s = hA / (hA - hB)
    p = m + ax * s[..., None]
    fv, fw = _dot(_cross(p, b), n) / nn, _dot(_cross(a, p), n) / nn
    ok = (_dot(ax, ax) > 0) & (((hA < 0) & (hB > 0)) | ((hA > 0) & (hB < 0))) & (fv >= 0) & (fw >= 0) & (fv + fw <= 1)
    return ok, s, fv, fw


def tri_tri(v0, e1, e2, q0, q1, q2):
    """ct_triangle, operands broadcast against each other (..., 3) -> dist2, qu, qv, v, w: the header's rule 1."""
    ty = q0.dtype.type
    zero, one = ty(0), ty(1)
    with np.errstate(all="ignore"):
        u1, u2, e3 = q1 - q0, q2 - q0, e2 - e1
        u3 = u2 - u1
        nQ = _cross(u1, u2)
        area = _dot(nQ, nQ) > 0
        best, v, w = _cp_tri(e1, e2, q0 - v0)  # a.
        qu, qv = np.zeros_like(best), np.zeros_like(best)
        for k, qk in ((1, q1), (2, q2)):
            d2, cv, cw = _cp_tri(e1, e2, qk - v0)
            r = d2 < best
            best, v, w = np.where(r, d2, best), np.where(r, cv, v), np.where(r, cw, w)
            qu, qv = np.where(r, one if k == 1 else zero, qu), np.where(r, one if k == 2 else zero, qv)
        for k, sk in enumerate((v0, v0 + e1, v0 + e2)):  # b.
            d2, cu, cv = _cp_tri(u1, u2, sk - q0)
            r = area & (d2 < best)
            best, qu, qv = np.where(r, d2, best), np.where(r, cu, qu), np.where(r, cv, qv)
            v, w = np.where(r, one if k == 1 else zero, v), np.where(r, one if k == 2 else zero, w)
        axes = ((q0, u1), (q0, u2), (q1, u3))
        for i, (P, ax) in enumerate(axes):  # c.
            ap = P - v0
            m1 = ap - e1
            aa = _dot(ax, ax)
            for j, (m, e) in enumerate(((ap, e1), (ap, e2), (m1, e3))):
                d2, cs, cu = _pair_edge(m, e, ax, aa)
                r = d2 < best
                a, b = _edge_weights(i, cs)
                c, d = _edge_weights(j, cu)
                best = np.where(r, d2, best)
                qu, qv, v, w = np.where(r, a, qu), np.where(r, b, qv), np.where(r, c, v), np.where(r, d, w)
        for i, (P, ax) in enumerate(axes):  # d, the query's edges through the scene triangle
            ok, ps, fv, fw = _pierce(P - v0, ax, e1, e2)
            r = ok & (0 < best)
            a, b = _edge_weights(i, ps)
            best = np.where(r, zero, best)
            qu, qv, v, w = np.where(r, a, qu), np.where(r, b, qv), np.where(r, fv, v), np.where(r, fw, w)
        a0, a1 = v0 - q0, (v0 + e1) - q0
        for j, (m, e) in enumerate(((a0, e1), (a0, e2), (a1, e3))):  # d, the scene's edges through the query triangle
            ok, ps, fu, fv = _pierce(m, e, u1, u2)
            r = area & ok & (0 < best)
            c, d = _edge_weights(j, ps)
            best = np.where(r, zero, best)
            qu, qv, v, w = np.where(r, fu, qu), np.where(r, fv, qv), np.where(r, c, v), np.where(r, d, w)
        dt = q0.dtype
        return best.astype(dt), qu.astype(dt), qv.astype(dt), v.astype(dt), w.astype(dt)


def sphere_candidates(centre, radius, q0, q1, q2):
    """ct_sphere, operands broadcast against each other ((..., 3), radius (...)) -> dist2, qu, qv."""
    ty = q0.dtype.type
    zero, one = ty(0), ty(1)
    with np.errstate(all="ignore"):
        u1, u2 = q1 - q0, q2 - q0
        near2, qu, qv = _cp_tri(u1, u2, centre - q0)
        x2, xv, xu = _cp_tri(u2, u1, centre - q0)  # the edges exchanged where the first has no length
        exchanged = ~(_dot(u1, u1) > 0)
        near2, qu, qv = np.where(exchanged, x2, near2), np.where(exchanged, xu, qu), np.where(exchanged, xv, qv)
        far2, fu, fv = None, None, None
        for k, qk in enumerate((q0, q1, q2)):
            m = qk - centre
            d2 = _dot(m, m)
            if k == 0:
                far2, fu, fv = d2, np.zeros_like(d2), np.zeros_like(d2)
            else:
                r = d2 > far2
                far2, fu, fv = np.where(r, d2, far2), np.where(r, one if k == 1 else zero, fu), np.where(r, one if k == 2 else zero, fv)
        dn, df = np.sqrt(near2), np.sqrt(far2)
        pn = q0 + (u1 * qu[..., None] + u2 * qv[..., None])
        pf = np.where((fu != 0)[..., None], q1, np.where((fv != 0)[..., None], q2, q0))
        ax, mA = pf - pn, pn - centre
        aa, b, c = _dot(ax, ax), _dot(mA, ax), _dot(mA, mA) - radius * radius
        disc = b * b - aa * c
        sq = np.where(disc > 0, np.sqrt(disc), zero)
        s = np.where(aa > 0, _clamp01((sq - b) / aa), zero)
        outside = dn > radius
        inside = ~outside & (df < radius)
        crossing = ~outside & ~inside & (dn <= radius) & (radius <= df)
        d = np.where(outside, dn - radius, np.where(inside, radius - df, np.where(crossing, zero, ty(np.nan))))
        cu, cv = qu + (fu - qu) * s, qv + (fv - qv) * s
        qu = np.where(outside, qu, np.where(inside, fu, np.where(crossing, cu, qu)))
        qv = np.where(outside, qv, np.where(inside, fv, np.where(crossing, cv, qv)))
        dt = q0.dtype
        return (d * d).astype(dt), qu.astype(dt), qv.astype(dt)


def sphere_position(centre, radius, q0, q1, q2, qu, qv):
    """ct_sphere_position: cp_sphere's point from q0 + (u1 qu + u2 qv), elementwise (..., 3)."""
    with np.errstate(all="ignore"):
        p = q0 + ((q1 - q0) * qu[..., None] + (q2 - q0) * qv[..., None])
        oc = p - centre
        length = np.sqrt(_dot(oc, oc))
        at_centre = np.zeros_like(oc)
        at_centre[..., 0] = radius
        return np.where((length > 0)[..., None], centre + oc * (radius / length)[..., None], centre + at_centre).astype(q0.dtype)


def _vertices(tris, dtype):
    t = np.ascontiguousarray(tris, F32).astype(dtype)
    return np.ascontiguousarray(t[:, 0:3]), np.ascontiguousarray(t[:, 4:7]), np.ascontiguousarray(t[:, 8:11])


def pair_dist2(scene, tris, dtype=F32):
    """(N, 12) float32 queries -> dist2 (N, n_spheres + n_triangles) in `dtype` (float32: on the stored f32 edges; float64: on the
    exact ones): the spheres' columns first, then the triangles' by index.  A NaN where the statement gives one."""
    v0, e1, e2, _ = records(scene, dtype)
    centre, radius = _spheres(scene, dtype)
    q0, q1, q2 = _vertices(tris, dtype)
    out = np.zeros((len(q0), len(centre) + len(v0)), dtype)
    step = max(1, PAIRS_PER_CHUNK // max(out.shape[1], 1))
    for lo in range(0, len(q0), step):
        sl = slice(lo, lo + step)
        if len(centre):
            out[sl, :len(centre)] = sphere_candidates(centre[None], radius[None], q0[sl, None, :], q1[sl, None, :], q2[sl, None, :])[0]
        if len(v0):
            out[sl, len(centre):] = tri_tri(v0[None], e1[None], e2[None], q0[sl, None, :], q1[sl, None, :], q2[sl, None, :])[0]
    return out


def in_range(tris, d2):
    """(N, P) bool: the pairs the statement lists or counts, from pair_dist2's float32 matrix."""
    tris = np.ascontiguousarray(tris, F32)
    with np.errstate(all="ignore"):
        mm = tris[:, 3] * tris[:, 3]
        return (d2 < mm[:, None]) & valid(tris)[:, None]


def contacts_all(scene, tris, k=CONTACT_MAX, d2=None):
    """(N, 12) float32 queries -> records (N, k, 8) float32, listed counts (N,) uint32 = min(total, k), total counts (N,) uint32 =
    the candidates in range (what RT_QUERY_COUNT_ALL reports).  d2: pair_dist2(scene, tris) where the caller has it."""
    tris = np.ascontiguousarray(tris, F32)
    n = len(tris)
    d2 = pair_dist2(scene, tris) if d2 is None else d2
    key, material = keys(scene)
    n_sph = len(scene.spheres)
    out = np.zeros((n, k), T.TRIANGLE_CONTACT)
    out["distance"] = tris[:, 3, None]
    out["prim_id"] = PRIM_MISS
    if d2.shape[1] == 0:
        return out.view(F32).reshape(n, k, 8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    listed_pairs = in_range(tris, d2)
    total = listed_pairs.sum(1).astype(np.uint32)
    order = np.where(listed_pairs, _order(d2, np.broadcast_to(key, d2.shape)), OUT_OF_RANGE)
    first = np.argsort(order, 1, kind="stable")[:, :k]  # (n, <= k) columns, ascending order
    rows = np.arange(n)[:, None]
    listed = np.take_along_axis(listed_pairs, first, 1)
    kk = first.shape[1]
    q0, q1, q2 = (np.broadcast_to(tris[:, None, c:c + 3], (n, kk, 3)) for c in (0, 4, 8))
    is_tri = first >= n_sph
    rec = np.zeros(first.shape, T.TRIANGLE_CONTACT)
    pos, qu, qv = np.zeros((n, kk, 3), F32), np.zeros((n, kk), F32), np.zeros((n, kk), F32)
    v0, e1, e2, _ = records(scene)
    if len(v0):  # the listed entries once more, for the weights and the point
        t = np.where(is_tri, first - n_sph, 0)
        _, tu, tv, sv, sw = tri_tri(v0[t], e1[t], e2[t], q0, q1, q2)
        with np.errstate(all="ignore"):
            tpos = v0[t] + (e1[t] * sv[..., None] + e2[t] * sw[..., None])
        pos, qu, qv = np.where(is_tri[..., None], tpos, pos), np.where(is_tri, tu, qu), np.where(is_tri, tv, qv)
    if n_sph:
        centre, radius = _spheres(scene, F32)
        i = np.where(is_tri, 0, first)
        _, su, sv = sphere_candidates(centre[i], radius[i], q0, q1, q2)
        spos = sphere_position(centre[i], radius[i], q0, q1, q2, su, sv)
        pos, qu, qv = np.where(is_tri[..., None], pos, spos), np.where(is_tri, qu, su), np.where(is_tri, qv, sv)
    rec["position"], rec["qu"], rec["qv"] = pos, qu, qv
    with np.errstate(all="ignore"):
        rec["distance"] = np.sqrt(d2[rows, first])
    rec["prim_id"] = (key[first] ^ np.uint64(SPHERE_FLAG)).astype(np.uint32)
    rec["material_id"] = material[first]
    out[:, :kk] = np.where(listed, rec, out[:, :kk])
    return out.view(F32).reshape(n, k, 8), np.minimum(total, k).astype(np.uint32), total


def first_k(recs, total, k):
    """The statement at max_contacts = k from contacts_all's at a larger one: (records (N, k, 8), listed counts)."""
    return np.ascontiguousarray(recs[:, :k]), np.minimum(total, k).astype(np.uint32)


# -- the batches --------------------------------------------------------------------------------------------------------------------
SOUP_MARGINS = (0.01, 0.5)  # log-uniform: chosen on the CPU so that batch_condition holds on soup() at K = 4 and K = 16


def soup_triangles_with_margins(scene, n, seed, margins=SOUP_MARGINS):
    """overlap_triangle_cases.soup_triangles' triangles (sizes 0.05 to 3.0) with margins log-uniform in `margins`."""
    rng = np.random.default_rng(seed + 91)
    return with_margin(otc.soup_triangles(scene, n, seed), np.exp(rng.uniform(np.log(margins[0]), np.log(margins[1]), n)))


def batch_condition(total, k):
    """The fractions of queries with some but fewer than k contacts, with more than k, and with none: the soup batch needs > 5 %,
    > 5 % and > 0 at k = 4 and k = 16."""
    total = np.asarray(total)
    return float(((total > 0) & (total < k)).mean()), float((total > k).mean()), float((total == 0).mean())


def small_triangles(scene, n, seed):
    """Small triangles near surfaces: edges of about 0.1, margin 0.03 - what a walk that culls answers with a few triangle tests."""
    centre = cc.near_surface(scene, n, seed, sigma=0.02).astype(F64)
    offset = (np.random.default_rng(seed + 92).random((n, 3, 3)) - 0.5) * 0.1
    v = (centre[:, None, :] + offset).astype(F32)
    return make_contact_triangles(v[:, 0], v[:, 1], v[:, 2], 0.03)


def lattice_triangles(n=1024, seed=5):
    """overlap_triangle_cases.lattice_triangles on closest_point_all_cases.coplanar_walls() - vertices on the half-integer lattice,
    in the walls' planes (distance 0 without piercing), through them, parallel above them, every eighth a segment and every eighth a
    point - with
    margins 0.75 and 1.25 in turn: everything is exact in f32, equal distances tie bit for bit and the key decides."""
    tris = with_margin(otc.lattice_triangles(n, seed), np.where(np.arange(n) % 2 == 0, 0.75, 1.25))
    kind = np.arange(n) % 8
    tris[kind == 5, 8:11] = tris[kind == 5, 4:7]  # every eighth a segment, given as v2 == v1
    tris[kind == 6, 4:7] = tris[kind == 6, 8:11] = tris[kind == 6, 0:3]  # and every eighth a point
    return tris


def deck_triangles(kind, n=64):
    """overlap_triangle_cases.deck_triangles' slivers on stack_cases.deck_scene() with a small margin: `corner` through the empty
    corner (nothing in range, every card's box entered), `covered` through every card (distance 0, the lowest keys listed), `mixed`
    per wave."""
    import stack_cases as sk
    return with_margin(otc.deck_triangles(kind, n), sk.MARGIN / 16)


# -- shared references: computed once per process, never modified -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@functools.lru_cache(maxsize=None)
def soup_reference(n=2048, seed=11):
    """(queries, dist2 (N, P) float32, records (N, CONTACT_MAX, 8), total (N,)) of soup_triangles_with_margins(soup(), n, seed)."""
    tris = soup_triangles_with_margins(soup(), n, seed)
    d2 = pair_dist2(soup(), tris)
    recs, _, total = contacts_all(soup(), tris, CONTACT_MAX, d2)
    for a in (tris, d2, recs, total):
        a.setflags(write=False)
    return tris, d2, recs, total
