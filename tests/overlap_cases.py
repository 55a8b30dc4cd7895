"""The overlap query's statement (include/rt_hip.h "Overlap queries", csrc/overlap_rules.h) in numpy, and the boxes the tests ask about.

touching() evaluates the float32 statement for every box against every triangle record and sphere of a scene, in chunks - every numpy
operation is one f32 rounding, in the header's order - and overlap_all() turns it into the ids and counts rt_overlap_box must return,
byte for byte; first_k gives the statement at a smaller max_prims.  margins() is the same statement in float64 on the exact edges with
a signed, scaled margin per pair, which the float32 statement is held to away from zero.  Helpers, no tests."""
import numpy as np

import closest_point_all_cases as ca
import closest_point_cases as cc
import stack_cases as sc

F32 = np.float32
F64 = np.float64
OVERLAP_MAX = 32
PRIM_MISS = cc.PRIM_MISS
SPHERE_FLAG = cc.SPHERE_FLAG
PAIRS_PER_CHUNK = 1 << 19  # box x primitive pairs evaluated at a time
FLT_MAX = np.finfo(F32).max


def make_boxes(center, half_extent):
    """(N, 8) float32 rt_box records: cx cy cz 0 hx hy hz 0."""
    c = np.asarray(center, F32).reshape(-1, 3)
    out = np.zeros((len(c), 8), F32)
    out[:, 0:3] = c
    out[:, 4:7] = np.asarray(half_extent, F32)
    return out


def valid(boxes):
    """Which queries are not degenerate: finite centre and half extent, half extent >= 0."""
    c, h = boxes[:, 0:3], boxes[:, 4:7]
    with np.errstate(all="ignore"):
        return np.isfinite(c).all(1) & np.isfinite(h).all(1) & (h >= 0).all(1)


def _span(p, r):
    """p (..., 3) over the vertices, r (...): min_k p_k <= r && max_k p_k >= -r, and (p_0 + p_1) + p_2 is not a NaN."""
    s = (p[..., 0] + p[..., 1]) + p[..., 2]
    lo = np.fmin(np.fmin(p[..., 0], p[..., 1]), p[..., 2])
    hi = np.fmax(np.fmax(p[..., 0], p[..., 1]), p[..., 2])
    return (lo <= r) & (hi >= -r) & (s == s)


def _cross_axes(f, a, h):
    """f (n, 3) an edge per record, a (m, n, 3 vertices, 3 axes), h (m, 1, 3) -> (m, n) bool: the three axes cross(unit_i, f)."""
    g = np.abs(f)
    fx, fy, fz = f[None, :, None, 0], f[None, :, None, 1], f[None, :, None, 2]
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    hx, hy, hz = h[..., 0], h[..., 1], h[..., 2]
    ok = _span(fy * az - fz * ay, g[None, :, 2] * hy + g[None, :, 1] * hz)
    ok &= _span(fz * ax - fx * az, g[None, :, 2] * hx + g[None, :, 0] * hz)
    ok &= _span(fx * ay - fy * ax, g[None, :, 1] * hx + g[None, :, 0] * hy)
    return ok


def triangle_families(v0, e1, e2, c, h):
    """c, h (m, 3) against n records -> four (m, n) bool arrays, in the arrays' dtype: the vertices are finite, and no axis of the
    family separates - the three box axes, the normal, the nine cross axes.  A triangle touches iff all four hold."""
    with np.errstate(all="ignore"):
        cc_, hh = c[:, None, :], h[:, None, :]
        a = np.stack([v0[None] - cc_, (v0 + e1)[None] - cc_, (v0 + e2)[None] - cc_], 2)  # (m, n, vertex, axis)
        finite = (np.abs(a) <= np.finfo(a.dtype).max).all((2, 3))
        box = ((np.fmin(np.fmin(a[:, :, 0], a[:, :, 1]), a[:, :, 2]) <= hh) & (np.fmax(np.fmax(a[:, :, 0], a[:, :, 1]), a[:, :, 2]) >= -hh)).all(2)
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        d, r = cc._dot(n[None], a[:, :, 0]), cc._dot(np.abs(n)[None], hh)
        normal = (d <= r) & (d >= -r)
        cross = _cross_axes(e1, a, hh) & _cross_axes(e2 - e1, a, hh) & _cross_axes(e2, a, hh)
        return finite, box, normal, cross


def triangle_touches(v0, e1, e2, c, h):
    """c, h (m, 3) against n records -> (m, n) bool, in the arrays' dtype (float32: the bits of ov_triangle)."""
    finite, box, normal, cross = triangle_families(v0, e1, e2, c, h)
    return finite & box & normal & cross


def sphere_touches(centre, radius, c, h):
    """c, h (m, 3) against s spheres -> (m, s) bool."""
    with np.errstate(all="ignore"):
        g = np.abs(centre[None] - c[:, None, :])
        near, far = np.fmax(g - h[:, None, :], g.dtype.type(0)), g + h[:, None, :]
        rr = (radius * radius)[None]
        return (cc._dot(near, near) <= rr) & (cc._dot(far, far) >= rr)


def _scene_arrays(scene, dtype=F32):
    v0, e1, e2, _ = cc.records(scene, dtype)
    sph = scene.spheres
    return v0, e1, e2, np.ascontiguousarray(sph["center"], F32).reshape(-1, 3).astype(dtype), sph["radius"].astype(F32).astype(dtype)


def touching(scene, boxes):
    """(N, 8) float32 boxes -> (N, n_spheres + n_triangles) bool in key order: the spheres' columns, then the triangles'."""
    boxes = np.ascontiguousarray(boxes, F32)
    v0, e1, e2, centre, radius = _scene_arrays(scene)
    n, cols = len(boxes), len(centre) + len(v0)
    out = np.zeros((n, cols), bool)
    ok = valid(boxes)
    step = max(1, PAIRS_PER_CHUNK // max(cols, 1))
    for lo in range(0, n, step):
        c, h = boxes[lo:lo + step, 0:3], boxes[lo:lo + step, 4:7]
        parts = []
        if len(centre):
            parts.append(sphere_touches(centre, radius, c, h))
        if len(v0):
            parts.append(triangle_touches(v0, e1, e2, c, h))
        if parts:
            out[lo:lo + step] = np.concatenate(parts, 1) & ok[lo:lo + step, None]
    return out


def prim_ids(scene):
    """The id (rt_hit.prim_id's encoding) of each column of touching()."""
    return np.concatenate([np.arange(len(scene.spheres), dtype=np.uint32) | np.uint32(SPHERE_FLAG), np.arange(len(scene.triangles), dtype=np.uint32)])


def overlap_all(scene, boxes, k=OVERLAP_MAX, touch=None):
    """-> ids (N, k) uint32 (ascending key, then PRIM_MISS), listed counts (N,) uint32 = min(total, k), total counts (N,) uint32."""
    t = touching(scene, boxes) if touch is None else touch
    ids = prim_ids(scene)
    total = t.sum(1).astype(np.uint32)
    out = np.full((len(t), k), PRIM_MISS, np.uint32)
    rank = np.cumsum(t, 1) - 1  # the columns are in key order already
    rows, cols = np.nonzero(t & (rank < k))
    out[rows, rank[rows, cols]] = ids[cols]
    return out, np.minimum(total, k).astype(np.uint32), total


def first_k(ids, total, k):
    """The statement at max_prims = k from overlap_all's at a larger one: (ids (N, k), listed counts)."""
    return np.ascontiguousarray(ids[:, :k]), np.minimum(total, k).astype(np.uint32)


# -- the float64 statement with a margin --------------------------------------------------------------------------------------------
def _axis_margin(p, r, scale):
    with np.errstate(all="ignore"):
        return np.minimum(r - p.min(-1), p.max(-1) + r) / np.where(scale > 0, scale, 1.0)


def margins(scene, boxes):
    """(N, n_spheres + n_triangles) float64: the statement on the exact edges with a signed margin per pair.  Per axis the margin is
    min(r - pmin, pmax + r) over a scale of the magnitudes that entered it - (|c| + h + |a|), maxima over components and vertices,
    times the axis' largest component - and the pair's margin is the minimum over its axes: the pair touches iff it is >= 0.  A sphere:
    min(rr - near^2, far^2 - rr) over the square of (|c| + h + |centre| + radius).  Degenerate queries and non-finite triangles are
    not handled: the caller passes ordinary input."""
    boxes = np.ascontiguousarray(boxes, F32).astype(F64)
    v0, e1, e2, centre, radius = _scene_arrays(scene, F64)
    n = len(boxes)
    out = np.zeros((n, len(centre) + len(v0)), F64)
    step = max(1, (PAIRS_PER_CHUNK // 4) // max(out.shape[1], 1))
    nrm = np.cross(e1, e2)
    for lo in range(0, n, step):
        c, h = boxes[lo:lo + step, 0:3], boxes[lo:lo + step, 4:7]
        cm, hm = np.abs(c).max(1)[:, None], h.max(1)[:, None]
        if len(centre):
            g = np.abs(centre[None] - c[:, None, :])
            near, far = np.maximum(g - h[:, None, :], 0.0), g + h[:, None, :]
            rr = (radius * radius)[None]
            scale = cm + hm + np.abs(centre).max(1)[None] + radius[None]
            out[lo:lo + step, :len(centre)] = np.minimum(rr - (near * near).sum(-1), (far * far).sum(-1) - rr) / (scale * scale)
        if len(v0):
            cc_, hh = c[:, None, :], h[:, None, :]
            a = np.stack([v0[None] - cc_, (v0 + e1)[None] - cc_, (v0 + e2)[None] - cc_], 2)  # (m, n, vertex, axis)
            mag = cm + hm + np.abs(a).max((2, 3))
            m = np.full(a.shape[:2], np.inf)
            for ax in range(3):
                m = np.minimum(m, _axis_margin(a[..., ax], hh[..., ax], mag))
            axes = [nrm] + [np.cross(np.eye(3)[i][None], f) for f in (e1, e2 - e1, e2) for i in range(3)]
            for x in axes:
                p = (a * x[None, :, None, :]).sum(-1)
                r = (np.abs(x)[None] * hh).sum(-1)
                m = np.minimum(m, _axis_margin(p, r, mag * np.abs(x).max(1)[None]))
            out[lo:lo + step, len(centre):] = m
    return out


# -- case makers ----------------------------------------------------------------------------------------------------------------------
SOUP_EXTENT = np.array([1.0, 0.5, 1.5], F32)
SOUP_SIZES = np.array([0.02, 0.08, 0.25, 0.6], F32)


def soup_boxes(scene, n, seed):
    """n boxes centred on closest_point_cases.four_kinds, half extents (1, 0.5, 1.5) x {0.02, 0.08, 0.25, 0.6} by index."""
    return make_boxes(cc.four_kinds(scene, n, seed), SOUP_EXTENT[None] * SOUP_SIZES[np.arange(n) % 4][:, None])


def lattice_boxes():
    """Boxes on closest_point_all_cases.coplanar_walls() whose faces, edges and corners lie exactly in the walls' planes, on their
    shared edges and on their shared corners: centres on the half-integer lattice over the walls, half extents 0.5 and 0.25 (all
    exact in f32), flat boxes in the planes themselves, segments along shared edges and points on shared corners."""
    boxes = []
    for hx in (0.5, 0.25):
        for x in np.arange(-0.5, 3.01, 0.5):
            for y in (-0.5, 0.0, 0.5, 1.0, 1.5):
                for z in (-0.5, 0.0, 0.5, 1.5):
                    boxes.append(((x, y, z), (hx, hx, hx)))
    for x in (0.0, 0.5, 1.0, 1.5, 2.0):
        boxes.append(((x, 0.5, 0.0), (0.25, 0.5, 0.0)))    # flat, in the floor's plane
        boxes.append(((x, 0.5, 0.5), (0.0, 0.5, 0.5)))     # flat, parallel to the wall (in its plane at x = 2)
        boxes.append(((x, 0.5, 0.0), (0.0, 0.75, 0.0)))    # a segment in the floor, along the shared edge at x = 1
        for y in (0.0, 1.0):
            for z in (0.0, 1.0):
                boxes.append(((x, y, z), (0.0, 0.0, 0.0)))  # points: the walls' corners among them
    c, h = zip(*boxes)
    return make_boxes(np.array(c, F32), np.array(h, F32))


def deck_boxes(kind, n=64):
    """Boxes on stack_cases.deck_scene(), long and thin along z over the deck's whole length:
      corner    through the empty corner x + y >= MARGIN: enters every card's box and touches none
      covered   through the covered half: touches every card
      mixed     stack_cases.mixed_covered per wave
    The thin half extent is a quarter of MARGIN / 2, so that a box stays on its side of the hypotenuse whatever the jitter."""
    rng = np.random.default_rng(sc.SEED + 9)
    covered = {"corner": np.zeros(n, bool), "covered": np.ones(n, bool), "mixed": sc.mixed_covered(n)}[kind]
    thin = sc.MARGIN / 8
    cov, emp = sc._region_points(rng, n, True), sc._region_points(rng, n, False)
    # keep the whole cross-section inside the region and inside every card's box
    cov, emp = np.clip(cov, -sc.INSIDE + thin, sc.INSIDE - thin), np.clip(emp, -sc.INSIDE + thin, sc.INSIDE - thin)
    xy = np.where(covered[:, None], cov - thin, emp + thin)
    centre = np.concatenate([xy, np.full((n, 1), sc.Z_FRONT - sc.Z_LENGTH / 2)], 1)
    return make_boxes(centre, (thin, thin, sc.Z_LENGTH / 2 + 0.5))
